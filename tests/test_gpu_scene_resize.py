"""The resized load on the GPU (tf_map_load_resized and the layers above it, topfusion_amd/csrc/tf_scene_ckpt.hip): a map
checkpoint into a context of other capacities, against the serial restatement (tests/scene_resize_ref.py) bit for bit,
its refusals, and as a resumed sequence -- a context of more blocks, more excess slots or another hash size that loads
a map holds the map that was saved."""
import numpy as np
import pytest

import scene_map_ref as MR
import scene_resize_ref as Z
import test_gpu_scene_ckpt as C
import test_gpu_scene_map as T
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

W, H = T.W, T.H


# ---- 1. against the restatement ------------------------------------------------------------------------------------------
def _ctx(swapping, **kw):
    return T._ctx(swapping, voxel_rgb=0 if swapping else 1, **kw)


_files = {}


def _made_file(tmp_path_factory, swapping):
    """(path, the saving context's state) of the made map of either version, saved once."""
    if swapping not in _files:
        g = _ctx(swapping, **Z.MADE)
        s = Z.made_state(swapping)
        (T._upload_map if swapping else C._upload_state)(g, s)
        path = tmp_path_factory.mktemp("resize") / f"made{int(swapping)}.tfmap"
        g.save_map(path)
        _files[swapping] = (path, T._state(g))
        g.close()
    return _files[swapping]


def _assert_resized(tag, got, want, swapping):
    for k in ("hash", "visType", "vba", "allocList", "excessList", "pose"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (tag, k)
    assert got["counters"] == want["counters"], (tag, got["counters"], want["counters"])
    n = want["counters"]["noVisibleEntries"]
    assert np.asarray(got["visibleIds"])[:n].tobytes() == want["visibleIds"].tobytes(), (tag, "visibleIds")
    assert all(np.asarray(a, np.float32).tobytes() == b.tobytes() for a, b in zip(got["maps"], want["maps"])), (tag, "maps")
    if not swapping:
        assert got["rgb"].tobytes() == want["rgb"].tobytes(), (tag, "rgb")
        return
    for k in ("swapState", "swapFlags"):
        assert got[k].tobytes() == want[k].tobytes(), (tag, k)
    ids = np.flatnonzero(want["swapFlags"] == 1)
    assert got["store"].reshape(-1, 512)[ids].tobytes() == want["store"].reshape(-1, 512)[ids].tobytes(), (tag, "store")


def _bytes(g):
    """Everything the download entry points give, as bytes."""
    s = T._state(g)
    out = {k: np.ascontiguousarray(v).tobytes() for k, v in s.items() if isinstance(v, np.ndarray) and k != "params"}
    out["maps"] = b"".join(np.ascontiguousarray(m).tobytes() for m in s["maps"])
    out["counters"] = s["counters"]
    return out


@pytest.mark.parametrize("n_buckets", Z.MADE_TARGET_BUCKETS)
@pytest.mark.parametrize("swapping", [True, False])
def test_against_restatement(tmp_path_factory, swapping, n_buckets):
    """The made map (version 2) and the made colour scene (version 1) into n_buckets' = file / 4, the file's, file x 4,
    each with n_blocks' = B exactly, the file's, twice the file's and n_excess' = X exactly (with a vis_capacity' below
    the visible count) or generous: every downloaded table and counter is resize()'s, the report too; a second load
    leaves the same bytes."""
    path, sa = _made_file(tmp_path_factory, swapping)
    need = Z.needs(sa, n_buckets)
    B, X = need["blocks"], need["excess_used"]
    assert B > 256 and X > 0 and X % 16 == 0 and need["records_dropped"] > 0
    rec = MR.records_of(sa)
    visible = int(((rec["visType"] > 0) & (rec["entry"]["ptr"] >= -1)).sum())
    for n_blocks in (B, Z.MADE["n_blocks"], 2 * Z.MADE["n_blocks"]):
        for n_excess, vis_capacity in ((X, 100), (X + 208, 4096)):
            assert vis_capacity == 4096 or vis_capacity < visible
            tag = (n_buckets, n_excess, n_blocks)
            g = _ctx(swapping, n_buckets=n_buckets, n_excess=n_excess, n_blocks=n_blocks, vis_capacity=vis_capacity)
            want, report = Z.resize(sa, n_buckets, n_excess, n_blocks, vis_capacity)
            assert g.load_map_resized(path) == report == need, tag
            _assert_resized(tag, T._state(g), want, swapping)
            if n_blocks == B:
                assert want["counters"]["lastFreeBlockId"] == -1
            if n_excess == X:
                assert want["counters"]["lastFreeExcessListId"] == -1 and want["counters"]["noVisibleEntries"] == vis_capacity
            first = _bytes(g)
            assert g.load_map_resized(path) == report
            assert _bytes(g) == first, tag
            if swapping:
                assert g.swap_counts() == (0, 0, 0)
            g.close()


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------
def _stale(g):
    """Flags, states and stored blocks over the whole cache of a swapping context."""
    from topfusion_amd import _lib as L
    n_total = g.params_.n_buckets + g.params_.n_excess
    rng = np.random.default_rng(n_total)
    g.upload(L.TF_BUF_SWAP_STORED_FLAGS, rng.integers(0, 2, n_total).astype(np.uint8))
    g.upload(L.TF_BUF_SWAP_STATE, rng.integers(0, 3, n_total).astype(np.uint8))
    g.upload(L.TF_BUF_SWAP_STORED, rng.integers(0, 1 << 24, n_total * 512, dtype=np.uint32))


def test_refusals(tmp_path_factory, tmp_path):
    from topfusion_amd import TfError, _lib as L
    path, sa = _made_file(tmp_path_factory, True)
    path1, _ = _made_file(tmp_path_factory, False)
    nb = Z.MADE["n_buckets"]
    need = Z.needs(sa, nb)
    B, X = need["blocks"], need["excess_used"]
    short = Z.needs(sa, Z.MADE_SHORT_BUCKETS)                   # (n_buckets + X - 1) % 16 == 0 there: such a context exists
    truncated = tmp_path / "truncated.tfmap"
    truncated.write_bytes(path.read_bytes()[:-1])
    generous = dict(n_buckets=nb, n_excess=X + 208, n_blocks=2 * Z.MADE["n_blocks"])

    def refused(g, file, status, report=None):
        before = _bytes(g)
        with pytest.raises(TfError) as e:
            g.load_map_resized(file)
        assert e.value.status == status, (e.value.status, status)
        assert e.value.report == report
        assert _bytes(g) == before

    # capacity: one block, one excess slot too few; the report says what is needed
    for kw, want in ((dict(generous, n_blocks=B - 1), need), (dict(generous, n_blocks=B - 1, n_excess=X), need),
                     (dict(n_buckets=Z.MADE_SHORT_BUCKETS, n_excess=short["excess_used"] - 1, n_blocks=B), short)):
        g = _ctx(True, **kw)
        _stale(g)
        refused(g, path, L.TF_CAPACITY, want)
        g.close()
    g = _ctx(True, n_buckets=Z.MADE_SHORT_BUCKETS, n_excess=short["excess_used"] + 15, n_blocks=B)     # ... and fits with them
    assert g.load_map_resized(path) == short
    g.close()
    # a context that holds the map and a stale cache: a truncated file, the other version, the strict load
    g = _ctx(True, **generous)
    g.load_map_resized(path)
    _stale(g)
    refused(g, truncated, L.TF_INVALID_ARG)
    refused(g, path1, L.TF_INVALID_ARG)
    refused(g, tmp_path / "missing.tfmap", L.TF_INVALID_ARG)
    before = _bytes(g)
    assert C._status(g.load_map, path) == L.TF_INVALID_ARG      # capacities differ: the strict load still refuses
    assert _bytes(g) == before
    g.close()
    # parameter mismatches
    for kw in (dict(voxelSize=0.006), dict(cols=W + 4), dict(mu=0.03)):
        g = _ctx(True, **dict(generous, **kw))
        _stale(g)
        refused(g, path, L.TF_INVALID_ARG)
        g.close()
    g = _ctx(False, **generous)                                 # version 2 into a context without swapping (colour: voxel_rgb too)
    refused(g, path, L.TF_INVALID_ARG)
    g.close()
    g = T._ctx(False, **generous)
    refused(g, path, L.TF_INVALID_ARG)
    refused(g, path1, L.TF_INVALID_ARG)                         # voxel_rgb differs
    g.close()


# ---- 3, 4, 6. the tracked twin: TopFu::operator() over the 320 x 240 orbit ------------------------------------------------
TW, TH = 320, 240
N_SAVE, N_MORE = 5, 4
# test_gpu_scene_map.TRACKED's tables (4096 buckets, 512 excess slots, 4096 blocks) hold the 320 x 240 orbit without an
# allocation failure at 15 mm voxels (at TRACKED's own 7.5 mm the excess list runs out) -- asserted on A, not assumed
TRACKED_VOXELS = dict(voxelSize=0.015, mu=0.03)


def _tracked_ctx(**kw):
    from topfusion_amd import TopFu, default_params
    fx, fy, cx, cy = synth.intrinsics(TW, TH)
    args = dict(cols=TW, rows=TH, fx=fx, fy=fy, cx=cx, cy=cy, **T.TRACKED)
    args.update(TRACKED_VOXELS)
    args.update(kw)
    return TopFu(default_params(**args))


def _position_map(g):
    """{block position -> 512 voxels} as two arrays sorted by position."""
    h, vba = g.hash(), g.vba().view(np.uint32).reshape(-1, 512)
    live = np.flatnonzero(h["ptr"] >= 0)
    pos = np.stack([h["x"][live], h["y"][live], h["z"][live]], 1).astype(np.int64)
    order = np.lexsort((pos[:, 2], pos[:, 1], pos[:, 0]))
    return pos[order].tobytes(), vba[h["ptr"][live][order]].tobytes()


def _sorted_mesh(g, whole=False):
    t = np.ascontiguousarray(g.mesh(whole=whole)).view(np.uint8).reshape(-1, 36)
    return t[np.lexsort(t.T[::-1])].tobytes()


def _observe(g):
    return dict(pose=g.getCameraPose().tobytes(), map=_position_map(g), mesh=_sorted_mesh(g), image=g.renderImage().tobytes(),
                lastFreeBlockId=g.stats()["lastFreeBlockId"])


def _render_at_pose(g):
    """renderImage at the context's pose straight after a load: the range image is not part of a checkpoint (a load
    marks it for clearing), so CreateExpectedDepths at that pose first, as a frame would have."""
    m = g.getCameraPose()
    g.stage_expected_depths(synth.world_to_camera_rt(m[:3, :3], m[:3, 3]))
    return g.renderImage().tobytes()


_tracked = {}


def _tracked_a(tmp_path_factory):
    """Context A over the orbit: the file saved after N_SAVE frames, what A showed then and after each later frame."""
    if not _tracked:
        seq = synth.orbit_sequence(N_SAVE + N_MORE, TW, TH, seed=7)
        a = _tracked_ctx()
        oks = [bool(a(seq[k])) for k in range(N_SAVE)]
        path = tmp_path_factory.mktemp("tracked") / "a.tfmap"
        a.save_map(path)
        at_save = _observe(a)
        twin = _tracked_ctx()                                    # A itself is left to its frames
        twin.load_map(path)
        at_save["image"] = _render_at_pose(twin)
        twin.close()
        later = []
        for k in range(N_SAVE, N_SAVE + N_MORE):
            ok = bool(a(seq[k]))
            later.append(dict(_observe(a), ok=ok))
        tot = a.totals()
        _tracked.update(seq=seq, path=path, oks=oks, at_save=at_save, later=later, totals=tot, n_blocks=T.TRACKED["n_blocks"])
        a.close()
    return _tracked


def test_tracked_twin_same_buckets(tmp_path_factory):
    """B has twice A's blocks and excess slots and loads A's map resized; both track N_MORE more frames: verdicts,
    poses, the map by position, the sorted mesh and renderImage agree after every frame, and B's free-block top stays
    n_blocks_B - n_blocks_A above A's.  Asserted on A: no allocation failed, and the later frames allocated."""
    a = _tracked_a(tmp_path_factory)
    assert a["totals"]["alloc_failed_type1"] == 0 and a["totals"]["alloc_failed_type2"] == 0
    assert all(a["oks"]) and a["later"][-1]["lastFreeBlockId"] < a["at_save"]["lastFreeBlockId"]
    nb = T.TRACKED["n_blocks"]
    b = _tracked_ctx(n_blocks=2 * nb, n_excess=2 * T.TRACKED["n_excess"])
    report = b.load_map_resized(a["path"])
    assert report["blocks"] == nb - 1 - a["at_save"]["lastFreeBlockId"] == report["records_carried"]
    ob = _observe(b)
    for key in ("pose", "map", "mesh"):
        assert ob[key] == a["at_save"][key], ("at the load", key)
    assert ob["lastFreeBlockId"] - a["at_save"]["lastFreeBlockId"] == nb
    shown = _tracked_ctx(n_blocks=2 * nb, n_excess=2 * T.TRACKED["n_excess"])      # (B itself is left to its frames)
    shown.load_map_resized(a["path"])
    assert _render_at_pose(shown) == a["at_save"]["image"], "the image at the load"
    shown.close()
    for i, k in enumerate(range(N_SAVE, N_SAVE + N_MORE)):
        ok = bool(b(a["seq"][k]))
        ob = _observe(b)
        assert ok == a["later"][i]["ok"], k
        for key in ("pose", "map", "mesh", "image"):
            assert ob[key] == a["later"][i][key], (k, key)
        assert ob["lastFreeBlockId"] - a["later"][i]["lastFreeBlockId"] == nb, k
    tot = b.totals()
    assert tot["alloc_failed_type1"] == 0 and tot["alloc_failed_type2"] == 0
    b.close()


@pytest.mark.parametrize("n_buckets", [1024, 16384])
def test_other_hash_size(tmp_path_factory, n_buckets):
    """A's file into 1024 and 16384 buckets: straight after the load the map by position, the sorted mesh and
    renderImage at the saved pose are A's.  (No claim about later frames: a frame allocates one new block per bucket,
    so which allocations are deferred to the next frame differs between hash sizes.)"""
    a = _tracked_a(tmp_path_factory)
    b = _tracked_ctx(n_buckets=n_buckets, n_excess=4096)
    report = b.load_map_resized(a["path"])
    assert report["blocks"] == a["n_blocks"] - 1 - a["at_save"]["lastFreeBlockId"] and report["longest_chain"] >= 1
    ob = _observe(b)
    for key in ("pose", "map", "mesh"):
        assert ob[key] == a["at_save"][key], key
    assert _render_at_pose(b) == a["at_save"]["image"]
    h = b.hash()
    assert int((h["ptr"][n_buckets:] >= -1).sum()) == report["excess_used"] > 0
    b.close()


def test_growing_out_of_failure(tmp_path):
    """A context with too few blocks fails to allocate during the orbit's first frames; its map loaded into four
    times the blocks continues without a failure."""
    seq = synth.orbit_sequence(3 + N_MORE, TW, TH, seed=7)
    small = 512
    a = _tracked_ctx(n_blocks=small)
    for k in range(3):
        a(seq[k])
    assert a.totals()["alloc_failed_type1"] > 0
    path = tmp_path / "small.tfmap"
    a.save_map(path)
    b = _tracked_ctx(n_blocks=4 * small)
    report = b.load_map_resized(path)
    assert report["blocks"] == small and b.stats()["lastFreeBlockId"] == 3 * small - 1
    assert _position_map(b) == _position_map(a)
    b.reset_totals()
    for k in range(3, 3 + N_MORE):
        b(seq[k])
    tot = b.totals()
    assert tot["alloc_failed_type1"] == 0 and tot["alloc_failed_type2"] == 0
    assert 0 <= b.stats()["lastFreeBlockId"] < 3 * small - 1       # it went on allocating, and blocks are left
    a.close()
    b.close()


# ---- 5. the swapping twin: tf_scene_fuse_frames over the turning camera -----------------------------------------------------
SWAP_T = 2048          # blocks per transfer: far above what a frame of this walk moves, so "the first T in index order" --
SWAP_SAVE = 9          # the one thing a re-hash changes -- never cuts a transfer short (asserted on A's records)


def test_swapping_twin_same_buckets(tmp_path):
    """The turning camera of test_gpu_mesh_whole fused by tf_scene_fuse_frames on a swapping context of 256 blocks; the
    map saved in mid-walk goes into twice the blocks and both fuse on: the per-frame swap counts and both tiers
    resolved by position (the sorted whole-map mesh) agree."""
    from test_gpu_mesh_whole import ANGLES, ENGINE
    from test_gpu_swapping import _yaw_pose
    n = len(ANGLES)
    poses = [_yaw_pose(deg) for deg in ANGLES]
    frames = np.stack([synth.render_depth(R, t, W, H, noise_mm=1.0, seed=1000 + k) for k, (R, t) in enumerate(poses)])
    w2c = synth.world_to_camera_rt(np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses]))
    dev = synth.DeviceStream(n, W, H)
    dev.upload(frames)
    kw = dict(ENGINE, n_blocks=256, swap_transfer_blocks=SWAP_T)
    a, b = T._ctx(**kw), T._ctx(**dict(kw, n_blocks=512))
    first = a.fuse_frames(dev.ptr, w2c[:SWAP_SAVE + 1])
    path = tmp_path / "a.tfmap"
    a.save_map(path)
    report = b.load_map_resized(path)
    assert report["cache_blocks"] > 0 and report["blocks"] > 0
    assert _sorted_mesh(b, whole=True) == _sorted_mesh(a, whole=True)
    ra = a.fuse_frames(dev.frame_ptr(SWAP_SAVE + 1), w2c[SWAP_SAVE + 1:])
    rb = b.fuse_frames(dev.frame_ptr(SWAP_SAVE + 1), w2c[SWAP_SAVE + 1:])
    for rec in (first, ra):                                      # the condition, on A
        for key in ("swapped_in", "swapped_out", "swap_realloc"):
            assert (rec[key] < SWAP_T).all(), key
        assert (rec["alloc_failed_type1"] == 0).all() and (rec["alloc_failed_type2"] == 0).all()
    assert ra["swapped_in"].sum() > 0 and ra["swapped_out"].sum() > 0        # ... and the engine did move blocks after the load
    for key in ("swapped_in", "swapped_out", "swap_realloc", "swapped_in_merged", "noVisibleEntries", "alloc_failed_type1",
                "alloc_failed_type2"):
        assert rb[key].tolist() == ra[key].tolist(), key
    assert (rb["lastFreeBlockId"] - ra["lastFreeBlockId"] == 256).all()
    ma = _sorted_mesh(a, whole=True)
    assert len(ma) > 0 and _sorted_mesh(b, whole=True) == ma
    assert _sorted_mesh(b) == _sorted_mesh(a)
    dev.free()
    a.close()
    b.close()
