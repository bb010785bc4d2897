"""Map checkpoints on the GPU (tf_map_save / tf_map_load and the layers above them, topfusion_amd/csrc/tf_scene_ckpt.hip):
the checkpoint of a swapping context, both tiers, against the numpy restatement of the version-2 file
(tests/scene_map_ref.py) byte for byte, and as a resumed sequence -- a swapping context that loads a map
checkpoint is the context that saved it, now and after further frames and engine calls, checked against twins
and against the CPU oracle that ran straight through."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_ref as M
import mesh_whole_ref as WR
import scene_ckpt_ref as R
import scene_map_ref as MR
import test_gpu_scene_ckpt as C
from parity_util import assert_bit_exact
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 72


def _ctx(swapping=True, **kw):
    from topfusion_amd import TopFu, default_params
    fx, fy, cx, cy = synth.intrinsics(W, H)
    args = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=M.VOXEL_SIZE)
    if swapping:
        args.update(use_swapping=1, swap_transfer_blocks=16)
    args.update(kw)
    return TopFu(default_params(**args))


def _state(g):
    """The context's state as scene_map_ref takes it, from the download entry points."""
    s = C._state(g)
    if g.params_.use_swapping:
        s.update(swapState=g.swap_state(), swapFlags=g.swap_stored_flags(), store=g.swap_stored().view(np.uint32))
    return s


def _upload_map(g, s):
    from topfusion_amd import _lib as L
    C._upload_state(g, s)
    g.upload(L.TF_BUF_SWAP_STATE, s["swapState"])
    g.upload(L.TF_BUF_SWAP_STORED_FLAGS, s["swapFlags"])
    g.upload(L.TF_BUF_SWAP_STORED, s["store"])


CORNERS = (0, 255, 256, M.RANDOM["n_buckets"] + M.RANDOM["n_excess"] - 1)     # of the 256-entry count groups


def _made_map():
    """mesh_whole_ref.two_tier_case() with made free lists, a visible list, counters and random maps (as
    test_gpu_scene_ckpt._made_scene), and a flag or a state at every corner of the count groups, placed so that the
    whole mesh stays the case's: an unallocated corner entry (ptr -2: never resolved) gets flag 1, state 1 and a
    random stored block, a lost one (ptr -1, flag 0) state 1; an allocated one keeps the case's bytes."""
    c = WR.two_tier_case()
    cfg = M.RANDOM
    n_total = cfg["n_buckets"] + cfg["n_excess"]
    rng = np.random.default_rng(23)
    h = c["hash"].copy()
    state, flags = c["state"].copy(), c["flags"].copy()
    store = c["store"].copy().view(np.uint32)
    for i in CORNERS:
        if h["ptr"][i] == -2:
            flags[i], state[i] = 1, 1
            store.reshape(-1, 512)[i] = rng.integers(0, 1 << 24, 512, dtype=np.uint32)
        elif h["ptr"][i] == -1 and not flags[i]:
            state[i] = 1
    vis = np.zeros(n_total, np.uint8)
    live = np.flatnonzero(h["ptr"] >= 0)
    vis[live[::4]] = 1
    vis[live[1::4]] = 3
    vis[300] = 2
    ids = live[::4].astype(np.int32)
    pose = np.eye(4, dtype=np.float32)[:3].reshape(12).copy()
    pose[[3, 7, 11]] = (0.125, -0.5, 0.75)
    return dict(hash=h, visType=vis, vba=c["vba"].copy().view(np.uint32), rgb=None, visibleIds=ids,
                allocList=rng.permutation(cfg["n_blocks"]).astype(np.int32), excessList=rng.permutation(cfg["n_excess"]).astype(np.int32),
                counters=dict(lastFreeBlockId=37, lastFreeExcessListId=400, noVisibleEntries=len(ids)), pose=pose,
                maps=C._random_maps(rng), swapState=state, swapFlags=flags, store=store)


def _save_made_map(path):
    g = _ctx(**M.RANDOM)
    _upload_map(g, _made_map())
    g.save_map(path)
    s = _state(g)
    g.close()
    return s


def _save_and_reload(path, path2):
    """(for a child process with its own chunk size) the made map saved, loaded into a fresh context, saved again"""
    _save_made_map(path)
    g = _ctx(**M.RANDOM)
    g.load_map(path)
    g.save_map(path2)
    g.close()


def test_save_against_reference(tmp_path):
    m = _made_map()
    for i in CORNERS:
        assert m["swapFlags"][i] or m["swapState"][i], i
    assert m["swapFlags"][list(CORNERS)].any()
    path = tmp_path / "made.tfmap"
    s = _save_made_map(path)
    data = path.read_bytes()
    want = MR.pack(s)
    rec = MR.records_of(s)
    b, n_cache = int((rec["entry"]["ptr"] >= 0).sum()), int((rec["hasStoredData"] == 1).sum())
    assert b > 3 and n_cache > 3 and n_cache == int(s["swapFlags"].sum())
    assert len(data) == len(want) == MR.file_size(s["params"], s["counters"], len(rec), b, n_cache)
    assert data == want
    # several chunks with a ragged last one: the knob is read at tf_create, so a fresh process.  The case holds 48
    # active and 44 flagged blocks: chunks of 3 leave the stored payload ragged, chunks of 5 both
    assert (b % 3 or n_cache % 3) and b % 5 and n_cache % 5
    for chunk in (3, 5):
        p2, p3 = tmp_path / f"chunk{chunk}.tfmap", tmp_path / f"chunk{chunk}_again.tfmap"
        env = dict(os.environ, TFUSION_CKPT_CHUNK_BLOCKS=str(chunk))
        code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_scene_map as T; "
                f"T._save_and_reload({str(p2)!r}, {str(p3)!r})")
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert p2.read_bytes() == data, f"chunks of {chunk} blocks"
        assert p3.read_bytes() == data, f"loaded and saved again in chunks of {chunk} blocks"


def _assert_state(tag, got, want):
    for k in ("hash", "visType", "vba", "excessList", "pose", "swapState", "swapFlags"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (tag, k)
    assert got["counters"] == want["counters"], tag
    live = want["counters"]["lastFreeBlockId"] + 1                       # (above the top the list is not state: scene_map_ref)
    assert got["allocList"][:live].tobytes() == want["allocList"][:live].tobytes(), (tag, "allocList")
    ids = np.flatnonzero(want["swapFlags"] == 1)
    assert got["store"].reshape(-1, 512)[ids].tobytes() == want["store"].reshape(-1, 512)[ids].tobytes(), (tag, "store")
    assert MR.states_equal(got, want), tag


def _stale_cache(g, O):
    """A used swapping context of the made map's tables: alloc / integrate / swap over a turning camera until its own
    cache holds flags, states and stored blocks, then -- so that every entry the file does not name is stale whatever
    the frames left -- flags and states set over the whole table."""
    from topfusion_amd import _lib as L
    from test_gpu_engines import Pitched, _f, _ok
    from test_gpu_swapping import _rt32, _yaw_pose
    lib = L.load()
    intr = np.array(synth.intrinsics(W, H), np.float32)
    dists = Pitched(H, W, np.float32)
    for k, deg in enumerate((0, 40, 80, 120)):
        Rm, t = _yaw_pose(deg)
        dists.put(O.compute_dists(synth.render_depth(Rm, t, W, H, noise_mm=1.0, seed=1000 + k)))
        w2c = O.rigid_inv(_rt32(Rm, t))
        _ok(lib.tf_scene_alloc(g._h, _f(intr), _f(w2c), dists.ptr, dists.step, 0, 0), "tf_scene_alloc")
        _ok(lib.tf_scene_integrate(g._h, _f(intr), _f(w2c), dists.ptr, dists.step), "tf_scene_integrate")
        g.swap()
    dists.free()
    n_total = g.params_.n_buckets + g.params_.n_excess
    assert g.swap_state().any() and (g.hash()["ptr"] >= 0).any()
    rng = np.random.default_rng(99)
    g.upload(L.TF_BUF_SWAP_STORED_FLAGS, np.ones(n_total, np.uint8))
    g.upload(L.TF_BUF_SWAP_STATE, rng.integers(0, 3, n_total).astype(np.uint8))
    g.upload(L.TF_BUF_SWAP_STORED, rng.integers(0, 1 << 24, n_total * 512, dtype=np.uint32))


@pytest.mark.parametrize("used", [False, True])
def test_load_against_reference(tmp_path, used, oracle_mod):
    """pack() of the made map, written by numpy, into a fresh context and into a used one (_stale_cache): every
    downloaded buffer is unpack()'s (the store where flagged; elsewhere what the context held before), the whole mesh
    is the two-tier case's -- grid, hash walk and cache are all in place -- and a save reproduces the file."""
    case = WR.two_tier_case()
    src = _ctx(**M.RANDOM)
    _upload_map(src, _made_map())
    data = MR.pack(_state(src))
    src.close()
    path = tmp_path / "made.tfmap"
    path.write_bytes(data)
    g = _ctx(**M.RANDOM)
    if used:
        _stale_cache(g, oracle_mod)
    before = g.swap_stored().view(np.uint32).copy()
    g.load_map(path)
    got = _state(g)
    _assert_state("loaded", got, MR.unpack(data, store=before))
    # blocks of entries the file does not flag are left as they are
    off = np.flatnonzero(got["swapFlags"] == 0)
    assert got["store"].reshape(-1, 512)[off].tobytes() == before.reshape(-1, 512)[off].tobytes()
    assert g.swap_counts() == (0, 0, 0)
    # grid, hash walk and cache are all in place
    assert_bit_exact("whole mesh after load", g.mesh(whole=True), case["tris"])
    resident = M.extract(got["hash"], g.vba(), M.VOXEL_SIZE, M.RANDOM["n_buckets"])
    assert_bit_exact("resident mesh after load", g.mesh(), resident)
    p2 = tmp_path / "again.tfmap"
    g.save_map(p2)
    assert p2.read_bytes() == data
    g.close()


# ---- the engine twin: the turning camera of test_gpu_mesh_whole.test_engine_path ------------------------------------
SAVE_AFTER = 13


def _engine_observe(g):
    s = _state(g)
    ids = np.flatnonzero(s["swapFlags"] == 1)
    return dict(stats=g.stats(), swap_counts=g.swap_counts(), hash=s["hash"].tobytes(), vba=s["vba"].tobytes(),
                vis=s["visType"].tobytes(), ids=s["visibleIds"].tobytes(),
                alloc=s["allocList"][:s["counters"]["lastFreeBlockId"] + 1].tobytes(), excess=s["excessList"].tobytes(),
                state=s["swapState"].tobytes(), flags=s["swapFlags"].tobytes(), store=s["store"].reshape(-1, 512)[ids].tobytes())


def test_engine_twin(tmp_path, oracle_mod):
    """A saves after frame 13 of the turning camera (on the oracle: 115 stored-only, 4 pending, 29 merged, 14
    never-stored blocks); B (fresh) and C (used: the first six frames of the sequence reversed, so a stale hash, VBA
    and cache) load; frames 14..19 swap in with merges and swap out on all three, which agree after each; B equals
    the oracle that ran straight through; the three whole meshes are byte-identical."""
    from topfusion_amd import _lib
    from test_gpu_engines import Pitched, _f, _ok
    from test_gpu_mesh_whole import ENGINE, _classes, _turning_frames
    from test_gpu_swapping import _compare
    L = _lib.load()
    frames = _turning_frames(oracle_mod)
    fx, fy, cx, cy = synth.intrinsics(W, H)
    o = oracle_mod.Oracle(oracle_mod.default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, use_swapping=1,
                                                    swap_transfer_blocks=16, **ENGINE))
    intr = np.array([fx, fy, cx, cy], np.float32)
    dists = Pitched(H, W, np.float32)

    def step(ctxs, k, oracle=True):
        dd, w2c = frames[k]
        dists.put(dd)
        for t in ctxs:
            _ok(L.tf_scene_alloc(t._h, _f(intr), _f(w2c), dists.ptr, dists.step, 0, 0), "tf_scene_alloc")
            _ok(L.tf_scene_integrate(t._h, _f(intr), _f(w2c), dists.ptr, dists.step), "tf_scene_integrate")
            t.swap()
        if oracle:
            o.alloc(w2c, dd)
            o.integrate(w2c, dd)
            o.swap()

    a, b, c = (_ctx(**ENGINE) for _ in range(3))
    for k in range(SAVE_AFTER + 1):
        step([a], k)
    oc = _classes(o.hash(), o.swap_state(), o.swap_stored_flags())
    assert oc == dict(stored=115, pending=4, merged=29, active=14), oc
    assert min(oc.values()) > 0
    _compare(a, o, "A at the save point", stored=True)
    path = tmp_path / "a.tfmap"
    a.save_map(path)
    for k in (19, 18, 17, 16, 15, 14):
        step([c], k, oracle=False)
    assert c.swap_stored_flags().any()
    b.load_map(path)
    c.load_map(path)
    sa = _state(a)
    for name, g in (("B", b), ("C", c)):
        _assert_state(name, _state(g), sa)
        assert g.swap_counts() == (0, 0, 0)
    merged, pending = [], []
    for k in range(SAVE_AFTER + 1, len(frames)):
        step([a, b, c], k)
        oa = _engine_observe(a)
        for name, g in (("B", b), ("C", c)):
            og = _engine_observe(g)
            for key in oa:
                assert og[key] == oa[key], (name, k, key)
        assert b.swap_counts() == o.swap_counts(), k
        _compare(b, o, f"B after frame {k}", stored=True)
        cl = _classes(o.hash(), o.swap_state(), o.swap_stored_flags())
        merged.append(cl["merged"])
        pending.append(cl["pending"])
    assert merged[-1] == 36 and max(pending) == 22, (merged, pending)      # swap-ins with merges happened after the load
    ma = a.mesh(whole=True)
    assert len(ma) > a.mesh_count() > 0
    assert b.mesh(whole=True).tobytes() == ma.tobytes() == c.mesh(whole=True).tobytes()
    dists.free()
    for g in (a, b, c):
        g.close()


# ---- the tracked twin: the frame path ---------------------------------------------------------------------------------
TRACKED = dict(voxelSize=0.0075, n_buckets=4096, n_excess=512, n_blocks=4096)


def _tracked_observe(g, resets0):
    """test_resume_twin's observations and the cache; n_resets, a count over the context's life like the totals (not
    stored), as the resets since the load."""
    o = C._observe(g)
    o["stats"] = dict(o["stats"], n_resets=o["stats"]["n_resets"] - resets0)
    flags = g.swap_stored_flags()
    o.update(swap_counts=g.swap_counts(), state=g.swap_state().tobytes(), flags=flags.tobytes(),
             store=g.swap_stored().view(np.uint32).reshape(-1, 512)[np.flatnonzero(flags == 1)].tobytes())
    return o


# (angle step, last angle, blocks per transfer, the frame after which A saves, the last frame run, the oracle's stored
# flags at the save point, {frame: (verdict, swap counts)} on the oracle)
TRACKED_CASES = [
    (3, 27, 512, 3, 9, 250, {4: (True, (512, 512, 0)), 5: (False, (0, 0, 0)), 6: (True, (512, 0, 0)), 9: (True, (512, 372, 0))}),
    (2, 18, 1024, 17, 18, 140, {18: (True, (684, 1024, 10))}),
]


@pytest.mark.parametrize("step,last,transfer,save_after,until,stored,expect", TRACKED_CASES)
def test_tracked_twin(tmp_path, oracle_mod, step, last, transfer, save_after, until, stored, expect):
    """TopFu::operator() on a swapping context, orbit angles 0, step .. last and back.  A saves after frame
    `save_after`; B (fresh) and C (used: four frames of another orbit, a whole-map mesh, then flags set over its
    whole cache) load; the three run on and agree after every frame, verdicts as the oracle's.  Case 1: frame 4 tracks
    and swaps 512 in / 512 out, frame 5's ICP fails -- the in-frame reset after a load (scene_external: a full clear)
    must empty the loaded cache over the whole table -- and frames 6..9 track and store again.  Case 2: frame 18
    swaps 684 in and 1024 out, reallocates 10 swapped-out entries and merges their 10 stored blocks."""
    from topfusion_amd import _lib as L
    from test_gpu_swapping import _compare
    angles = list(range(0, last + 1, step)) + list(range(last - step, -1, -step))
    fx, fy, cx, cy = synth.intrinsics(W, H)
    kw = dict(use_swapping=1, swap_transfer_blocks=transfer, **TRACKED)
    o = oracle_mod.Oracle(oracle_mod.default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, **kw))
    a, b, c = (_ctx(**kw) for _ in range(3))

    def depth(k):
        Rm, t = synth.orbit_pose(1, deg_per_frame=angles[k])
        return synth.render_depth(Rm, t, W, H, noise_mm=1.0, seed=7000 + k)

    for k in range(save_after + 1):
        d = depth(k)
        assert bool(a(d)) == bool(o(d)), k
    assert int(o.swap_stored_flags().sum()) == stored > 0
    assert np.array_equal(a.swap_stored_flags(), o.swap_stored_flags())
    path = tmp_path / "a.tfmap"
    a.save_map(path)
    for f in synth.orbit_sequence(4, W, H, seed=3):
        c(f)
    assert c.mesh_count(whole=True) > 0
    n_total = TRACKED["n_buckets"] + TRACKED["n_excess"]
    c.upload(L.TF_BUF_SWAP_STORED_FLAGS, np.ones(n_total, np.uint8))
    c.upload(L.TF_BUF_SWAP_STATE, np.full(n_total, 1, np.uint8))
    b.load_map(path)
    c.load_map(path)
    sa = _state(a)
    for name, g in (("B", b), ("C", c)):
        _assert_state(name, _state(g), sa)
    merged0 = o.swap_merged_total()
    resets0 = {id(g): g.stats()["n_resets"] for g in (a, b, c)}
    for k in range(save_after + 1, until + 1):
        d = depth(k)
        oko = bool(o(d))
        oks = []
        for g in (a, b, c):                                                 # one context's frame at a time on the device: a per-call
            oks.append(bool(g(d)))                                          # frame returns on its verdict, the rest still running
            g.swap_counts()
        assert oks == [oko] * 3, (k, oks, oko)
        if k in expect:
            assert (oko, o.swap_counts()) == expect[k], (k, oko, o.swap_counts())
        oa = _tracked_observe(a, resets0[id(a)])
        assert oa["swap_counts"] == o.swap_counts(), k
        for name, g in (("B", b), ("C", c)):
            og = _tracked_observe(g, resets0[id(g)])
            for key in oa:
                assert og[key] == oa[key], (name, k, key)
        if not oko:                                                         # the reset emptied the cache, all of it
            assert not b.swap_stored_flags().any() and not b.swap_state().any() and not c.swap_stored_flags().any()
    if transfer == 1024:
        assert o.swap_merged_total() - merged0 == 10
    assert b.swap_stored_flags().any()
    _compare(b, o, "B at the end", stored=True)
    for g in (a, b, c):
        g.close()


# ---- arguments and refusals -----------------------------------------------------------------------------------------------
def _status(fn, *args):
    return C._status(fn, *args)


def test_arguments_and_refusal(tmp_path):
    import topfusion_amd
    from topfusion_amd import TopFu, _lib as L
    m = _made_map()
    a = _ctx(**M.RANDOM)
    _upload_map(a, m)
    path = tmp_path / "a.tfmap"
    a.save_map(path)
    data = path.read_bytes()
    sa = _state(a)
    rec = MR.records_of(sa)
    # map_file_info: the header, against stats() and the params
    info = topfusion_amd.map_file_info(path)
    st = a.stats()
    for k in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries", "frame_counter"):
        assert info[k] == st[k], k
    assert bytes(info["params"]) == bytes(a.params_) and info["pose_algebra"] == a.pose_algebra()
    assert info["file_bytes"] == len(data) and info["pose"].tobytes() == a.getCameraPose()[:3].tobytes()
    assert info["version"] == 2 and info["n_records"] == len(rec)
    assert info["n_blocks_stored"] == int((rec["entry"]["ptr"] >= 0).sum()) > 0
    assert info["n_cache_blocks"] == int(sa["swapFlags"].sum()) > 0
    # version 1 through the map entry points: tf_scene_save's bytes, tf_scene_load's behaviour
    plain = _ctx(False, **M.RANDOM)
    C._upload_state(plain, m)
    v1, v1m = tmp_path / "plain.tfscene", tmp_path / "plain.tfmap"
    plain.save_scene(v1)
    plain.save_map(v1m)
    assert v1m.read_bytes() == v1.read_bytes()
    i1 = topfusion_amd.map_file_info(v1)
    assert i1["version"] == 1 and i1["n_cache_blocks"] == 0 and i1["n_records"] == topfusion_amd.scene_file_info(v1)["n_records"]
    plain2 = _ctx(False, **M.RANDOM)
    plain2.load_map(v1)
    assert R.states_equal(C._state(plain2), R.unpack(v1.read_bytes()))      # (the uploaded tables, less what no entry holds)
    # the version-1 entry points refuse the version-2 file, as any unknown version
    assert _status(topfusion_amd.scene_file_info, path) == L.TF_INVALID_ARG
    before = C._state(plain2)
    assert _status(plain2.load_scene, path) == L.TF_INVALID_ARG
    assert _status(plain2.load_map, path) == L.TF_INVALID_ARG              # version 2 into a context without swapping
    assert R.states_equal(C._state(plain2), before)
    assert _status(a.save_map, tmp_path / "no" / "such" / "dir.tfmap") == L.TF_INVALID_ARG
    # refused loads leave the context as it was, cache buffers included
    bad = {"version 1": v1.read_bytes(), "truncated": data[:-1], "header only": data[:MR.HEADER_BYTES], "empty": b"",
           "extended": data + b"\0"}
    flip = bytearray(data)
    flip[R.PARAMS_OFFSET] ^= 1                                              # cols
    bad["corrupt header"] = bytes(flip)

    def patched(offset, value, n_cache=None):
        """A byte of the first record overwritten (or n_cache_blocks), both checksums recomputed."""
        import struct
        import zlib
        d = bytearray(data)
        if n_cache is None:
            d[MR.HEADER_BYTES + offset] = value
        else:
            struct.pack_into("<q", d, MR.CACHE_BLOCKS_OFFSET, n_cache)
        struct.pack_into("<I", d, MR.RECORDS_CRC_OFFSET, zlib.crc32(bytes(d[MR.HEADER_BYTES:MR.HEADER_BYTES + 24 * len(rec)])))
        struct.pack_into("<I", d, MR.CRC_OFFSET, zlib.crc32(bytes(d[:MR.CRC_OFFSET])))
        return bytes(d)

    bad["state byte 3"] = patched(21, 3)
    bad["flag byte 2"] = patched(22, 2)
    bad["pad byte"] = patched(23, 1)
    bad["n_cache_blocks + 1"] = patched(0, 0, info["n_cache_blocks"] + 1)
    bad["n_cache_blocks - 1"] = patched(0, 0, info["n_cache_blocks"] - 1)
    targets = {"same": _ctx(**M.RANDOM), "n_blocks": _ctx(**dict(M.RANDOM, n_blocks=256)),
               "mu": _ctx(**dict(M.RANDOM), mu=0.03)}
    other = _made_map()
    other["swapState"] = np.roll(other["swapState"], 7)
    other["swapFlags"] = np.roll(other["swapFlags"], 5)
    for name, g in targets.items():
        if g.params_.n_blocks == M.RANDOM["n_blocks"]:
            _upload_map(g, other)
        before = _state(g)
        if name == "same":
            for tag, blob in bad.items():
                p = tmp_path / "bad.tfmap"
                p.write_bytes(blob)
                assert _status(g.load_map, p) == L.TF_INVALID_ARG, tag
            assert _status(g.load_map, tmp_path / "missing.tfmap") == L.TF_INVALID_ARG
        else:
            assert _status(g.load_map, path) == L.TF_INVALID_ARG, name
        after = _state(g)
        assert MR.states_equal(after, before), name
        for k in ("hash", "vba", "swapState", "swapFlags", "store", "pose"):
            assert after[k].tobytes() == before[k].tobytes(), (name, k)
    # ... and the intact file still loads there, with another transfer size of its own; from_map builds the context itself
    targets["same"].load_map(path)
    want = MR.unpack(data)
    _assert_state("same", _state(targets["same"]), want)
    t2 = _ctx(**dict(M.RANDOM, swap_transfer_blocks=5))
    t2.load_map(path)
    assert t2.params_.swap_transfer_blocks == 5
    f = TopFu.from_map(path)
    assert bytes(f.params_) == bytes(a.params_) and f.params_.use_swapping == 1
    _assert_state("from_map", _state(f), want)
    p3 = tmp_path / "f.tfmap"
    f.save_map(p3)
    assert p3.read_bytes() == data
    f1 = TopFu.from_map(v1)
    assert f1.params_.use_swapping == 0 and R.states_equal(C._state(f1), R.unpack(v1.read_bytes()))
    for g in list(targets.values()) + [a, f, f1, t2, plain, plain2]:
        g.close()


def test_save_refuses_what_load_would(tmp_path):
    """Tables that came through tf_upload and that tf_map_load would refuse are not written: a swap state of 3, a
    stored flag of 2, a chain offset past the excess list, one block named by two entries."""
    from topfusion_amd import _lib as L
    path = tmp_path / "bad.tfmap"

    def state3(s):
        s["swapState"][100] = 3

    def flag2(s):
        s["swapFlags"][CORNERS[-1]] = 2

    def offset(s):
        s["hash"]["offset"][0] = M.RANDOM["n_excess"] + 1

    def twice(s):
        live = np.flatnonzero(s["hash"]["ptr"] >= 0)
        s["hash"]["ptr"][live[1]] = s["hash"]["ptr"][live[0]]

    g = _ctx(**M.RANDOM)
    for damage in (state3, flag2, offset, twice):
        s = _made_map()
        damage(s)
        _upload_map(g, s)
        assert _status(g.save_map, path) == L.TF_INVALID_ARG, damage.__name__
        assert not path.exists()
    _upload_map(g, _made_map())
    g.save_map(path)                                                       # the undamaged tables still save
    assert path.read_bytes() == MR.pack(_state(g))
    g.close()


def test_map_resume_check_app(tmp_path):
    """apps/map_resume_check: a swapping Scene saved half way through a short walk (Scene::saveMap), a second one
    resumed from the file (Scene::loadMap), both fused to the end through the C++ engine layer: equal counters and
    byte-identical whole-map meshes; the file is a version-2 checkpoint far smaller than the GlobalCache's own dump."""
    import topfusion_amd
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "apps"), "map_resume_check"], check=True)
    path = tmp_path / "app.tfmap"
    r = subprocess.run([os.path.join(ROOT, "apps", "map_resume_check"), "12", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MATCH" in r.stdout and "MISMATCH" not in r.stdout, r.stdout + r.stderr
    info = topfusion_amd.map_file_info(path)
    assert info["version"] == 2 and info["n_cache_blocks"] > 0 and info["file_bytes"] == os.path.getsize(path)
    assert f"map file {info['file_bytes']} bytes" in r.stdout and f"SaveToFile {(4096 + 512) * 2049} bytes" in r.stdout, r.stdout
    assert info["file_bytes"] < (4096 + 512) * 2049 // 4
