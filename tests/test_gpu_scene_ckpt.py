"""Scene checkpoints on the GPU (tf_scene_save / tf_scene_load and the layers above them,
topfusion_amd/csrc/tf_scene_ckpt.hip) against the numpy restatement of the file (tests/scene_ckpt_ref.py),
byte for byte, and as a resumed sequence: a context that loads a checkpoint is the context that saved it,
now and after further frames."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_indexed_ref as I
import mesh_ref as M
import scene_ckpt_ref as R
from parity_util import assert_bit_exact
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 72
TABLES = dict(n_buckets=4096, n_excess=512)


def _ctx(n_blocks=128, **kw):
    from topfusion_amd import TopFu, default_params
    fx, fy, cx, cy = synth.intrinsics(W, H)
    args = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=M.VOXEL_SIZE, n_blocks=n_blocks, **TABLES)
    args.update(kw)
    return TopFu(default_params(**args))


def _state(g):
    """The context's state as scene_ckpt_ref takes it, from the download entry points."""
    from topfusion_amd import _lib as L
    import ctypes
    p = L.TfParams()
    L.check(L.load().tf_get_params(g._h, ctypes.byref(p)), "tf_get_params")
    st = g.stats()
    maps = []
    for l in range(3):
        maps.extend(g.prev_maps(l))
    return dict(params=R.params_record(p), pose_algebra=g.pose_algebra(),
                counters={k: st[k] for k in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries", "frame_counter")},
                pose=g.getCameraPose()[:3].reshape(12).copy(), hash=g.hash(), visType=g.visible_type(),
                vba=g.vba().view(np.uint32), rgb=g.vba_rgb() if p.voxel_rgb else None, visibleIds=g.visible_ids(),
                allocList=g.alloc_list(), excessList=g.excess_list(), maps=maps)


def _random_maps(rng):
    return [rng.standard_normal((H >> l, W >> l, 4)).astype(np.float32) for l in range(3) for _ in range(2)]


def _upload_state(g, s):
    """A numpy-made state into a context, through the upload entry points."""
    from topfusion_amd import _lib as L
    g.upload(L.TF_BUF_HASH, s["hash"])
    g.upload(L.TF_BUF_VBA, s["vba"])
    if s["rgb"] is not None:
        g.upload(L.TF_BUF_VBA_RGB, s["rgb"])
    g.upload(L.TF_BUF_VISIBLE_TYPE, s["visType"])
    ids = np.zeros(g.params_.vis_capacity, np.int32)
    ids[:len(s["visibleIds"])] = s["visibleIds"]
    g.upload(L.TF_BUF_VISIBLE_IDS, ids)
    g.upload(L.TF_BUF_ALLOC_LIST, s["allocList"])
    g.upload(L.TF_BUF_EXCESS_LIST, s["excessList"])
    for l in range(3):
        g.upload(L.TF_BUF_PREV_POINTS, s["maps"][2 * l], level=l)
        g.upload(L.TF_BUF_PREV_NORMALS, s["maps"][2 * l + 1], level=l)
    g.set_pose(s["pose"])
    c = s["counters"]
    g.set_counters(c["lastFreeBlockId"], c["lastFreeExcessListId"], c["noVisibleEntries"])


N_BUCKETS, N_EXCESS, N_BLOCKS = 4096, 512, 128
PTRS = (5, 0, 127, 64, 3, 17, 100, 33, 9, 77)          # ten stored blocks


def _made_scene(rgb):
    """Entries at the corners of the count groups and of both tables (0, 511, 512, 4095, the first and last
    excess slot), a bucket with a two-entry excess chain, an entry with only visType set, an entry without a
    block, shuffled blocks, non-identity free lists with counters of their own."""
    rng = np.random.default_rng(5 + rgb)
    n_total = N_BUCKETS + N_EXCESS
    h = np.full(n_total, R.reset_entry(), R.HASH_DTYPE)
    at = [0, 511, 512, 4095, N_BUCKETS, n_total - 1, 1000, N_BUCKETS + 7, N_BUCKETS + 300, 2048]
    for k, (i, ptr) in enumerate(zip(at, PTRS)):
        h[i] = (k - 4, 3 * k, -k, 0, 0, ptr)
    h["offset"][1000] = 8                               # 1000 -> excess slot 7 -> excess slot 300
    h["offset"][N_BUCKETS + 7] = 301
    h[2000] = (9, 9, 9, 0, 0, -1)                       # no block
    vis = np.zeros(n_total, np.uint8)
    vis[[0, 512, N_BUCKETS + 7]] = (1, 3, 1)
    vis[3000] = 2                                       # only visType
    alloc = rng.permutation(N_BLOCKS).astype(np.int32)
    excess = rng.permutation(N_EXCESS).astype(np.int32)
    pose = np.eye(4, dtype=np.float32)[:3].reshape(12).copy()
    pose[[3, 7, 11]] = (0.125, -0.5, 0.75)
    return dict(hash=h, visType=vis, vba=rng.integers(0, 1 << 24, N_BLOCKS * 512, dtype=np.uint32),
                rgb=rng.integers(0, 1 << 32, N_BLOCKS * 512, dtype=np.uint32) if rgb else None,
                visibleIds=np.array([0, 512, N_BUCKETS + 7], np.int32), allocList=alloc, excessList=excess,
                counters=dict(lastFreeBlockId=N_BLOCKS - len(PTRS) - 1, lastFreeExcessListId=400, noVisibleEntries=3),
                pose=pose, maps=_random_maps(rng))


def _save_made_scene(path, rgb):
    g = _ctx(voxel_rgb=rgb)
    _upload_state(g, _made_scene(rgb))
    g.save_scene(path)
    s = _state(g)
    g.close()
    return s


@pytest.mark.parametrize("rgb", [0, 1])
def test_save_against_reference(tmp_path, rgb):
    path = tmp_path / "made.tfscene"
    s = _save_made_scene(path, rgb)
    data = path.read_bytes()
    want = R.pack(s)
    assert len(data) == len(want) == R.file_size(s["params"], s["counters"], 12, 10)
    assert data == want
    # several chunks with a ragged last one (10 blocks: 3 + 3 + 3 + 1): the knob is read at tf_create, so a
    # fresh process
    for chunk in (3,):
        p2 = tmp_path / f"chunk{chunk}.tfscene"
        env = dict(os.environ, TFUSION_CKPT_CHUNK_BLOCKS=str(chunk))
        code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_scene_ckpt as T; "
                f"T._save_made_scene({str(p2)!r}, {rgb})")
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert p2.read_bytes() == data, f"chunks of {chunk} blocks"


def _sphere_state(g, rgb):
    """mesh_ref's sphere (64 blocks) as a checkpoint state of context g's tables, with a visible list and free
    lists of its own."""
    case = I.sphere_case()
    rng = np.random.default_rng(17)
    s = _state(g)
    s["hash"] = case["hash"].copy()
    s["vba"] = case["vba"].view(np.uint32).copy()
    s["rgb"] = case["rgb"].copy() if rgb else None
    live = np.flatnonzero(s["hash"]["ptr"] >= 0)
    used = s["hash"]["ptr"][live]
    free = np.setdiff1d(np.arange(N_BLOCKS), used).astype(np.int32)
    s["allocList"] = np.arange(N_BLOCKS, dtype=np.int32)
    s["allocList"][:len(free)] = rng.permutation(free)
    s["excessList"] = np.arange(N_EXCESS, dtype=np.int32)
    s["excessList"][:200] = rng.permutation(200)
    s["visType"] = np.zeros(len(s["hash"]), np.uint8)
    s["visType"][live[::3]] = 1
    s["visType"][live[1::3]] = 3
    s["visibleIds"] = live[::3].astype(np.int32)
    s["counters"] = dict(lastFreeBlockId=len(free) - 1, lastFreeExcessListId=199, noVisibleEntries=len(live[::3]),
                         frame_counter=6)
    s["pose"] = np.array([1, 0, 0, 0.1, 0, 1, 0, -0.2, 0, 0, 1, 0.3], np.float32)
    s["maps"] = _random_maps(rng)
    return s, case


@pytest.mark.parametrize("rgb", [0, 1])
def test_load_against_reference(tmp_path, rgb):
    g = _ctx(voxel_rgb=rgb)
    s, case = _sphere_state(g, rgb)
    data = R.pack(s)
    path = tmp_path / "sphere.tfscene"
    path.write_bytes(data)
    g.load_scene(path)
    want = R.unpack(data)                                # s, with what no entry holds at ResetScene's values
    got = _state(g)
    for k in ("hash", "visType", "vba", "allocList", "excessList", "pose"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    assert got["counters"] == want["counters"]
    assert R.states_equal(got, want)
    # the block grid: both meshers find every block and its neighbours
    assert_bit_exact("mesh after load", g.mesh(), case["tris"])
    v, i, _, _ = g.mesh_indexed()
    assert v.tobytes() == case["vertices"].tobytes() and i.tobytes() == case["indices"].tobytes()
    p2 = tmp_path / "again.tfscene"
    g.save_scene(p2)
    assert p2.read_bytes() == data
    g.close()


FRAMES = dict(voxelSize=0.0075)        # at 96 x 72 in 4096 + 512 entries the seed-7 orbit tracks all of frames 0..8 with 7.5 mm voxels


def _frames(seed, n, rgb):
    seq = synth.orbit_sequence(n, W, H, seed=seed)
    cols = [synth.render_colour(*synth.orbit_pose(k), W, H) for k in range(n)] if rgb else [None] * n
    return seq, cols


def _run(g, seq, cols, ks):
    return [bool(g(seq[k], rgb=cols[k])) for k in ks]


def _observe(g):
    """What the twin test compares: poses, stats, the scene, visType, the mesh."""
    s = _state(g)
    return dict(stats=g.stats(), pose=s["pose"].tobytes(), hash=s["hash"].tobytes(), vba=s["vba"].tobytes(),
                rgb=None if s["rgb"] is None else s["rgb"].tobytes(), vis=s["visType"].tobytes(), mesh=g.mesh().tobytes())


@pytest.mark.parametrize("rgb,first", [(0, 4), (1, 4), (0, 1)])
def test_resume_twin(tmp_path, rgb, first):
    """A runs `first` frames and saves; B (fresh) and C (used: four frames of another seed and a mesh extraction,
    so a stale range image, visible list, mesh scratch and tile order) load; all three run four more frames.
    first = 1: the previous maps are frame 0's depth-derived ones, which no raycast reproduces."""
    seq, cols = _frames(7, first + 4, rgb)
    other, ocols = _frames(3, 4, rgb)
    a, b, c = (_ctx(4096, voxel_rgb=rgb, **FRAMES) for _ in range(3))
    assert all(_run(a, seq, cols, range(first)))
    path = tmp_path / "a.tfscene"
    a.save_scene(path)
    assert all(_run(c, other, ocols, range(4)))
    assert len(c.mesh()) > 0
    b.load_scene(path)
    c.load_scene(path)
    sa = _state(a)
    for name, g in (("B", b), ("C", c)):
        sg = _state(g)
        assert sg["hash"].tobytes() == sa["hash"].tobytes(), name
        assert sg["vba"].tobytes() == sa["vba"].tobytes(), name
        assert R.states_equal(sg, sa), name
    # frame by frame; every continued frame tracks, so the loaded maps, lists and scene carry all four
    for k in range(first, first + 4):
        oks = _run(a, seq, cols, [k]) + _run(b, seq, cols, [k]) + _run(c, seq, cols, [k])
        assert oks == [True, True, True], (k, oks)
        oa = _observe(a)
        for name, g in (("B", b), ("C", c)):
            og = _observe(g)
            for key in oa:
                assert og[key] == oa[key], (name, k, key)
    for g in (a, b, c):
        g.close()


def test_reset_after_load(tmp_path):
    seq, cols = _frames(7, 4, 0)
    a, fresh = _ctx(4096, **FRAMES), _ctx(4096, **FRAMES)
    assert all(_run(a, seq, cols, range(4)))
    path = tmp_path / "a.tfscene"
    a.save_scene(path)
    b = _ctx(4096, **FRAMES)
    b.load_scene(path)
    b.reset()
    assert all(_run(b, seq, cols, range(4))) and all(_run(fresh, seq, cols, range(4)))
    sb, sf = _state(b), _state(fresh)
    assert sb["hash"].tobytes() == sf["hash"].tobytes() and sb["vba"].tobytes() == sf["vba"].tobytes()
    assert sb["pose"].tobytes() == sf["pose"].tobytes()
    assert R.states_equal(sb, sf)
    for g in (a, b, fresh):
        g.close()


def _status(fn, *args):
    from topfusion_amd import TfError
    try:
        fn(*args)
    except TfError as e:
        return e.status
    return 0


def test_arguments_and_refusal(tmp_path):
    import topfusion_amd
    from topfusion_amd import TopFu, _lib as L
    seq, cols = _frames(7, 2, 0)
    a = _ctx(4096)
    assert all(_run(a, seq, cols, range(2)))
    path = tmp_path / "a.tfscene"
    a.save_scene(path)
    data = path.read_bytes()
    # scene_file_info: the header, against stats() and params
    info = topfusion_amd.scene_file_info(path)
    st = a.stats()
    for k in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries", "frame_counter"):
        assert info[k] == st[k], k
    assert bytes(info["params"]) == bytes(a.params_) and info["pose_algebra"] == a.pose_algebra()
    assert info["file_bytes"] == len(data) and info["pose"].tobytes() == a.getCameraPose()[:3].tobytes()
    rec = R.records_of(_state(a))
    assert info["n_records"] == len(rec) and info["n_blocks_stored"] == int((rec["entry"]["ptr"] >= 0).sum()) > 0
    # a swapping context neither saves nor loads
    sw = _ctx(4096, use_swapping=1)
    assert _status(sw.save_scene, tmp_path / "sw.tfscene") == L.TF_INVALID_ARG and not (tmp_path / "sw.tfscene").exists()
    assert _status(sw.load_scene, path) == L.TF_INVALID_ARG
    sw.close()
    assert _status(a.save_scene, tmp_path / "no" / "such" / "dir.tfscene") == L.TF_INVALID_ARG
    # refused loads leave the context as it was
    bad = {"truncated": data[:-1], "header only": data[:R.HEADER_BYTES], "empty": b"", "extended": data + b"\0"}
    flip = bytearray(data)
    flip[R.HEADER_BYTES + 16] ^= 0x40                                  # the first record's ptr
    bad["corrupt record"] = bytes(flip)
    flip = bytearray(data)
    flip[R.PARAMS_OFFSET] ^= 1                                         # cols
    bad["corrupt header"] = bytes(flip)
    targets = {"n_blocks": _ctx(128), "voxelSize": _ctx(4096, voxelSize=0.006), "voxel_rgb": _ctx(4096, voxel_rgb=1),
               "same": _ctx(4096)}
    for g in targets.values():
        assert all(_run(g, seq, [None] * 2 if not g.params_.voxel_rgb else [np.zeros((H, W, 4), np.uint8)] * 2, range(1)))
    for name, g in targets.items():
        before = _state(g)
        if name == "same":
            for tag, blob in bad.items():
                p = tmp_path / "bad.tfscene"
                p.write_bytes(blob)
                assert _status(g.load_scene, p) == L.TF_INVALID_ARG, tag
            assert _status(g.load_scene, tmp_path / "missing.tfscene") == L.TF_INVALID_ARG
        else:
            assert _status(g.load_scene, path) == L.TF_INVALID_ARG, name
        after = _state(g)
        assert R.states_equal(after, before), name
        assert after["hash"].tobytes() == before["hash"].tobytes() and after["vba"].tobytes() == before["vba"].tobytes()
        assert after["pose"].tobytes() == before["pose"].tobytes()
    # ... and the intact file still loads there; from_scene builds the context itself
    targets["same"].load_scene(path)
    assert R.states_equal(_state(targets["same"]), _state(a))
    f = TopFu.from_scene(path)
    assert bytes(f.params_) == bytes(a.params_)
    assert R.states_equal(_state(f), _state(a))
    p3 = tmp_path / "f.tfscene"
    f.save_scene(p3)
    assert p3.read_bytes() == data
    for g in list(targets.values()) + [a, f]:
        g.close()


def test_save_refuses_what_load_would(tmp_path):
    """Tables that came through tf_upload and that tf_scene_load would refuse are not written: a chain offset
    past the excess list, one block named by two entries, a free-list value outside the VBA."""
    from topfusion_amd import _lib as L
    path = tmp_path / "bad.tfscene"

    def offset(s):
        s["hash"]["offset"][0] = N_EXCESS + 1

    def twice(s):
        s["hash"]["ptr"][511] = s["hash"]["ptr"][0]

    def free_list(s):
        s["allocList"][0] = N_BLOCKS

    g = _ctx()
    for damage in (offset, twice, free_list):
        s = _made_scene(0)
        damage(s)
        _upload_state(g, s)
        assert _status(g.save_scene, path) == L.TF_INVALID_ARG, damage.__name__
        assert not path.exists()
    _upload_state(g, _made_scene(0))
    g.save_scene(path)                                                 # the undamaged tables still save
    assert path.read_bytes() == R.pack(_state(g))
    g.close()


def test_demo_headless_scene(tmp_path):
    """demo_headless --save-scene writes the bytes a Python context given the same frames writes; a second run
    with --load-scene over the next three frames meshes what a context that ran all six meshes."""
    from topfusion_amd import TopFu, default_params, io
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "apps")], check=True)
    seq = synth.orbit_sequence(6, W, H, seed=7)
    for part in (0, 1):
        os.makedirs(tmp_path / f"p{part}")
        for i in range(3):
            io.write_pgm16(tmp_path / f"p{part}" / f"{i:04d}.pgm", seq[3 * part + i])
    exe = os.path.join(ROOT, "apps", "demo_headless")
    scene, ply = tmp_path / "demo.tfscene", tmp_path / "demo.ply"
    r = subprocess.run([exe, "--pgm", str(tmp_path / "p0" / "%04d.pgm"), "--save-scene", str(scene)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    s = W / 640.0                                                  # the demo's intrinsics: float constants scaled in double
    intr = [float(np.float32(float(np.float32(c)) * s)) for c in (synth.FX, synth.FY, synth.CX, synth.CY)]
    g = TopFu(default_params(cols=W, rows=H, fx=intr[0], fy=intr[1], cx=intr[2], cy=intr[3]))
    for f in seq[:3]:
        g(f)
    mine = tmp_path / "mine.tfscene"
    g.save_scene(mine)
    data = scene.read_bytes()
    assert data == mine.read_bytes()
    from topfusion_amd import scene_file_info
    info = scene_file_info(scene)
    line = f"scene saved to {scene}: {info['n_records']} records, {info['n_blocks_stored']} blocks, {len(data)} bytes\n"
    assert line in r.stdout, r.stdout
    r = subprocess.run([exe, "--pgm", str(tmp_path / "p1" / "%04d.pgm"), "--load-scene", str(scene), "--mesh", str(ply)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert line.replace("saved to", "loaded from") in r.stdout, r.stdout
    for f in seq[3:]:
        g(f)
    verts, faces = io.read_ply(ply)
    tris = g.mesh()
    assert len(tris) > 0
    assert_bit_exact("demo mesh after resume", verts[faces], tris)
    g.close()
