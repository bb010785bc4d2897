"""The mesher's whole reading on the GPU (tf_mesh_extract_whole, TF_MESH_WHOLE; topfusion_amd/csrc/tf_mesh.hip)
against the numpy restatement of its specification (tests/mesh_whole_ref.py), bit for bit: the triangle count,
every float of the positions and the normals, in order.  A hand-made scene of both tiers with every row of
the resolution table (its conditions are asserted on the CPU, tests/test_mesh_whole_ref.py), scenes without
stored data (whole == resident, byte for byte), the capacity and argument rules, a scene the swapping engine
itself produced, and the files."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_attr_ref as A
import mesh_ref as M
import mesh_whole_ref as WR
from parity_util import DeviceFrames, assert_bit_exact
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


def _load_two_tier(g, c):
    from topfusion_amd import _lib as L
    g.upload(L.TF_BUF_HASH, c["hash"])
    g.upload(L.TF_BUF_VBA, c["vba"])
    g.upload(L.TF_BUF_SWAP_STATE, c["state"])
    g.upload(L.TF_BUF_SWAP_STORED_FLAGS, c["flags"])
    g.upload(L.TF_BUF_SWAP_STORED, c["store"])


def _tiers(g):
    """The five buffers the whole reading resolves, downloaded."""
    return g.hash(), g.vba(), g.swap_state(), g.swap_stored_flags(), g.swap_stored()


def _download(ptr, n_words):
    from topfusion_amd import _lib as L
    out = np.empty(n_words, np.uint32)
    assert L.hip_runtime().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), out.nbytes, 2) == 0
    return out


def test_two_tier_scene():
    """Every row of the resolution table in one scene: active, stored-only, pending merge (state 1 and 0, with
    oldW == 0, the maxW clamp and an empty active block), a stale store, lost entries; neighbours through the
    grid and through the hash walk.  The resident reading of the same context is untouched."""
    c = WR.two_tier_case()
    g = _ctx(**M.RANDOM)
    _load_two_tier(g, c)
    want = c["tris"]
    n = g.mesh_count(whole=True)
    assert n == len(want), f"{n} triangles, reference {len(want)}"
    assert_bit_exact("whole mesh", g.mesh(whole=True), want)
    tris, normals, colours = g.mesh_attr(normals=True, whole=True)
    assert colours is None
    assert_bit_exact("whole mesh (attr)", tris, want)
    assert_bit_exact("whole normals", normals, c["normals"])
    resident = M.extract(c["hash"], c["vba"], M.VOXEL_SIZE, M.RANDOM["n_buckets"])
    assert g.mesh_count() == len(resident)
    assert_bit_exact("resident mesh", g.mesh(), resident)
    g.close()


@pytest.mark.parametrize("swapping", [False, True])
def test_no_stored_data(swapping):
    """Without stored data the whole mesh is the resident one, byte for byte; an empty scene has none."""
    h, vba, want, _ = M.sphere_case()
    g = _ctx(swapping, **M.SMALL)
    assert g.mesh_count(whole=True) == 0 and g.mesh(whole=True).shape == (0, 3, 3)
    from topfusion_amd import _lib as L
    g.upload(L.TF_BUF_HASH, h)
    g.upload(L.TF_BUF_VBA, vba)
    assert g.mesh_count(whole=True) == len(want)
    assert g.mesh(whole=True).tobytes() == g.mesh().tobytes() == want.tobytes()
    tw, nw, _ = g.mesh_attr(normals=True, whole=True)
    tr, nr, _ = g.mesh_attr(normals=True)
    assert tw.tobytes() == tr.tobytes() and nw.tobytes() == nr.tobytes()
    g.close()


def test_capacity_and_arguments(tmp_path):
    from topfusion_amd import _lib as L
    lib = L.load()
    c = WR.two_tier_case()
    g = _ctx(**M.RANDOM)
    _load_two_tier(g, c)
    want, wantn = c["tris"], c["normals"]
    n = len(want)
    half = n // 2
    sentinel = np.full(n * 9, 0xdeadbeef, np.uint32)
    bt, bn = DeviceFrames(sentinel), DeviceFrames(sentinel)
    got_n = ctypes.c_longlong(-1)
    L.check(lib.tf_mesh_extract_whole(g._h, ctypes.c_void_p(bt.ptr), ctypes.c_void_p(bn.ptr), half, ctypes.byref(got_n)),
            "tf_mesh_extract_whole")
    assert got_n.value == n                                       # the full count, whatever the capacity
    for tag, buf, ref in (("triangles", bt, want), ("normals", bn, wantn)):
        out = _download(buf.ptr, n * 9)
        assert_bit_exact(f"first half of the {tag}", out[:half * 9].view(np.float32).reshape(-1, 3, 3), ref[:half])
        assert np.array_equal(out[half * 9:], sentinel[half * 9:]), f"{tag}: wrote past the capacity"
    got_n.value = -1
    L.check(lib.tf_mesh_extract_whole(g._h, None, None, 0, ctypes.byref(got_n)), "tf_mesh_extract_whole")
    assert got_n.value == n                                       # count only
    assert np.array_equal(_download(bt.ptr, n * 9)[half * 9:], sentinel[half * 9:])
    tp, np_ = ctypes.c_void_p(bt.ptr), ctypes.c_void_p(bn.ptr)
    assert lib.tf_mesh_extract_whole(None, tp, np_, n, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    assert lib.tf_mesh_extract_whole(g._h, tp, np_, n, None) == L.TF_INVALID_ARG
    assert lib.tf_mesh_extract_whole(g._h, tp, np_, -1, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    assert lib.tf_mesh_extract_whole(g._h, None, None, 5, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    path = str(tmp_path / "x.ply").encode()
    assert lib.tf_mesh_save_ply_indexed(g._h, path, L.TF_MESH_WHOLE) == L.TF_INVALID_ARG
    assert lib.tf_mesh_save_ply_indexed(g._h, path, L.TF_MESH_WHOLE | L.TF_MESH_INDEXED) == L.TF_INVALID_ARG
    assert lib.tf_mesh_save_ply_attr(g._h, path, L.TF_MESH_WHOLE | L.TF_MESH_COLOURS) == L.TF_INVALID_ARG
    for call in (lambda: g.save_mesh(tmp_path / "y.ply", indexed=True, whole=True),
                 lambda: g.save_mesh(tmp_path / "y.ply", colours=True, whole=True),
                 lambda: g.mesh_attr(colours=True, whole=True)):
        with pytest.raises(L.TfError) as e:
            call()
        assert e.value.status == L.TF_INVALID_ARG
    assert not (tmp_path / "x.ply").exists() and not (tmp_path / "y.ply").exists()
    bt.free()
    bn.free()
    g.close()


# ---- a scene the swapping engine produced ---------------------------------------------------------------------
ENGINE = dict(voxelSize=0.04, mu=0.08, vis_capacity=8192, **M.SMALL)     # 4 cm voxels: the room is ~160 blocks, the VBA 128
ANGLES = list(range(0, 400, 40)) + list(range(360, -1, -40))


def _turning_frames(oracle_mod):
    """test_swapping_engine_path's camera: turning in place through 400 deg and back, ground-truth poses."""
    from test_gpu_swapping import _rt32, _yaw_pose
    out = []
    for k, deg in enumerate(ANGLES):
        R, t = _yaw_pose(deg)
        depth = synth.render_depth(R, t, W, H, noise_mm=1.0, seed=1000 + k)
        out.append((oracle_mod.compute_dists(depth), oracle_mod.rigid_inv(_rt32(R, t))))
    return out


def _classes(h, state, flags):
    p = h["ptr"]
    return dict(stored=int(((p == -1) & (flags == 1)).sum()), pending=int(((p >= 0) & (flags == 1) & (state != 2)).sum()),
                merged=int(((p >= 0) & (flags == 1) & (state == 2)).sum()), active=int(((p >= 0) & (flags == 0)).sum()))


def test_engine_path(oracle_mod):
    """tf_scene_alloc / tf_scene_integrate / swap() over the turning camera with a VBA of 128 blocks and 16
    blocks per transfer (chosen by running the oracle over these poses: both backlogs carry over, so after the
    last frame stored-only, pending and merged entries all exist -- asserted on the oracle and on the GPU's
    buffers).  The whole mesh equals the reference on the downloaded tiers, holds more than the resident one,
    and a twin context that never meshed is bit-identical in all five buffers."""
    from topfusion_amd import _lib
    from test_gpu_engines import Pitched, _f, _ok
    L = _lib.load()
    frames = _turning_frames(oracle_mod)
    fx, fy, cx, cy = synth.intrinsics(W, H)
    o = oracle_mod.Oracle(oracle_mod.default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, use_swapping=1,
                                                    swap_transfer_blocks=16, **ENGINE))
    for dd, w2c in frames:
        o.alloc(w2c, dd)
        o.integrate(w2c, dd)
        o.swap()
    oc = _classes(o.hash(), o.swap_state(), o.swap_stored_flags())
    assert min(oc["stored"], oc["pending"], oc["merged"]) > 0, oc
    g, twin = _ctx(**ENGINE), _ctx(**ENGINE)
    intr = np.array([fx, fy, cx, cy], np.float32)
    dists = Pitched(H, W, np.float32)
    for k, (dd, w2c) in enumerate(frames):
        dists.put(dd)
        for t in (g, twin):
            _ok(L.tf_scene_alloc(t._h, _f(intr), _f(w2c), dists.ptr, dists.step, 0, 0), "tf_scene_alloc")
            _ok(L.tf_scene_integrate(t._h, _f(intr), _f(w2c), dists.ptr, dists.step), "tf_scene_integrate")
            t.swap()
        if k == len(frames) // 2:
            assert g.mesh_count(whole=True) > 0                   # a meshing in mid-sequence: the frames after it must not see it
    h, vba, state, flags, store = _tiers(g)
    gc = _classes(h, state, flags)
    assert gc == oc, (gc, oc)
    want, wantn = WR.extract(h, vba, state, flags, store, ENGINE["voxelSize"], ENGINE["n_buckets"], normals=True)
    n = g.mesh_count(whole=True)
    assert n == len(want), f"{n} triangles, reference {len(want)}"
    tris, normals, _ = g.mesh_attr(normals=True, whole=True)
    assert_bit_exact("engine whole mesh", tris, want)
    assert_bit_exact("engine whole normals", normals, wantn)
    assert g.mesh(whole=True).tobytes() == tris.tobytes()
    assert n > g.mesh_count() > 0
    for name, a, b in zip(("hash", "vba", "swap state", "stored flags", "stored blocks"), _tiers(g), _tiers(twin)):
        assert a.tobytes() == b.tobytes(), f"{name}: the meshing context differs from its twin"
    assert g.stats() == twin.stats()
    dists.free()
    g.close()
    twin.close()


# ---- files ------------------------------------------------------------------------------------------------------
def _assert_welded(path, want_tris, normals=None):
    from topfusion_amd import io
    if normals is None:
        verts, faces = io.read_ply(path)
        wv, wf = M.weld(want_tris)
        assert len(verts) == len(wv) and len(faces) == len(wf) == len(want_tris)
        assert_bit_exact(f"{path.name}", verts[faces], want_tris)
        assert np.array_equal(np.unique(verts.view(np.uint32).reshape(-1, 3), axis=0), wv.view(np.uint32).reshape(-1, 3))
    else:
        verts, faces, nrm, _ = io.read_ply_attr(path)
        rec, wf = A.weld(want_tris, normals)
        assert len(verts) == len(rec) and len(faces) == len(wf)
        assert_bit_exact(f"{path.name} positions", verts[faces], want_tris)
        assert_bit_exact(f"{path.name} normals", nrm[faces], normals)


def test_save_mesh_whole(tmp_path):
    c = WR.two_tier_case()
    g = _ctx(**M.RANDOM)
    _load_two_tier(g, c)
    g.save_mesh(tmp_path / "whole.ply", whole=True)
    _assert_welded(tmp_path / "whole.ply", c["tris"])
    g.save_mesh(tmp_path / "whole_n.ply", normals=True, whole=True)
    _assert_welded(tmp_path / "whole_n.ply", c["tris"], c["normals"])
    # without the flag: today's file
    resident = M.extract(c["hash"], c["vba"], M.VOXEL_SIZE, M.RANDOM["n_buckets"])
    g.save_mesh(tmp_path / "resident.ply")
    _assert_welded(tmp_path / "resident.ply", resident)
    from topfusion_amd import io
    io.write_ply(tmp_path / "resident_host.ply", g.mesh())
    assert (tmp_path / "resident.ply").read_bytes() == (tmp_path / "resident_host.ply").read_bytes()
    g.close()


def test_mesh_whole_check_app(tmp_path):
    """apps/mesh_whole_check fuses a turning camera into a swapping Scene through the C++ engine layer and saves
    the whole mesh: the file is the weld of the reference's triangles for the tiers the program dumps."""
    from topfusion_amd.topfu import HASH_DTYPE, VOXEL_DTYPE
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "apps"), "mesh_whole_check"], check=True)
    ply, prefix = tmp_path / "app.ply", tmp_path / "tiers"
    r = subprocess.run([os.path.join(ROOT, "apps", "mesh_whole_check"), str(ply), str(prefix)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MATCH" in r.stdout and "MISMATCH" not in r.stdout, r.stdout + r.stderr
    rd = lambda ext, dt: np.fromfile(str(prefix) + ext, dt)
    h, vba, store = rd(".hash", HASH_DTYPE), rd(".vba", VOXEL_DTYPE), rd(".store", VOXEL_DTYPE)
    state, flags = rd(".state", np.uint8), rd(".flags", np.uint8)
    assert ((h["ptr"] == -1) & (flags == 1)).any(), "the program's scene has no stored-only block"
    want = WR.extract(h, vba, state, flags, store, 0.04, 4096)
    assert len(want) > len(M.extract(h, vba, 0.04, 4096))
    _assert_welded(ply, want)
