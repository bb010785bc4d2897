"""Mesh extraction on the GPU (tf_mesh_extract and the layers above it, topfusion_amd/csrc/tf_mesh.hip)
against the numpy restatement of its specification (tests/mesh_ref.py), bit for bit: the triangle
count and every float, in order.  Scenes are built by hand (synth.build_hash + uploads) in small
contexts, except the pipeline and demo tests, which mesh what real frames fused."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import mesh_ref as M
from parity_util import DeviceFrames, assert_bit_exact
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 72


def _ctx(**kw):
    from topfusion_amd import TopFu, default_params
    fx, fy, cx, cy = synth.intrinsics(W, H)
    args = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=M.VOXEL_SIZE)
    args.update(kw)
    return TopFu(default_params(**args))


def _load(g, h, vba):
    from topfusion_amd import _lib as L
    g.upload(L.TF_BUF_HASH, h)
    g.upload(L.TF_BUF_VBA, vba)


def _check(tag, g, want):
    n = g.mesh_count()
    assert n == len(want), f"{tag}: {n} triangles, reference {len(want)}"
    assert_bit_exact(tag, g.mesh(), want)


def _download(ptr, n_floats):
    from topfusion_amd import _lib as L
    out = np.empty(n_floats, np.float32)
    assert L.hip_runtime().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), out.nbytes, 2) == 0
    return out


def test_sphere():
    h, vba, want, _ = M.sphere_case()
    g = _ctx(**M.SMALL)
    _load(g, h, vba)
    _check("sphere", g, want)
    g.close()


def test_random_scene():
    """~60 % of 4 x 4 x 4 blocks around the origin, most of them chained in excess entries (16 buckets),
    shuffled VBA blocks, sdf over the whole short range with 0 / +-32767 frequent, w from {0, 0, 1, 5}:
    cube validity, all seven neighbour directions present and missing, every (tetrahedron, case) pair
    (asserted in tests/test_mesh_ref.py)."""
    h, vba, want, _ = M.random_case()
    g = _ctx(**M.RANDOM)
    _load(g, h, vba)
    _check("random scene", g, want)
    g.close()


def test_grid_boundary_and_beyond():
    """Blocks on both sides of the block grid's edges (x, y, z = 127 | 128 and -129 | -128) and a
    cluster far outside it: neighbours found through the grid, by the hash walk, and a mix of both
    within one cube."""
    from topfusion_amd.topfu import HASH_DTYPE, VOXEL_DTYPE
    pos = [(127, 0, 0), (128, 0, 0), (-129, 1, -1), (-128, 1, -1), (5, 127, 3), (5, 128, 3), (2, -129, 7), (2, -128, 7),
           (-4, 9, 127), (-4, 9, 128), (6, 6, -129), (6, 6, -128), (127, 127, 127), (128, 128, 128), (127, 128, 127),
           (-129, -129, -129), (-128, -128, -128), (-128, -129, -128)]
    pos += [(300 + dx, -200 + dy, 250 + dz) for dx, dy, dz in itertools.product((0, 1), repeat=3)]
    pos = np.array(pos)
    h, _, _ = synth.build_hash(pos, M.SMALL["n_buckets"], M.SMALL["n_excess"], HASH_DTYPE)
    rng = np.random.default_rng(3)
    vba = np.zeros(M.SMALL["n_blocks"] * 512, VOXEL_DTYPE)
    vba["sdf"] = rng.integers(-32768, 32768, vba.size)
    vba["w"] = rng.choice(np.array([0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 5], np.uint8), vba.size)
    want = M.extract(h, vba, M.VOXEL_SIZE, M.SMALL["n_buckets"])
    # cubes that reach across a block face exist on both sides of every edge
    assert len(want) > 5000
    g = _ctx(**M.SMALL)
    _load(g, h, vba)
    _check("grid boundary", g, want)
    g.close()


def test_capacity_and_arguments():
    from topfusion_amd import _lib as L
    lib = L.load()
    h, vba, want, _ = M.sphere_case()
    g = _ctx(**M.SMALL)
    _load(g, h, vba)
    n = len(want)
    half = n // 2
    sentinel = np.full(n * 9, 0xdeadbeef, np.uint32)
    buf = DeviceFrames(sentinel)
    got_n = ctypes.c_longlong(-1)
    L.check(lib.tf_mesh_extract(g._h, ctypes.c_void_p(buf.ptr), half, ctypes.byref(got_n)), "tf_mesh_extract")
    assert got_n.value == n                                       # the full count, whatever the capacity
    out = _download(buf.ptr, n * 9)
    assert_bit_exact("first half", out[:half * 9].reshape(-1, 3, 3), want[:half])
    assert np.array_equal(out[half * 9:].view(np.uint32), sentinel[half * 9:]), "wrote past the capacity"
    got_n.value = -1
    L.check(lib.tf_mesh_extract(g._h, None, 0, ctypes.byref(got_n)), "tf_mesh_extract")
    assert got_n.value == n                                       # count only
    assert np.array_equal(_download(buf.ptr, n * 9).view(np.uint32), out.view(np.uint32))
    assert lib.tf_mesh_extract(g._h, ctypes.c_void_p(buf.ptr), n, None) == L.TF_INVALID_ARG
    assert lib.tf_mesh_extract(g._h, ctypes.c_void_p(buf.ptr), -1, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    assert lib.tf_mesh_extract(g._h, None, 5, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    assert lib.tf_mesh_extract(None, ctypes.c_void_p(buf.ptr), n, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    buf.free()
    g.close()


def test_empty_and_swapped_out():
    """A freshly reset scene has no triangles; entries with ptr -1 (swapped out) are not meshed and
    their blocks are missing for the neighbours' cubes."""
    h, vba, full, _ = M.sphere_case()
    g = _ctx(**M.SMALL)
    assert g.mesh_count() == 0 and g.mesh().shape == (0, 3, 3)
    h = h.copy()
    live = np.nonzero(h["ptr"] >= 0)[0]
    h["ptr"][live[::5]] = -1
    want = M.extract(h, vba, M.VOXEL_SIZE, M.SMALL["n_buckets"])
    assert 0 < len(want) < len(full)
    _load(g, h, vba)
    _check("swapped out", g, want)
    g.reset()
    assert g.mesh_count() == 0
    g.close()


def test_pipeline():
    """Four frames of the synthetic orbit through TopFu, then mesh() straight after the frame call (the
    frame's deferred launches are flushed first): the mesh equals the reference applied to the
    downloaded scene, extraction leaves hash and VBA untouched, two extractions are byte-identical,
    and a twin context that never meshed is bit-identical after two further frames."""
    kw = dict(voxelSize=0.01, n_buckets=4096, n_excess=512, n_blocks=4096)
    g, twin = _ctx(**kw), _ctx(**kw)
    seq = synth.orbit_sequence(6, W, H, seed=7)
    for k in range(4):
        assert g(seq[k]) == twin(seq[k])
    tris = g.mesh()
    h, v = g.hash(), g.vba()
    assert len(tris) > 0
    assert_bit_exact("pipeline mesh", tris, M.extract(h, v, 0.01, 4096))
    again = g.mesh()
    assert tris.tobytes() == again.tobytes()
    assert g.hash().tobytes() == h.tobytes() and g.vba().tobytes() == v.tobytes()
    for k in range(4, 6):
        assert g(seq[k]) == twin(seq[k])
    assert g.getCameraPose().tobytes() == twin.getCameraPose().tobytes()
    assert g.stats() == twin.stats()
    assert g.hash().tobytes() == twin.hash().tobytes() and g.vba().tobytes() == twin.vba().tobytes()
    g.close()
    twin.close()


def test_save_mesh_file(tmp_path):
    from topfusion_amd import io
    h, vba, want, _ = M.sphere_case()
    g = _ctx(**M.SMALL)
    _load(g, h, vba)
    path = tmp_path / "sphere.ply"
    g.save_mesh(path)
    verts, faces = io.read_ply(path)
    assert_bit_exact("save_mesh", verts[faces], g.mesh())
    assert len(faces) == len(want)
    g.close()


def test_demo_headless_mesh(tmp_path):
    """demo_headless --mesh over a PGM sequence writes the mesh of the scene it fused: the same
    triangle list as mesh() of a Python context given the same frames and parameters."""
    from topfusion_amd import TopFu, default_params, io
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "apps")], check=True)
    seq = synth.orbit_sequence(3, W, H, seed=7)
    for i, f in enumerate(seq):
        io.write_pgm16(tmp_path / f"{i:04d}.pgm", f)
    path = tmp_path / "demo.ply"
    r = subprocess.run([os.path.join(ROOT, "apps", "demo_headless"), "--pgm", str(tmp_path / "%04d.pgm"), "--mesh", str(path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mesh written" in r.stdout
    s = W / 640.0                                                  # the demo's intrinsics: float constants scaled in double
    intr = [float(np.float32(float(np.float32(c)) * s)) for c in (synth.FX, synth.FY, synth.CX, synth.CY)]
    g = TopFu(default_params(cols=W, rows=H, fx=intr[0], fy=intr[1], cx=intr[2], cy=intr[3]))
    for f in seq:
        g(f)
    verts, faces = io.read_ply(path)
    tris = g.mesh()
    assert len(tris) > 0
    assert_bit_exact("demo mesh", verts[faces], tris)
    g.close()
