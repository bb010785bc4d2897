"""Indexed mesh extraction on the GPU (tf_mesh_extract_indexed and the layers above it, the kernels of
topfusion_amd/csrc/tf_mesh.hip) against the numpy restatement of its specification
(tests/mesh_indexed_ref.py), bit for bit: both counts, every position and normal float, every colour byte
and every index.  Scenes are built by hand (synth.build_hash + uploads) in small contexts, except the
pipeline and demo tests, which mesh what real frames fused."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import mesh_attr_ref as A
import mesh_indexed_ref as X
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


def _load(g, h, vba, rgb=None):
    from topfusion_amd import _lib as L
    g.upload(L.TF_BUF_HASH, h)
    g.upload(L.TF_BUF_VBA, vba)
    if rgb is not None:
        g.upload(L.TF_BUF_VBA_RGB, rgb)


def _check(tag, g, want, colours=True):
    """Counts and all four outputs against the reference (vertices, indices, normals, colours), and the
    invariants against the soup calls of the same context."""
    v, f, n, c = want
    assert g.mesh_indexed_count() == (len(v), len(f)), f"{tag}: {g.mesh_indexed_count()}, reference {(len(v), len(f))}"
    gv, gf, gn, gc = g.mesh_indexed(normals=True, colours=colours)
    assert gv.shape == (len(v), 3) and gf.shape == (len(f), 3) and gf.dtype == np.uint32
    assert_bit_exact(f"{tag} indices", gf, f)
    assert_bit_exact(f"{tag} vertices", gv, v)
    assert_bit_exact(f"{tag} normals", gn, n)
    if colours:
        assert_bit_exact(f"{tag} colours", gc, c)
    else:
        assert gc is None
    # positions alone come from another instance of the kernel
    pv, pf, pn, pc = g.mesh_indexed()
    assert pn is None and pc is None and pv.tobytes() == gv.tobytes() and pf.tobytes() == gf.tobytes()
    assert gv[gf].tobytes() == g.mesh().tobytes()
    if colours:
        st, sn, sc = g.mesh_attr(True, True)
        assert gn[gf].tobytes() == sn.tobytes() and gc[gf].tobytes() == sc.tobytes() and gv[gf].tobytes() == st.tobytes()
        cv, cf, cn, cc = g.mesh_indexed(colours=True)                 # colours alone: the third instance
        assert cn is None and cc.tobytes() == gc.tobytes() and cv.tobytes() == gv.tobytes()


def _download(buf, dtype):
    from topfusion_amd import _lib as L
    out = np.empty(buf.nbytes // np.dtype(dtype).itemsize, dtype)
    assert L.hip_runtime().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(buf.ptr), out.nbytes, 2) == 0
    return out


def _want(c):
    return c["vertices"], c["indices"], c["normals"], c["colours"]


@pytest.mark.parametrize("name", ["sphere", "dense"])
def test_scene(name):
    """The closed sphere, and the dense random scene: owners at every block offset and in excess entries,
    distinct edges with bit-equal positions (asserted where the scene is built, tests/mesh_indexed_ref.py)."""
    c = X._case(name)
    g = _ctx(voxel_rgb=1, **c["cfg"])
    _load(g, c["hash"], c["vba"], c["rgb"])
    _check(name, g, _want(c))
    g.close()


def _boundary_scene():
    from topfusion_amd.topfu import HASH_DTYPE, VOXEL_DTYPE
    pos = [(127, 0, 0), (128, 0, 0), (-129, 1, -1), (-128, 1, -1), (5, 127, 3), (5, 128, 3), (2, -129, 7), (2, -128, 7),
           (-4, 9, 127), (-4, 9, 128), (6, 6, -129), (6, 6, -128), (127, 127, 127), (128, 128, 128), (127, 128, 127),
           (-129, -129, -129), (-128, -128, -128), (-128, -129, -128)]
    pos += [(300 + dx, -200 + dy, 250 + dz) for dx, dy, dz in itertools.product((0, 1), repeat=3)]
    h, _, _ = synth.build_hash(np.array(pos), M.SMALL["n_buckets"], M.SMALL["n_excess"], HASH_DTYPE)
    rng = np.random.default_rng(3)
    vba = np.zeros(M.SMALL["n_blocks"] * 512, VOXEL_DTYPE)
    vba["sdf"] = rng.integers(-32768, 32768, vba.size)
    vba["w"] = rng.choice(np.array([0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 5], np.uint8), vba.size)
    return h, vba


def test_grid_boundary_and_beyond():
    """test_gpu_mesh.py::test_grid_boundary_and_beyond's block set: owners found through the block grid, by
    the hash walk, and by both within one cube."""
    h, vba = _boundary_scene()
    rgb = A.colour_plane(vba.size, seed=8)
    stats = {}
    want = X.indexed(h, vba, M.VOXEL_SIZE, M.SMALL["n_buckets"], rgb, stats=stats)
    assert stats["nt"] > 5000 and len(stats["owner_dirs"]) > 1
    g = _ctx(voxel_rgb=1, **M.SMALL)
    _load(g, h, vba, rgb)
    _check("grid boundary", g, want)
    g.close()


def test_empty_and_swapped_out():
    """A reset scene has no vertices and no triangles; entries with ptr -1 (swapped out) are not meshed, own
    nothing, and their blocks are missing for the neighbours' cubes.  A context without the colour plane."""
    c = X.sphere_case()
    g = _ctx(**M.SMALL)
    assert g.mesh_indexed_count() == (0, 0)
    v, f, n, col = g.mesh_indexed(normals=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3) and col is None
    h = c["hash"].copy()
    live = np.nonzero(h["ptr"] >= 0)[0]
    h["ptr"][live[::5]] = -1
    want = X.indexed(h, c["vba"], M.VOXEL_SIZE, M.SMALL["n_buckets"])
    assert 0 < len(want[1]) < len(c["indices"])
    _load(g, h, c["vba"])
    _check("swapped out", g, want, colours=False)
    g.reset()
    assert g.mesh_indexed_count() == (0, 0)
    g.close()


def test_capacity_and_arguments():
    from topfusion_amd import _lib as L
    lib = L.load()
    c = X.sphere_case()
    wv, wf, wn, wc = _want(c)
    g = _ctx(voxel_rgb=1, **M.SMALL)
    _load(g, c["hash"], c["vba"], c["rgb"])
    nv, nt = len(wv), len(wf)
    hv, ht = nv // 2, nt // 2
    sent = lambda n: np.full(n, 0xdeadbeef, np.uint32)
    bv, bn, bc, bi = DeviceFrames(sent(nv * 3)), DeviceFrames(sent(nv * 3)), DeviceFrames(sent(nv)), DeviceFrames(sent(nt * 3))
    P = lambda b: ctypes.c_void_p(b.ptr)
    gv, gt = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    call = lambda *a: lib.tf_mesh_extract_indexed(g._h, *a, ctypes.byref(gv), ctypes.byref(gt))
    # vertices clipped at nv // 2, indices whole
    L.check(call(P(bv), P(bn), P(bc), hv, P(bi), nt), "tf_mesh_extract_indexed")
    assert (gv.value, gt.value) == (nv, nt)                              # the full counts, whatever the capacities
    ov, on, oc, oi = _download(bv, np.uint32), _download(bn, np.uint32), _download(bc, np.uint32), _download(bi, np.uint32)
    assert ov[:hv * 3].tobytes() == wv[:hv].tobytes() and on[:hv * 3].tobytes() == wn[:hv].tobytes()
    assert oc[:hv].tobytes() == wc[:hv].tobytes()
    for o, k in ((ov, 3), (on, 3), (oc, 1)):
        assert (o[hv * k:] == 0xdeadbeef).all(), "wrote past the vertex capacity"
    assert oi.tobytes() == wf.tobytes() and (wf >= hv).any()             # indices past the clipped table keep their values
    # indices clipped at nt // 2, positions alone and whole
    bv2, bi2 = DeviceFrames(sent(nv * 3)), DeviceFrames(sent(nt * 3))
    gv.value = gt.value = -1
    L.check(call(P(bv2), None, None, nv, P(bi2), ht), "tf_mesh_extract_indexed")
    assert (gv.value, gt.value) == (nv, nt)
    assert _download(bv2, np.uint32).tobytes() == wv.tobytes()
    oi2 = _download(bi2, np.uint32)
    assert oi2[:ht * 3].tobytes() == wf[:ht].tobytes() and (oi2[ht * 3:] == 0xdeadbeef).all(), "wrote past the triangle capacity"
    # one side only: the other's capacity 0 writes nothing there
    bv3, bi3 = DeviceFrames(sent(nv * 3)), DeviceFrames(sent(nt * 3))
    L.check(call(None, None, None, 0, P(bi3), nt), "tf_mesh_extract_indexed")
    assert _download(bi3, np.uint32).tobytes() == wf.tobytes()
    L.check(call(P(bv3), None, None, 0, P(bi3), 0), "tf_mesh_extract_indexed")
    assert (_download(bv3, np.uint32) == 0xdeadbeef).all() and _download(bi3, np.uint32).tobytes() == wf.tobytes()
    # count only
    gv.value = gt.value = -1
    L.check(call(None, None, None, 0, None, 0), "tf_mesh_extract_indexed")
    assert (gv.value, gt.value) == (nv, nt)
    assert _download(bv, np.uint32).tobytes() == ov.tobytes() and _download(bi, np.uint32).tobytes() == oi.tobytes()
    # argument errors
    bad = L.TF_INVALID_ARG
    assert call(P(bv), None, None, -1, P(bi), nt) == bad
    assert call(P(bv), None, None, nv, P(bi), -1) == bad
    assert call(None, None, None, 5, P(bi), nt) == bad                    # a capacity without a buffer
    assert call(P(bv), None, None, nv, None, 5) == bad
    assert lib.tf_mesh_extract_indexed(g._h, P(bv), None, None, nv, P(bi), nt, None, ctypes.byref(gt)) == bad
    assert lib.tf_mesh_extract_indexed(g._h, P(bv), None, None, nv, P(bi), nt, ctypes.byref(gv), None) == bad
    assert lib.tf_mesh_extract_indexed(None, P(bv), None, None, nv, P(bi), nt, ctypes.byref(gv), ctypes.byref(gt)) == bad
    plain = _ctx(**M.SMALL)
    assert lib.tf_mesh_extract_indexed(plain._h, P(bv), None, P(bc), nv, P(bi), nt, ctypes.byref(gv), ctypes.byref(gt)) == bad
    assert lib.tf_mesh_save_ply_indexed(plain._h, b"/dev/null", L.TF_MESH_COLOURS) == bad
    with pytest.raises(L.TfError):
        plain.mesh_indexed(colours=True)
    plain.close()
    assert lib.tf_mesh_save_ply_indexed(g._h, None, 0) == bad and lib.tf_mesh_save_ply_indexed(g._h, b"/dev/null", 8) == bad
    for b in (bv, bn, bc, bi, bv2, bi2, bv3, bi3):
        b.free()
    g.close()


def test_stale_masks():
    """One context, two scenes that use the same VBA block numbers: the second extraction must not see the
    first one's edge bits."""
    a, b = X.sphere_case(), X.dense_case()
    g = _ctx(voxel_rgb=1, **M.RANDOM)
    # the sphere in the random scene's capacities: its own hash there
    from topfusion_amd.topfu import HASH_DTYPE
    pos = np.array(list(itertools.product(range(4), repeat=3)), np.int64)
    h, _, _ = synth.build_hash(pos, M.RANDOM["n_buckets"], M.RANDOM["n_excess"], HASH_DTYPE)
    first = X.indexed(h, a["vba"], M.VOXEL_SIZE, M.RANDOM["n_buckets"], a["rgb"])
    assert set(h["ptr"][h["ptr"] >= 0]) & set(b["hash"]["ptr"][b["hash"]["ptr"] >= 0]), "the scenes share no VBA block"
    _load(g, h, a["vba"], a["rgb"])
    _check("first scene", g, first)
    _load(g, b["hash"], b["vba"], b["rgb"])
    _check("second scene", g, _want(b))
    _load(g, h, a["vba"], a["rgb"])
    _check("first scene again", g, first)
    g.close()


def test_pipeline():
    """Four frames of the synthetic orbit through TopFu, then mesh_indexed() straight after the frame call:
    the indexed mesh equals the reference applied to the downloaded scene, two extractions are byte-identical
    (the marks are atomic ORs), a mesh() in between disturbs neither, hash and VBA are untouched, and a twin
    context that never meshed is bit-identical after two further frames."""
    kw = dict(voxelSize=0.01, n_buckets=4096, n_excess=512, n_blocks=4096)
    g, twin = _ctx(**kw), _ctx(**kw)
    seq = synth.orbit_sequence(6, W, H, seed=7)
    for k in range(4):
        assert g(seq[k]) == twin(seq[k])
    v, f, n, _ = g.mesh_indexed(normals=True)
    h, vox = g.hash(), g.vba()
    assert len(f) > 0
    wv, wf, wn, _ = X.indexed(h, vox, 0.01, 4096)
    assert_bit_exact("pipeline indices", f, wf)
    assert_bit_exact("pipeline vertices", v, wv)
    assert_bit_exact("pipeline normals", n, wn)
    soup = g.mesh()                                                     # the soup call's scratch beside the indexed one's
    assert v[f].tobytes() == soup.tobytes()
    v2, f2, n2, _ = g.mesh_indexed(normals=True)
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes() and n2.tobytes() == n.tobytes()
    assert g.mesh().tobytes() == soup.tobytes()
    assert g.hash().tobytes() == h.tobytes() and g.vba().tobytes() == vox.tobytes()
    for k in range(4, 6):
        assert g(seq[k]) == twin(seq[k])
    assert g.getCameraPose().tobytes() == twin.getCameraPose().tobytes()
    assert g.stats() == twin.stats()
    assert g.hash().tobytes() == twin.hash().tobytes() and g.vba().tobytes() == twin.vba().tobytes()
    g.close()
    twin.close()


def test_save_mesh_file(tmp_path):
    from topfusion_amd import io
    c = X.sphere_case()
    g = _ctx(voxel_rgb=1, **M.SMALL)
    _load(g, c["hash"], c["vba"], c["rgb"])
    path = tmp_path / "sphere.ply"
    g.save_mesh(path, indexed=True)
    verts, faces = io.read_ply(path)
    assert_bit_exact("save_mesh indexed", verts[faces], g.mesh())
    assert len(verts) == len(c["vertices"]) and verts.tobytes() == c["vertices"].tobytes()
    path = tmp_path / "sphere_attr.ply"
    g.save_mesh(path, normals=True, colours=True, indexed=True)
    verts, faces, nrm, col = io.read_ply_attr(path)
    assert verts.tobytes() == c["vertices"].tobytes() and np.array_equal(faces, c["indices"].astype(np.int32))
    assert nrm.tobytes() == c["normals"].tobytes() and col.tobytes() == c["colours"].tobytes()
    g.reset()
    path = tmp_path / "empty.ply"
    g.save_mesh(path, normals=True, indexed=True)
    verts, faces, nrm, col = io.read_ply_attr(path)
    assert len(verts) == 0 and len(faces) == 0 and nrm.shape == (0, 3) and col is None
    g.close()


def test_demo_headless_mesh_indexed(tmp_path):
    """demo_headless --mesh out.ply --mesh-indexed writes the indexed mesh of the scene it fused: verts[faces]
    is mesh() of a Python context given the same frames, and the vertex table is mesh_indexed()'s."""
    from topfusion_amd import TopFu, default_params, io
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "apps")], check=True)
    seq = synth.orbit_sequence(3, W, H, seed=7)
    for i, f in enumerate(seq):
        io.write_pgm16(tmp_path / f"{i:04d}.pgm", f)
    path = tmp_path / "demo.ply"
    r = subprocess.run([os.path.join(ROOT, "apps", "demo_headless"), "--pgm", str(tmp_path / "%04d.pgm"), "--mesh", str(path),
                        "--mesh-indexed"], capture_output=True, text=True, timeout=120)
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
    nv, nt = g.mesh_indexed_count()
    assert (len(verts), len(faces)) == (nv, nt)
    assert verts.tobytes() == g.mesh_indexed()[0].tobytes()
    assert f"indexed mesh: {nv} vertices, {nt} triangles, highest index {nv - 1}\n" in r.stdout     # TopFu::extractMeshIndexed
    g.close()
