"""The whole map's indexed mesh on the GPU (tf_mesh_extract_indexed_whole, tf_mesh_save_ply_indexed_whole and the
layers above them; the slot-keyed kernels of topfusion_amd/csrc/tf_mesh.hip) against the composition of the two
numpy specifications (tests/mesh_indexed_whole_ref.py), bit for bit: both counts, every position and normal float,
every index.  The hand-made two-tier scene (its coverage is asserted on the CPU, tests/test_mesh_indexed_whole_ref.py),
scenes without stored data, the capacity and argument rules, the life of the slot scratch on one context, a scene
the swapping engine itself produced, the chunked files and the app."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_indexed_ref as X
import mesh_indexed_whole_ref as XW
import mesh_ref as M
import mesh_whole_ref as WR
from parity_util import DeviceFrames, assert_bit_exact
from test_gpu_mesh_whole import ENGINE, H, W, _classes, _ctx, _load_two_tier, _tiers, _turning_frames
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_whole(tag, g, want):
    """Counts and the three outputs against (vertices, indices, normals), and the identities against the soup."""
    v, f, n = want
    assert g.mesh_indexed_whole_count() == (len(v), len(f)), f"{tag}: {g.mesh_indexed_whole_count()}, reference {(len(v), len(f))}"
    gv, gf, gn = g.mesh_indexed_whole(normals=True)
    assert gv.shape == (len(v), 3) and gf.shape == (len(f), 3) and gf.dtype == np.uint32
    assert_bit_exact(f"{tag} indices", gf, f)
    assert_bit_exact(f"{tag} vertices", gv, v)
    assert_bit_exact(f"{tag} normals", gn, n)
    pv, pf, pn = g.mesh_indexed_whole()                                  # positions alone: the other instance of the kernel
    assert pn is None and pv.tobytes() == gv.tobytes() and pf.tobytes() == gf.tobytes()
    return gv, gf, gn


def _check_resident(tag, g, want):
    v, f, n, _ = want
    assert g.mesh_indexed_count() == (len(v), len(f)), tag
    gv, gf, gn, _ = g.mesh_indexed(normals=True)
    assert_bit_exact(f"{tag} indices", gf, f)
    assert_bit_exact(f"{tag} vertices", gv, v)
    assert_bit_exact(f"{tag} normals", gn, n)


def _want(c):
    return c["vertices"], c["indices"], c["vnormals"]


def test_two_tier_scene():
    """Every resolving class emits and owns edges of other entries' triangles, owners at all seven offsets and in
    excess entries, stored-only owners outside the block grid.  The soup identities hold, and the resident indexed
    form of the same context -- its own scratch -- still equals its reference on the unresolved tables."""
    c = XW.two_tier_indexed()
    g = _ctx(**M.RANDOM)
    _load_two_tier(g, c)
    gv, gf, gn = _check_whole("two tiers", g, _want(c))
    assert gv[gf].tobytes() == g.mesh(whole=True).tobytes()
    st, sn, _ = g.mesh_attr(normals=True, whole=True)
    assert gn[gf].tobytes() == sn.tobytes() and gv[gf].tobytes() == st.tobytes()
    resident = X.indexed(c["hash"], c["vba"], M.VOXEL_SIZE, M.RANDOM["n_buckets"])
    _check_resident("resident of the two-tier tables", g, resident)
    v2, f2, n2 = g.mesh_indexed_whole(normals=True)                       # determinism, and after a resident extraction
    assert v2.tobytes() == gv.tobytes() and f2.tobytes() == gf.tobytes() and n2.tobytes() == gn.tobytes()
    g.close()


@pytest.mark.parametrize("swapping", [False, True])
def test_no_stored_data(swapping):
    """Without stored data the whole indexed mesh is tf_mesh_extract_indexed's, byte for byte; an empty scene has none."""
    c = X.sphere_case()
    g = _ctx(swapping, **M.SMALL)
    assert g.mesh_indexed_whole_count() == (0, 0)
    v, f, n = g.mesh_indexed_whole(normals=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    from topfusion_amd import _lib as L
    g.upload(L.TF_BUF_HASH, c["hash"])
    g.upload(L.TF_BUF_VBA, c["vba"])
    assert g.mesh_indexed_whole_count() == g.mesh_indexed_count() == (len(c["vertices"]), len(c["indices"]))
    wv, wf, wn = g.mesh_indexed_whole(normals=True)
    rv, rf, rn, _ = g.mesh_indexed(normals=True)
    assert wv.tobytes() == rv.tobytes() == c["vertices"].tobytes()
    assert wf.tobytes() == rf.tobytes() == c["indices"].tobytes()
    assert wn.tobytes() == rn.tobytes() == c["normals"].tobytes()
    g.close()


def _download(buf, dtype=np.uint32):
    from topfusion_amd import _lib as L
    out = np.empty(buf.nbytes // np.dtype(dtype).itemsize, dtype)
    assert L.hip_runtime().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(buf.ptr), out.nbytes, 2) == 0
    return out


def test_capacity_and_arguments(tmp_path):
    from topfusion_amd import _lib as L
    lib = L.load()
    c = XW.two_tier_indexed()
    wv, wf, wn = _want(c)
    g = _ctx(**M.RANDOM)
    _load_two_tier(g, c)
    nv, nt = len(wv), len(wf)
    hv, ht = nv // 2, nt // 2
    sent = lambda n: np.full(n, 0xdeadbeef, np.uint32)
    bv, bn, bi = DeviceFrames(sent(nv * 3)), DeviceFrames(sent(nv * 3)), DeviceFrames(sent(nt * 3))
    P = lambda b: ctypes.c_void_p(b.ptr)
    gv, gt = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    call = lambda *a: lib.tf_mesh_extract_indexed_whole(g._h, *a, ctypes.byref(gv), ctypes.byref(gt))
    # vertices clipped at nv // 2, indices complete
    L.check(call(P(bv), P(bn), hv, P(bi), nt), "tf_mesh_extract_indexed_whole")
    assert (gv.value, gt.value) == (nv, nt)                              # the full counts, whatever the capacities
    ov, on, oi = _download(bv), _download(bn), _download(bi)
    assert ov[:hv * 3].tobytes() == wv[:hv].tobytes() and on[:hv * 3].tobytes() == wn[:hv].tobytes()
    for o in (ov, on):
        assert (o[hv * 3:] == 0xdeadbeef).all(), "wrote past the vertex capacity"
    assert oi.tobytes() == wf.tobytes() and (wf >= hv).any()             # an index keeps its true value past vertex_capacity
    # indices clipped at nt // 2, positions alone and complete
    bv2, bi2 = DeviceFrames(sent(nv * 3)), DeviceFrames(sent(nt * 3))
    gv.value = gt.value = -1
    L.check(call(P(bv2), None, nv, P(bi2), ht), "tf_mesh_extract_indexed_whole")
    assert (gv.value, gt.value) == (nv, nt)
    assert _download(bv2).tobytes() == wv.tobytes()
    oi2 = _download(bi2)
    assert oi2[:ht * 3].tobytes() == wf[:ht].tobytes() and (oi2[ht * 3:] == 0xdeadbeef).all(), "wrote past the triangle capacity"
    # one side only: a capacity of 0 writes nothing of that part
    bv3, bi3 = DeviceFrames(sent(nv * 3)), DeviceFrames(sent(nt * 3))
    L.check(call(None, None, 0, P(bi3), nt), "tf_mesh_extract_indexed_whole")
    assert _download(bi3).tobytes() == wf.tobytes()
    L.check(call(P(bv3), None, 0, P(bi3), 0), "tf_mesh_extract_indexed_whole")
    assert (_download(bv3) == 0xdeadbeef).all() and _download(bi3).tobytes() == wf.tobytes()
    L.check(call(None, P(bn), nv, None, 0), "tf_mesh_extract_indexed_whole")          # normals alone
    assert _download(bn).tobytes() == wn.tobytes()
    # count only
    gv.value = gt.value = -1
    L.check(call(None, None, 0, None, 0), "tf_mesh_extract_indexed_whole")
    assert (gv.value, gt.value) == (nv, nt)
    assert _download(bv).tobytes() == ov.tobytes() and _download(bi).tobytes() == oi.tobytes()
    # argument errors: every TF_INVALID_ARG of the header
    bad = L.TF_INVALID_ARG
    assert call(P(bv), None, -1, P(bi), nt) == bad
    assert call(P(bv), None, nv, P(bi), -1) == bad
    assert call(None, None, 5, P(bi), nt) == bad                          # a capacity without a buffer
    assert call(P(bv), None, nv, None, 5) == bad
    assert lib.tf_mesh_extract_indexed_whole(g._h, P(bv), None, nv, P(bi), nt, None, ctypes.byref(gt)) == bad
    assert lib.tf_mesh_extract_indexed_whole(g._h, P(bv), None, nv, P(bi), nt, ctypes.byref(gv), None) == bad
    assert lib.tf_mesh_extract_indexed_whole(None, P(bv), None, nv, P(bi), nt, ctypes.byref(gv), ctypes.byref(gt)) == bad
    path = str(tmp_path / "x.ply").encode()
    assert lib.tf_mesh_save_ply_indexed_whole(None, path, 0) == bad
    assert lib.tf_mesh_save_ply_indexed_whole(g._h, None, 0) == bad
    for attrs in (L.TF_MESH_COLOURS, L.TF_MESH_INDEXED, L.TF_MESH_WHOLE, L.TF_MESH_NORMALS | L.TF_MESH_COLOURS, 16):
        assert lib.tf_mesh_save_ply_indexed_whole(g._h, path, attrs) == bad, attrs
    assert lib.tf_mesh_save_ply_indexed_whole(g._h, str(tmp_path / "no" / "such" / "dir" / "x.ply").encode(), 0) == bad
    assert not (tmp_path / "x.ply").exists()
    # the old refusals stand
    assert lib.tf_mesh_save_ply_indexed(g._h, path, L.TF_MESH_WHOLE) == bad
    with pytest.raises(L.TfError) as e:
        g.save_mesh(tmp_path / "y.ply", indexed=True, whole=True)
    assert e.value.status == bad and not (tmp_path / "y.ply").exists()
    # the context is as usable as before
    assert g.mesh_indexed_whole_count() == (nv, nt)
    for b in (bv, bn, bi, bv2, bi2, bv3, bi3):
        b.free()
    g.close()


def test_scratch_life():
    """One context: a small scene first (few slots), then the two-tier scene (more entries resolve: the scratch
    grows), then the two-tier scene of another seed (other slots: a stale mask would show), then the whole and the
    resident extractions in alternation (separate scratch).  Every result equals its reference."""
    from topfusion_amd import _lib as L
    from topfusion_amd.topfu import HASH_DTYPE, VOXEL_DTYPE
    a, b = XW.two_tier_indexed(), XW.two_tier_indexed(1)
    cfg = M.RANDOM
    n_total = cfg["n_buckets"] + cfg["n_excess"]
    # the small scene: three neighbouring blocks, one of them stored only
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.int64)
    h, entry, _ = synth.build_hash(pos, cfg["n_buckets"], cfg["n_excess"], HASH_DTYPE)
    h["ptr"][entry] = [5, 9, -1]
    rng = np.random.default_rng(11)
    vba = np.zeros(cfg["n_blocks"] * 512, VOXEL_DTYPE)
    vba["sdf"] = rng.integers(-32768, 32768, vba.size)
    vba["w"] = rng.choice(np.array([0, 1, 1, 1, 5], np.uint8), vba.size)
    store = np.zeros(n_total * 512, VOXEL_DTYPE)
    store["sdf"] = rng.integers(-32768, 32768, store.size)
    store["w"] = rng.choice(np.array([0, 1, 1, 1, 5], np.uint8), store.size)
    state, flags = np.zeros(n_total, np.uint8), np.zeros(n_total, np.uint8)
    flags[entry[2]] = 1
    small = dict(hash=h, vba=vba, state=state, flags=flags, store=store)
    want_small = XW.indexed_whole(h, vba, state, flags, store, M.VOXEL_SIZE, cfg["n_buckets"])
    assert len(want_small[1]) > 0
    resolving = lambda c: int((WR.classify(c["hash"], c["state"], c["flags"]) >= 0).sum())
    assert resolving(small) == 3 < resolving(a), "the second scene does not grow the scratch"
    res_a = X.indexed(a["hash"], a["vba"], M.VOXEL_SIZE, cfg["n_buckets"])
    res_b = X.indexed(b["hash"], b["vba"], M.VOXEL_SIZE, cfg["n_buckets"])

    g = _ctx(**cfg)
    _load_two_tier(g, small)
    _check_whole("small scene", g, want_small)
    _load_two_tier(g, a)
    _check_whole("two tiers (the scratch grew)", g, _want(a))
    _load_two_tier(g, b)
    _check_whole("two tiers, another seed", g, _want(b))
    _check_resident("resident, another seed", g, res_b)
    _check_whole("two tiers, another seed, after a resident extraction", g, _want(b))
    _load_two_tier(g, a)
    _check_resident("resident, first seed", g, res_a)
    _check_whole("two tiers again", g, _want(a))
    _load_two_tier(g, small)
    _check_whole("small scene again (a scratch larger than needed)", g, want_small)
    g.close()


def test_engine_path(oracle_mod):
    """test_gpu_mesh_whole's turning camera through tf_scene_alloc / tf_scene_integrate / swap(): the whole indexed
    mesh equals the reference on the downloaded tiers, holds more vertices than the resident one, and a twin
    context that never meshed is identical in all five tier buffers and in its stats."""
    from topfusion_amd import _lib
    from test_gpu_engines import Pitched, _f, _ok
    L = _lib.load()
    frames = _turning_frames(oracle_mod)
    fx, fy, cx, cy = synth.intrinsics(W, H)
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
            assert g.mesh_indexed_whole_count()[1] > 0            # a meshing in mid-sequence: the frames after it must not see it
    h, vba, state, flags, store = _tiers(g)
    gc = _classes(h, state, flags)
    assert min(gc["stored"], gc["pending"], gc["merged"]) > 0, gc
    want = XW.indexed_whole(h, vba, state, flags, store, ENGINE["voxelSize"], ENGINE["n_buckets"])
    gv, gf, gn = _check_whole("engine", g, want)
    assert gv[gf].tobytes() == g.mesh(whole=True).tobytes()
    nv_res, nt_res = g.mesh_indexed_count()
    assert len(gv) > nv_res > 0 and len(gf) > nt_res > 0
    for name, a, b in zip(("hash", "vba", "swap state", "stored flags", "stored blocks"), _tiers(g), _tiers(twin)):
        assert a.tobytes() == b.tobytes(), f"{name}: the meshing context differs from its twin"
    assert g.stats() == twin.stats()
    dists.free()
    g.close()
    twin.close()


def test_save_files(tmp_path, monkeypatch):
    """save_mesh_indexed_whole under the default chunk size and under one small enough for several ragged chunks
    (1000 B: 41 vertex rows with normals, 83 without, 83 faces per chunk) writes one and the same file: the bytes
    tf_mesh_write_ply_indexed gives for the extracted arrays."""
    from topfusion_amd import _lib as L, io
    lib = L.load()
    c = XW.two_tier_indexed()
    wv, wf, wn = _want(c)
    assert len(wv) % 41 and len(wv) % 83 and len(wf) % 83, "no ragged last chunk"
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L.check(lib.tf_mesh_write_ply_indexed(str(tmp_path / "want.ply").encode(), P(wv), None, None, len(wv), P(wf), len(wf)), "write")
    L.check(lib.tf_mesh_write_ply_indexed(str(tmp_path / "want_n.ply").encode(), P(wv), P(wn), None, len(wv), P(wf), len(wf)), "write")
    monkeypatch.delenv("TFUSION_MESH_CHUNK_BYTES", raising=False)
    for tag, chunk in (("default", None), ("small", 1000)):
        if chunk:
            monkeypatch.setenv("TFUSION_MESH_CHUNK_BYTES", str(chunk))    # (read at tf_create)
        g = _ctx(**M.RANDOM)
        _load_two_tier(g, c)
        g.save_mesh_indexed_whole(tmp_path / f"{tag}.ply")
        g.save_mesh_indexed_whole(tmp_path / f"{tag}_n.ply", normals=True)
        assert (tmp_path / f"{tag}.ply").read_bytes() == (tmp_path / "want.ply").read_bytes(), tag
        assert (tmp_path / f"{tag}_n.ply").read_bytes() == (tmp_path / "want_n.ply").read_bytes(), tag
        if chunk:
            g.reset()                                                     # an empty map: a header, with the declared column
            g.save_mesh_indexed_whole(tmp_path / "empty.ply", normals=True)
            verts, faces, nrm, col = io.read_ply_attr(tmp_path / "empty.ply")
            assert len(verts) == 0 and len(faces) == 0 and nrm.shape == (0, 3) and col is None
        g.close()
    assert (tmp_path / "default_n.ply").read_bytes() == (tmp_path / "small_n.ply").read_bytes()
    verts, faces, nrm, col = io.read_ply_attr(tmp_path / "small_n.ply")
    assert col is None and verts.tobytes() == wv.tobytes() and nrm.tobytes() == wn.tobytes()
    assert np.array_equal(faces, wf.astype(np.int32))
    verts, faces = io.read_ply(tmp_path / "small.ply")
    assert_bit_exact("save_mesh_indexed_whole", verts[faces], c["tris"])


def test_mesh_whole_check_app_indexed(tmp_path):
    """apps/mesh_whole_check --indexed: the whole map through Scene::extractMeshIndexed and saveMeshIndexedWhole;
    the indexed file's faces dereference to the soup file the app already saves, triangle by triangle."""
    from topfusion_amd import io
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "apps"), "mesh_whole_check"], check=True)
    soup, indexed = tmp_path / "app.ply", tmp_path / "app_indexed.ply"
    r = subprocess.run([os.path.join(ROOT, "apps", "mesh_whole_check"), str(soup), "--indexed", str(indexed)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "MATCH" in r.stdout and "MISMATCH" not in r.stdout, r.stdout + r.stderr
    sv, sf = io.read_ply(soup)
    iv, itri, inrm, icol = io.read_ply_attr(indexed)
    assert icol is None and inrm.shape == iv.shape and len(itri) == len(sf) > 0
    assert f"indexed whole mesh: {len(iv)} vertices, {len(itri)} triangles\n" in r.stdout
    assert_bit_exact("the app's indexed file against its soup file", iv[itri], sv[sf])
    assert len(iv) >= len(sv)                                             # edges are never merged; the soup file is welded
