"""Mesh extraction with per-vertex attributes on the GPU (tf_mesh_extract_attr and the layers above it,
k_mesh_emit_attr in topfusion_amd/csrc/tf_mesh.hip) against the numpy restatement of its specification
(tests/mesh_attr_ref.py), bit for bit: the triangle count, every position and normal float and every
colour byte, in order.  Scenes are built by hand (synth.build_hash + uploads of hash, VBA and colour
plane) in small colour contexts, except the pipeline and demo tests, which mesh what real frames fused."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import mesh_attr_ref as A
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


def _check(tag, g, tris, normals, colours):
    """All three outputs of mesh_attr against the reference, and the positions against mesh()."""
    n = g.mesh_count()
    assert n == len(tris), f"{tag}: {n} triangles, reference {len(tris)}"
    gt, gn, gc = g.mesh_attr(normals=True, colours=colours is not None)
    assert_bit_exact(f"{tag} positions", gt, tris)
    assert_bit_exact(f"{tag} normals", gn, normals)
    if colours is not None:
        assert_bit_exact(f"{tag} colours", gc, colours)
    else:
        assert gc is None
    assert gt.tobytes() == g.mesh().tobytes()


def _download(buf, dtype):
    from topfusion_amd import _lib as L
    out = np.empty(buf.nbytes // np.dtype(dtype).itemsize, dtype)
    assert L.hip_runtime().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(buf.ptr), out.nbytes, 2) == 0
    return out


@pytest.mark.parametrize("name", ["sphere", "random", "slab"])
def test_scene(name):
    """The closed sphere (central gradients only), the random scene (every gradient and colour rule, -1
    neighbours from other blocks, blocks chained in excess entries: asserted in tests/test_mesh_attr_ref.py)
    and the slab (normals that vanish)."""
    h, vba, rgb, tris, normals, colours, _ = A._case(name)
    g = _ctx(voxel_rgb=1, **(M.RANDOM if name == "random" else M.SMALL))
    _load(g, h, vba, rgb)
    _check(name, g, tris, normals, colours)
    g.close()


def test_grid_boundary_and_short_range():
    """Blocks on both sides of the block grid's edges and a cluster far outside it (neighbours through
    the grid, by the hash walk, and both within one tile), plus blocks at coordinate -32768 and 32767
    on each axis: their -1 / +1 neighbours leave the short range and are missing, not wrapped."""
    from topfusion_amd.topfu import HASH_DTYPE, VOXEL_DTYPE
    pos = [(127, 0, 0), (128, 0, 0), (-129, 1, -1), (-128, 1, -1), (5, 127, 3), (5, 128, 3), (2, -129, 7), (2, -128, 7),
           (-4, 9, 127), (-4, 9, 128), (6, 6, -129), (6, 6, -128), (127, 127, 127), (128, 128, 128), (127, 128, 127),
           (-129, -129, -129), (-128, -128, -128), (-128, -129, -128)]
    pos += [(300 + dx, -200 + dy, 250 + dz) for dx, dy, dz in itertools.product((0, 1), repeat=3)]
    edge = [(-32768, 3, 4), (32767, 3, 4), (1, -32768, 2), (1, 32767, 2), (7, 7, -32768), (7, 7, 32767),
            (32767, 3, 5), (-32768, 4, 4)]    # (a wrapped coordinate would find the far end's block of the same row)
    pos = np.array(pos + edge)
    h, _, _ = synth.build_hash(pos, M.SMALL["n_buckets"], M.SMALL["n_excess"], HASH_DTYPE)
    rng = np.random.default_rng(3)
    vba = np.zeros(M.SMALL["n_blocks"] * 512, VOXEL_DTYPE)
    vba["sdf"] = rng.integers(-32768, 32768, vba.size)
    vba["w"] = rng.choice(np.array([0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 5], np.uint8), vba.size)
    rgb = A.colour_plane(vba.size, seed=8)
    tris, normals, colours = A.extract_attr(h, vba, rgb, M.VOXEL_SIZE, M.SMALL["n_buckets"])
    assert tris.tobytes() == M.extract(h, vba, M.VOXEL_SIZE, M.SMALL["n_buckets"]).tobytes()
    assert len(tris) > 5000
    x = tris[..., 0] / np.float32(M.VOXEL_SIZE)
    assert (x < -32768 * 8 + 8).any() and (x > 32767 * 8).any()      # the blocks at the range's ends are meshed
    g = _ctx(voxel_rgb=1, **M.SMALL)
    _load(g, h, vba, rgb)
    _check("grid boundary", g, tris, normals, colours)
    g.close()


def test_swapped_out_neighbours():
    """Every fifth live entry of the sphere swapped out (ptr -1): those blocks are missing for their
    neighbours' tiles, so gradients next to them turn one-sided -- also towards -x alone."""
    h, vba, rgb, full, _, _, _ = A.sphere_case()
    h = h.copy()
    live = np.nonzero(h["ptr"] >= 0)[0]
    h["ptr"][live[::5]] = -1
    state = {(int(e["x"]), int(e["y"]), int(e["z"])): int(e["ptr"]) for e in h[h["ptr"] >= -1]}
    others = [(1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    # a live block whose -x neighbour is swapped out and whose five other face neighbours are not
    alone = [b for b, p in state.items() if p >= 0 and state.get((b[0] - 1, b[1], b[2])) == -1
             and all(state.get((b[0] + d[0], b[1] + d[1], b[2] + d[2]), 0) != -1 for d in others)]
    assert alone, "no block whose -x neighbour alone is swapped out"
    stats = {}
    tris, normals, colours = A.extract_attr(h, vba, rgb, M.VOXEL_SIZE, M.SMALL["n_buckets"], stats=stats)
    assert 0 < len(tris) < len(full)
    assert (stats["rules"][:, 1:3] > 0).all(), stats["rules"]          # one-sided both ways on every axis
    g = _ctx(voxel_rgb=1, **M.SMALL)
    _load(g, h, vba, rgb)
    _check("swapped out", g, tris, normals, colours)
    g.close()


def test_capacity_and_arguments():
    from topfusion_amd import _lib as L
    lib = L.load()
    h, vba, rgb, tris, normals, colours, _ = A.sphere_case()
    g = _ctx(voxel_rgb=1, **M.SMALL)
    _load(g, h, vba, rgb)
    n = len(tris)
    half = n // 2
    want = (tris.reshape(n, 9).view(np.uint32), normals.reshape(n, 9).view(np.uint32), colours.reshape(n, 3, 4).view(np.uint32).reshape(n, 3))
    sentinel = [np.full((n, k), 0xdeadbeef, np.uint32) for k in (9, 9, 3)]
    got_n = ctypes.c_longlong(-1)

    def run(mask, cap):
        """Fresh sentinel buffers, one call with the outputs of `mask`, the three buffers downloaded."""
        bufs = [DeviceFrames(s) for s in sentinel]
        ptrs = [ctypes.c_void_p(b.ptr) if mask >> i & 1 else None for i, b in enumerate(bufs)]
        got_n.value = -1
        L.check(lib.tf_mesh_extract_attr(g._h, ptrs[0], ptrs[1], ptrs[2], cap, ctypes.byref(got_n)), "tf_mesh_extract_attr")
        assert got_n.value == n                                   # the full count, whatever the capacity
        out = [_download(b, np.uint32).reshape(s.shape) for b, s in zip(bufs, sentinel)]
        for b in bufs:
            b.free()
        return out

    # half capacity: all three clipped at the same triangle, sentinels intact behind it
    for o, w_, s in zip(run(7, half), want, sentinel):
        assert np.array_equal(o[:half], w_[:half])
        assert np.array_equal(o[half:], s[half:]), "wrote past the capacity"
    # every subset of the outputs: the chosen ones complete, the skipped buffers untouched
    for mask in range(1, 8):
        for i, (o, w_, s) in enumerate(zip(run(mask, n), want, sentinel)):
            assert np.array_equal(o, w_ if mask >> i & 1 else s), (mask, i)
    # count only
    for o, s in zip(run(0, 0), sentinel):
        assert np.array_equal(o, s)
    buf = DeviceFrames(sentinel[0])
    p = ctypes.c_void_p(buf.ptr)
    assert lib.tf_mesh_extract_attr(g._h, p, None, None, n, None) == L.TF_INVALID_ARG
    assert lib.tf_mesh_extract_attr(g._h, None, p, None, -1, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    assert lib.tf_mesh_extract_attr(g._h, None, None, None, 5, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    assert lib.tf_mesh_extract_attr(None, p, None, None, n, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    assert lib.tf_mesh_save_ply_attr(g._h, None, 1) == L.TF_INVALID_ARG
    assert lib.tf_mesh_save_ply_attr(g._h, b"x.ply", 4) == L.TF_INVALID_ARG
    g.close()
    # colours need the colour plane
    g = _ctx(**M.SMALL)
    _load(g, h, vba)
    assert lib.tf_mesh_extract_attr(g._h, None, None, p, n, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    assert lib.tf_mesh_extract_attr(g._h, p, p, p, 0, ctypes.byref(got_n)) == L.TF_INVALID_ARG
    assert lib.tf_mesh_save_ply_attr(g._h, b"x.ply", L.TF_MESH_COLOURS) == L.TF_INVALID_ARG
    assert lib.tf_mesh_save_ply_attr(g._h, b"x.ply", L.TF_MESH_NORMALS | L.TF_MESH_COLOURS) == L.TF_INVALID_ARG
    with pytest.raises(L.TfError):
        g.mesh_attr(normals=False, colours=True)
    assert not os.path.exists("x.ply")
    # ... normals do not
    gt, gn, gc = g.mesh_attr()
    assert gc is None
    assert_bit_exact("normals without a colour plane", gn, normals)
    assert_bit_exact("positions without a colour plane", gt, tris)
    buf.free()
    g.close()


def test_pipeline():
    """Four RGB-D frames of the synthetic orbit through a colour context (TopFu()(depth, rgb=...), as
    tests/test_gpu_colour.py drives it), then mesh_attr straight after the frame call: all three outputs
    equal the reference applied to the downloaded hash, VBA and colour plane; extraction leaves them
    untouched; two extractions are byte-identical; a twin context that never meshed is bit-identical
    after two further frames."""
    kw = dict(voxelSize=0.01, n_buckets=4096, n_excess=512, n_blocks=4096, voxel_rgb=1)
    g, twin = _ctx(**kw), _ctx(**kw)
    seq = synth.orbit_sequence(6, W, H, seed=7)
    rgbs = [synth.render_colour(*synth.orbit_pose(k), W, H) for k in range(6)]
    for k in range(4):
        assert g(seq[k], rgb=rgbs[k]) == twin(seq[k], rgb=rgbs[k])
    got = g.mesh_attr(normals=True, colours=True)
    h, v, c = g.hash(), g.vba(), g.vba_rgb()
    assert len(got[0]) > 0
    want = A.extract_attr(h, v, c, 0.01, 4096)
    for name, a, b in zip(("positions", "normals", "colours"), got, want):
        assert_bit_exact(f"pipeline {name}", a, b)
    print(f"vertices with colour: {(got[2][..., 3] == 255).mean():.3f}")
    assert (got[2][..., 3] == 255).any()                           # the surface was seen in colour
    length = np.linalg.norm(got[1].astype(np.float64), axis=-1)
    assert np.all((np.abs(length - 1) < 1e-6) | (length == 0))
    again = g.mesh_attr(normals=True, colours=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    assert g.hash().tobytes() == h.tobytes() and g.vba().tobytes() == v.tobytes() and g.vba_rgb().tobytes() == c.tobytes()
    for k in range(4, 6):
        assert g(seq[k], rgb=rgbs[k]) == twin(seq[k], rgb=rgbs[k])
    assert g.getCameraPose().tobytes() == twin.getCameraPose().tobytes()
    assert g.stats() == twin.stats()
    assert g.hash().tobytes() == twin.hash().tobytes() and g.vba().tobytes() == twin.vba().tobytes()
    assert g.vba_rgb().tobytes() == twin.vba_rgb().tobytes()
    g.close()
    twin.close()


def test_save_mesh_files(tmp_path):
    """save_mesh with attributes read back equals the welded reference; without, it writes the file it
    always wrote (tf_mesh_save_ply's, and tf_mesh_write_ply's of mesh())."""
    from topfusion_amd import io
    from topfusion_amd import _lib as L
    h, vba, rgb, tris, normals, colours, _ = A.random_case()
    g = _ctx(voxel_rgb=1, **M.RANDOM)
    _load(g, h, vba, rgb)
    for nr, co in ((normals, colours), (normals, None), (None, colours)):
        path = tmp_path / "attr.ply"
        g.save_mesh(path, normals=nr is not None, colours=co is not None)
        verts, faces, vn, vc = io.read_ply_attr(path)
        assert_bit_exact("save_mesh positions", verts[faces], tris)
        assert (vn is None) == (nr is None) and (vc is None) == (co is None)
        if nr is not None:
            assert_bit_exact("save_mesh normals", vn[faces], nr)
        if co is not None:
            assert_bit_exact("save_mesh colours", vc[faces], co)
        assert len(verts) == len(A.weld(tris, nr, co)[0])
    plain, old, ref = tmp_path / "plain.ply", tmp_path / "old.ply", tmp_path / "ref.ply"
    g.save_mesh(plain)
    L.check(L.load().tf_mesh_save_ply(g._h, str(old).encode()), "tf_mesh_save_ply")
    io.write_ply(ref, g.mesh())
    assert plain.read_bytes() == old.read_bytes() == ref.read_bytes()
    L.check(L.load().tf_mesh_save_ply_attr(g._h, str(plain).encode(), 0), "tf_mesh_save_ply_attr")
    assert plain.read_bytes() == old.read_bytes()
    g.reset()
    g.save_mesh(plain, normals=True, colours=True)                   # an empty scene: the columns, no records
    verts, faces, vn, vc = io.read_ply_attr(plain)
    assert len(verts) == 0 and len(faces) == 0 and vn.shape == (0, 3) and vc.shape == (0, 4)
    g.close()


def test_demo_headless_mesh_normals(tmp_path):
    """demo_headless --mesh f.ply --mesh-normals writes positions and normals of the scene it fused: the
    header lists nx ny nz, normals are unit or zero, and both equal mesh_attr() of a Python context given
    the same frames and parameters."""
    from topfusion_amd import TopFu, default_params, io
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "apps")], check=True)
    seq = synth.orbit_sequence(3, W, H, seed=7)
    for i, f in enumerate(seq):
        io.write_pgm16(tmp_path / f"{i:04d}.pgm", f)
    path = tmp_path / "demo.ply"
    r = subprocess.run([os.path.join(ROOT, "apps", "demo_headless"), "--pgm", str(tmp_path / "%04d.pgm"), "--mesh", str(path),
                        "--mesh-normals"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mesh written" in r.stdout
    header = path.read_bytes().split(b"end_header\n")[0]
    assert b"property float nx\nproperty float ny\nproperty float nz\n" in header and b"red" not in header
    verts, faces, vn, vc = io.read_ply_attr(path)
    assert vc is None and len(faces) > 0
    length = np.linalg.norm(vn.astype(np.float64), axis=-1)
    assert np.all((np.abs(length - 1) < 1e-6) | (length == 0))
    s = W / 640.0                                                  # the demo's intrinsics: float constants scaled in double
    intr = [float(np.float32(float(np.float32(c)) * s)) for c in (synth.FX, synth.FY, synth.CX, synth.CY)]
    g = TopFu(default_params(cols=W, rows=H, fx=intr[0], fy=intr[1], cx=intr[2], cy=intr[3]))
    for f in seq:
        g(f)
    tris, normals, _ = g.mesh_attr()
    assert_bit_exact("demo positions", verts[faces], tris)
    assert_bit_exact("demo normals", vn[faces], normals)
    g.close()
