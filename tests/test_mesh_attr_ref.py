"""The mesh attributes' specification on the CPU (tests/mesh_attr_ref.py, DESIGN.md §Mesh extraction,
attributes): the sphere's normals are unit, radial and agree with the triangles' orientation; the
random scene meets every rule the GPU comparison (tests/test_gpu_mesh_attr.py) must cover; the slab's
normals vanish exactly where the specification says; the byte rounding of colours; the attributed
PLY writer and reader round trip; and the shared per-vertex functions of tf_mesh.h, compiled as host
C++, give the reference's bits.  The library is loaded for its host-only PLY writer; nothing here
needs a GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import mesh_attr_ref as A
import mesh_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sphere_normals():
    """Unit length to float rounding (each component and L carry half an ulp: |1 - |n|| <= 4 * 2^-24),
    radial (dot >= 1 - 1e-4; measured minimum 0.9999845 over the 4 844 crossed edges), every gradient
    central (all 9 688 ends per axis), and consistent with the triangles' right-hand orientation."""
    _, _, _, tris, normals, _, stats = A.sphere_case()
    n = normals.astype(np.float64)
    length = np.linalg.norm(n, axis=-1)
    print(f"|n| in [{length.min():.9f}, {length.max():.9f}]")
    assert np.all(np.abs(length - 1) <= 4 * 2.0 ** -24)
    p = tris.astype(np.float64) / M.VOXEL_SIZE - np.array(M.SPHERE_C)
    radial = p / np.linalg.norm(p, axis=-1, keepdims=True)
    dot = (radial * n).sum(-1)
    print(f"min normal . radial {dot.min():.7f} over {stats['edges']} edges")
    assert dot.min() >= 1 - 1e-4
    assert stats["zero"] == 0
    assert np.array_equal(stats["rules"][:, 1:], np.zeros((3, 3), int)), stats["rules"]
    assert (stats["rules"][:, 0] == 2 * stats["edges"]).all()
    t = tris.astype(np.float64)
    geo = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    assert np.all(np.linalg.norm(geo, axis=-1) > 0)                   # no zero-area triangle on the sphere
    assert np.all((n.sum(1) * geo).sum(-1) > 0)


def test_random_scene_covers_every_rule():
    """Coverage of the random scene (mesh_ref.random_case() with the seed-5 colour plane, ~30 % of the
    words without colour): per axis each reachable gradient rule, each of the four colour rules and ends
    whose -1 neighbour comes from another block, >= 16 times each.  Measured: rules >= 236 per axis,
    colour rules 254 / 107 / 103 / 52, 146 ends."""
    _, _, rgb, tris, _, colours, stats = A.random_case()
    print(stats)
    assert abs(float((rgb >> 24 == 0).mean()) - 0.3) < 0.02
    assert (stats["rules"][:, :3] >= 16).all(), stats["rules"]
    assert (stats["rules"][:, 3] == 0).all()                         # unreachable for an end of a valid cube
    assert min(stats["colour_rules"]) >= 16, stats["colour_rules"]
    assert stats["down_block"] >= 16
    assert colours.shape == (len(tris), 3, 4)
    assert set(np.unique(colours[..., 3])) == {0, 255}
    assert not colours[colours[..., 3] == 0].any()


def test_slab_zero_normals():
    """One block, sdf = (-3, -1, 1, -5, ...) along x: the surface is crossed between x = 1 and 2 and
    between x = 2 and 3.  At x = 1 and x = 2 the central x gradients are +4 and -4 and t = 1/2, so
    exactly the vertices of the first crossing have the normal (0, 0, 0) (225 of the 450 crossed edges);
    all others are (-1, 0, 0) or (+1, 0, 0)."""
    _, _, _, tris, normals, _, stats = A.slab_case()
    assert len(tris) == 784
    x = tris[..., 0].astype(np.float64) / M.VOXEL_SIZE
    first = (x > 1) & (x < 2)
    assert np.all(first | ((x > 2) & (x < 3)))
    zero = (normals == 0).all(-1)
    assert np.array_equal(zero, first)
    assert stats["edges"] == 450 and stats["zero"] == 225
    rest = normals[~zero]
    assert np.all(np.abs(rest[:, 0]) == 1) and not rest[:, 1:].any()
    assert np.all(rest[:, 0] == -1)                                   # sdf falls from 1 to -5 there: the gradient points to -x


def _word(r, g, b, w):
    return np.uint32(r | g << 8 | b << 16 | w << 24)


def test_colour_byte_rounding():
    """Channel differences of +-255, t at 0 and 1, f exactly on k + 0.5 (rounds up), and the rules for
    one or no coloured end."""
    t = np.float32
    both = lambda tt, a, b: A.vertex_colour(t(tt), _word(*a), _word(*b), np.bool_(True), np.bool_(True)).tolist()
    assert both(0.0, (0, 255, 7, 1), (255, 0, 7, 1)) == [0, 255, 7, 255]
    assert both(1.0, (0, 255, 7, 1), (255, 0, 7, 1)) == [255, 0, 7, 255]
    assert both(0.5, (0, 255, 10, 9), (255, 0, 13, 1)) == [128, 128, 12, 255]     # 127.5 -> 128, 11.5 -> 12
    assert both(0.5, (0, 1, 254, 1), (1, 0, 255, 1)) == [1, 1, 255, 255]          # 0.5 -> 1, 254.5 -> 255
    assert both(0.25, (0, 255, 2, 1), (255, 0, 0, 1)) == [64, 191, 2, 255]        # 63.75 -> 64, 191.25 -> 191, 1.5 -> 2
    one = A.vertex_colour(t(0.3), _word(1, 2, 3, 0), _word(4, 5, 6, 9), np.bool_(False), np.bool_(True)).tolist()
    assert one == [4, 5, 6, 255]
    one = A.vertex_colour(t(0.3), _word(1, 2, 3, 2), _word(4, 5, 6, 0), np.bool_(True), np.bool_(False)).tolist()
    assert one == [1, 2, 3, 255]
    assert A.vertex_colour(t(0.3), _word(1, 2, 3, 0), _word(4, 5, 6, 0), np.bool_(False), np.bool_(False)).tolist() == [0, 0, 0, 0]


def test_ply_attr_round_trip(tmp_path):
    """io.write_ply with attributes -> io.read_ply_attr: the welded records expand back to the input bit
    for bit, there are as many as distinct (position, normal, colour) records, and the attribute-free
    call writes the file it always wrote."""
    from topfusion_amd import io
    _, _, _, tris, normals, colours, _ = A.random_case()
    for nr, co in ((normals, colours), (normals, None), (None, colours)):
        path = tmp_path / "attr.ply"
        io.write_ply(path, tris, normals=nr, colours=co)
        verts, faces, vn, vc = io.read_ply_attr(path)
        assert verts[faces].tobytes() == tris.tobytes()
        assert (vn is None) == (nr is None) and (vc is None) == (co is None)
        if nr is not None:
            assert vn[faces].tobytes() == nr.tobytes()
        if co is not None:
            assert vc[faces].tobytes() == co.tobytes()
        records, _ = A.weld(tris, nr, co)
        assert len(verts) == len(records)
    # two vertices at one position with different attributes stay apart
    t2 = np.zeros((2, 3, 3), np.float32)
    n2 = np.zeros((2, 3, 3), np.float32)
    n2[1, :, 2] = 1
    io.write_ply(tmp_path / "two.ply", t2, normals=n2)
    verts, faces, vn, _ = io.read_ply_attr(tmp_path / "two.ply")
    assert len(verts) == 2 and vn[faces].tobytes() == n2.tobytes()
    plain, old = tmp_path / "plain.ply", tmp_path / "old.ply"
    io.write_ply(plain, tris)
    from topfusion_amd import _lib as L
    t = np.ascontiguousarray(tris)
    L.check(L.load().tf_mesh_write_ply(str(old).encode(), t.ctypes.data_as(ctypes.c_void_p), len(t)), "tf_mesh_write_ply")
    assert plain.read_bytes() == old.read_bytes()
    L.check(L.load().tf_mesh_write_ply_attr(str(plain).encode(), t.ctypes.data_as(ctypes.c_void_p), None, None, len(t)),
            "tf_mesh_write_ply_attr")
    assert plain.read_bytes() == old.read_bytes()
    verts, faces, vn, vc = io.read_ply_attr(old)
    assert vn is None and vc is None and verts[faces].tobytes() == tris.tobytes()
    v0, f0 = io.read_ply(old)
    assert v0.tobytes() == verts.tobytes() and f0.tobytes() == faces.tobytes()
    io.write_ply(tmp_path / "empty.ply", np.zeros((0, 3, 3), np.float32), normals=np.zeros((0, 3, 3), np.float32))
    verts, faces, vn, vc = io.read_ply_attr(tmp_path / "empty.ply")
    assert len(verts) == 0 and len(faces) == 0 and vn.shape == (0, 3) and vc is None


def _ply_bytes(records, faces, normals, colours):
    """The file of DESIGN.md §Mesh extraction (PLY), built here: the header text, the vertex records (3 | 6 | 7
    little-endian dwords each), then per face the byte 3 and three little-endian int32."""
    head = "ply\nformat binary_little_endian 1.0\ncomment topfusion mesh\n" + f"element vertex {len(records)}\n" + \
           "property float x\nproperty float y\nproperty float z\n" + \
           ("property float nx\nproperty float ny\nproperty float nz\n" if normals else "") + \
           ("property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n" if colours else "") + \
           f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n"
    rec = np.zeros(len(faces), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    assert rec.dtype.itemsize == 13
    rec["n"], rec["i"] = 3, np.asarray(faces).reshape(-1, 3)
    return head.encode("ascii") + np.ascontiguousarray(records, "<u4").tobytes() + rec.tobytes()


def _first_appearance(records, faces):
    """A.weld's (sorted) records and faces renumbered in the order in which the triangles' vertices first
    name each record: the order the welding writers keep."""
    flat = np.asarray(faces).reshape(-1)
    first = np.full(len(records), -1, np.int64)
    first[flat[::-1]] = np.arange(len(flat))[::-1]
    assert (first >= 0).all()
    order = np.argsort(first)
    rank = np.empty(len(records), np.int64)
    rank[order] = np.arange(len(records))
    return records[order], rank[flat].reshape(-1, 3)


def test_ply_bytes(tmp_path):
    """Every byte of the three writers' files against _ply_bytes, independently of the writers' hash: the
    random attributed case (all column combinations; for the indexed writer its welded records as the vertex
    table), two vertices at one position with different normals, and the empty mesh with a declared normal
    column."""
    from topfusion_amd import io
    _, _, _, tris, normals, colours, _ = A.random_case()
    t2 = np.zeros((2, 3, 3), np.float32)
    n2 = np.zeros((2, 3, 3), np.float32)
    n2[1, :, 2] = 1
    e3 = np.zeros((0, 3, 3), np.float32)
    cases = [(tris, nr, co) for nr in (None, normals) for co in (None, colours)] + [(t2, n2, None), (e3, e3, None)]
    path = tmp_path / "bytes.ply"
    for t, nr, co in cases:
        records, faces = _first_appearance(*A.weld(t, nr, co)) if len(t) else (np.zeros((0, 6), np.uint32), np.zeros((0, 3), np.int64))
        want = _ply_bytes(records, faces, nr is not None, co is not None)
        io.write_ply(path, t, normals=nr, colours=co)
        assert path.read_bytes() == want, (len(t), nr is not None, co is not None)
        # the same table through the indexed writer: nothing welded, nothing reordered
        v = records[:, :3].view(np.float32)
        vn = None if nr is None else records[:, 3:6].view(np.float32)
        vc = None if co is None else np.ascontiguousarray(records[:, -1:]).view(np.uint8)
        io.write_ply_indexed(path, v, faces.astype(np.uint32), normals=vn, colours=vc)
        assert path.read_bytes() == want, (len(t), nr is not None, co is not None)
    assert len(_first_appearance(*A.weld(t2, n2))[0]) == 2
    # a table with repeated rows and a reversed order stays as given
    records, faces = A.weld(tris, normals, colours)
    rep = np.concatenate([records[::-1], records[:5]])
    f = (len(records) - 1 - faces).astype(np.uint32)
    io.write_ply_indexed(path, rep[:, :3].view(np.float32), f, normals=rep[:, 3:6].view(np.float32),
                         colours=np.ascontiguousarray(rep[:, -1:]).view(np.uint8))
    assert path.read_bytes() == _ply_bytes(rep, f, True, True)


def test_ply_writers_under_asan_ubsan(tmp_path):
    """tf_mesh_ply.cpp built for the CPU with -fsanitize=address,undefined and driven by tests/mesh_ply_main.cpp
    in one process: the three writers on 300 random triangles with duplicated vertices (every column
    combination, the files expanding back bit for bit), 0.0f beside -0.0f, empty meshes with and without
    attribute columns, an index equal to the vertex count and the null / negative arguments (refused) -- with
    no sanitizer report."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mesh_ply_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "mesh_ply_main.cpp"),
                        os.path.join(ROOT, "topfusion_amd", "csrc", "tf_mesh_ply.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = tmp_path / "files"
    out.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


_HOST_SRC = r"""
#include "tf_mesh.h"
extern "C" int h_grad(int sm, int s0, int sp, int um, int up) { return tfm_grad_axis(sm, s0, sp, um != 0, up != 0); }
extern "C" void h_normal(int n, const int* sp, const int* sq, const int* gp, const int* gq, float* out)
{
    for (int i = 0; i < n; ++i) tfm_normal(tfm_edge_t(sp[i], sq[i]), gp + 3 * i, gq + 3 * i, out + 3 * i);
}
extern "C" void h_colour(int n, const int* sp, const int* sq, const unsigned* wp, const unsigned* wq, unsigned* out)
{
    for (int i = 0; i < n; ++i) out[i] = tfm_colour(tfm_edge_t(sp[i], sq[i]), wp[i], wq[i]);
}
"""


def test_shared_functions_as_host_cxx(tmp_path):
    """tf_mesh.h's per-vertex functions (the ones the kernel calls) compiled as plain host C++ without
    contraction: gradient rule, normal and colour equal the numpy restatement bit for bit on random
    edges, including the extreme gradients (+-131070) and sdf pairs with t = 0 and t = 1."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, lib = tmp_path / "host.cpp", tmp_path / "libhost.so"
    src.write_text(_HOST_SRC)
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "topfusion_amd", "csrc"),
                    str(src), "-o", str(lib)], check=True)
    hl = ctypes.CDLL(str(lib))
    for sm, s0, sp in ((-32768, 5, 32767), (32767, -7, -32768), (3, 4, 9)):
        assert hl.h_grad(sm, s0, sp, 1, 1) == sp - sm
        assert hl.h_grad(sm, s0, sp, 0, 1) == 2 * (sp - s0)
        assert hl.h_grad(sm, s0, sp, 1, 0) == 2 * (s0 - sm)
        assert hl.h_grad(sm, s0, sp, 0, 0) == 0
    rng = np.random.default_rng(9)
    n = 20000
    neg = rng.integers(-32768, 0, n).astype(np.int32)
    pos = rng.integers(0, 32768, n).astype(np.int32)
    pos[:50] = 0                                                      # t = 1 (lower end inside) or t = 0
    swap = rng.random(n) < 0.5
    sp, sq = np.where(swap, pos, neg).astype(np.int32), np.where(swap, neg, pos).astype(np.int32)
    gp = rng.integers(-131070, 131071, (n, 3)).astype(np.int32)
    gq = rng.integers(-131070, 131071, (n, 3)).astype(np.int32)
    gp[:8], gq[:8] = 131070, -131070
    gp[8:16], gq[8:16] = 0, 0
    gp[16:24] = -gq[16:24]
    t = (sp.astype(np.float32) / (sp - sq).astype(np.float32)).astype(np.float32)
    assert t.min() == 0 and t.max() == 1
    ip = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.empty((n, 3), np.float32)
    hl.h_normal(n, ip(sp), ip(sq), ip(gp), ip(gq), ip(out))
    want = A.vertex_normal(t, gp, gq)
    assert out.tobytes() == want.tobytes()
    assert (want[8:16] == 0).all()
    wp = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    wq = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    wp[rng.random(n) < 0.3] &= np.uint32(0xffffff)
    wq[rng.random(n) < 0.3] &= np.uint32(0xffffff)
    wp[:50], wq[:50] = 0x01ff00ff, 0x0100ff00                         # +-255 at t = 0 | 1
    got = np.empty(n, np.uint32)
    hl.h_colour(n, ip(sp), ip(sq), ip(wp), ip(wq), ip(got))
    want = A.vertex_colour(t, wp, wq, wp >> 24 > 0, wq >> 24 > 0)
    assert got.view(np.uint8).reshape(n, 4).tobytes() == want.tobytes()
