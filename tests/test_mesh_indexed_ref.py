"""The indexed mesh extraction's specification, checked without a GPU: the numpy restatement
(tests/mesh_indexed_ref.py) against mesh_ref's triangles and against what a closed surface must satisfy, the
coverage of the dense random scene, tf_mesh.h's per-edge helpers compiled as host C++, and the indexed PLY
writer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import mesh_indexed_ref as X
import mesh_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sphere_is_a_closed_oriented_surface():
    c = X.sphere_case()
    v, f = c["vertices"], c["indices"].astype(np.int64)
    assert v[f].tobytes() == M.sphere_case()[2].tobytes()                 # vertices[indices] == M.extract, bit for bit
    assert np.array_equal(np.unique(f), np.arange(len(v)))                # every vertex referenced, none beyond
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    # every directed edge once, and its reverse once: watertight, consistently oriented
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = de[:, 0] * len(v) + de[:, 1]
    assert len(np.unique(key)) == len(key)
    assert np.array_equal(np.sort(key), np.sort(de[:, 1] * len(v) + de[:, 0]))
    assert len(v) - len(f) // 2 == 2 and len(f) % 2 == 0                  # V - F / 2 = 2: a sphere
    assert (len(f), len(v)) == (9684, 4844)
    assert len(v) == len(M.weld(M.sphere_case()[2])[0])                   # here no two edges share a position


def test_dense_scene_coverage():
    """The dense random scene asserts its own coverage when it is built (at least 5000 triangles, owners at all
    seven block offsets an edge's lower end can have, owners in excess entries, distinct edges with
    bit-equal positions); here what follows from it."""
    c = X.dense_case()
    v, f, st = c["vertices"], c["indices"].astype(np.int64), c["stats"]
    assert st["nt"] >= 5000 and len(f) == st["nt"] and len(v) == st["nv"]
    assert len(st["owner_dirs"]) == 7 and (1, 1, 1) not in st["owner_dirs"] and st["excess_owners"] > 0
    welded = len(M.weld(c["tris"])[0])
    assert len(v) > welded, (len(v), welded)                              # a weld on positions would merge edges
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    assert v[f].tobytes() == c["tris"].tobytes()
    assert c["normals"][f].tobytes() == c["tri_normals"].tobytes()
    assert c["colours"][f].tobytes() == c["tri_colours"].tobytes()
    # the order: owner entry, then voxel, then direction code -- the vertex table's keys ascend strictly,
    # re-derived here from the first triangle vertex that uses each vertex
    ent, P, D = X.triangle_edges(c["hash"], c["vba"], c["cfg"]["n_buckets"])
    first = np.full(len(v), -1, np.int64)
    flat = f.reshape(-1)
    first[flat[::-1]] = np.arange(len(flat))[::-1]
    p, d = P.reshape(-1, 3)[first], D.reshape(-1, 3)[first]
    owner = np.array([X.find_live(c["hash"], c["cfg"]["n_buckets"], b)[0] for b in p // 8])
    key = np.stack([owner, (p % 8) @ np.array([1, 8, 64]), d @ np.array([1, 2, 4])], -1)
    assert all(tuple(key[i]) < tuple(key[i + 1]) for i in range(len(key) - 1))


_HOST_SRC = r"""
#include "tf_mesh.h"
struct Marks { unsigned* out; int n; void operator()(const TfmEdgeRef& r) { out[2 * n] = r.owner; out[2 * n + 1] = r.bit; ++n; } };
struct Tris { unsigned* out; int n; void operator()(const unsigned* lo, const unsigned* hi)
    { for (int v = 0; v < 3; ++v) { out[6 * n + 2 * v] = lo[v]; out[6 * n + 2 * v + 1] = hi[v]; } ++n; } };
extern "C" {
void h_edge_ref(int px, int py, int pz, unsigned dc, unsigned* out) { const TfmEdgeRef r = tfm_edge_ref(px, py, pz, dc); out[0] = r.owner; out[1] = r.bit; }
unsigned h_edge_rank(unsigned word, unsigned prefix, unsigned bit) { return tfm_edge_rank(word, prefix, bit); }
// n cubes: sdf[8], valid, corner 0 at (x, y, z); marks (19 pairs each at most), triangle edges (12 triangles each at most)
void h_cubes(int n, const int* sdf, const int* valid, const int* xyz, unsigned* marks, int* n_marks, unsigned* tris, int* n_tris)
{
    for (int i = 0; i < n; ++i) {
        TfmCube q;
        for (int c = 0; c < 8; ++c) q.sdf[c] = sdf[8 * i + c];
        q.valid = valid[i] != 0;
        Marks m = { marks + 38 * i, 0 };
        tfm_cube_mark(q, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], m);
        n_marks[i] = m.n;
        Tris t = { tris + 72 * i, 0 };
        n_tris[i] = tfm_cube_emit_edges(q, t);
    }
}
void h_edge_vertex(int n, const unsigned* dc, const int* sp, const int* sq, const int* p, float vs, float* out)
{
    for (int i = 0; i < n; ++i) tfm_edge_vertex(dc[i], sp[i], sq[i], p[3 * i], p[3 * i + 1], p[3 * i + 2], vs, out + 3 * i);
}
void h_vertex(int n, const unsigned* lo, const unsigned* hi, const int* sp, const int* sq, const int* g, float vs, float* out)
{
    for (int i = 0; i < n; ++i) tfm_vertex(lo[i], hi[i], sp[i], sq[i], g[3 * i], g[3 * i + 1], g[3 * i + 2], vs, out + 3 * i);
}
}
"""


def test_edge_helpers_as_host_cxx(tmp_path):
    """tf_mesh.h's per-edge functions (the ones the indexed kernels call) compiled as plain host C++: the
    edge's owner and bit, its rank, a cube's marked edges and its triangles' edges equal the numpy rules --
    the marked set is exactly the set of edges the cube's triangles touch -- and the vertex computed from
    the edge's lower end equals, bit for bit, the one every cube sharing the edge computes."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, lib = tmp_path / "host.cpp", tmp_path / "libhost.so"
    src.write_text(_HOST_SRC)
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "topfusion_amd", "csrc"),
                    str(src), "-o", str(lib)], check=True)
    hl = ctypes.CDLL(str(lib))
    hl.h_edge_rank.restype = ctypes.c_uint
    ip = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # owner and bit of every edge of a tile
    out = np.zeros(2, np.uint32)
    for px in range(9):
        for py in range(9):
            for pz in range(9):
                for dc in range(1, 8):
                    hl.h_edge_ref(px, py, pz, dc, ip(out))
                    lp = px % 8 + 8 * (py % 8) + 64 * (pz % 8)
                    assert tuple(out) == (px // 8 + 2 * (py // 8) + 4 * (pz // 8), lp * 7 + dc - 1)
    assert out[1] < 112 * 32
    rng = np.random.default_rng(5)
    for word, prefix, bit in [(0xffffffff, 7, 31), (0xffffffff, 0, 32), (0x80000001, 3, 63), (1, 5, 0)] + \
            [(int(rng.integers(0, 1 << 32)), int(rng.integers(0, 3584)), int(rng.integers(0, 3584))) for _ in range(200)]:
        want = prefix + bin(word & ((1 << (bit % 32)) - 1)).count("1")
        assert hl.h_edge_rank(ctypes.c_uint(word), ctypes.c_uint(prefix), ctypes.c_uint(bit)) == want
    # cubes: random sdf with zeros frequent, some invalid, all 256 inside masks
    n = 4096
    sdf = rng.integers(-32768, 32768, (n, 8)).astype(np.int32)
    sdf[rng.random((n, 8)) < 0.1] = 0
    sdf[:256] = np.where((np.arange(256)[:, None] >> np.arange(8)) & 1, -5, 7)
    valid = (rng.random(n) < 0.9).astype(np.int32)
    valid[:256] = 1
    xyz = rng.integers(0, 8, (n, 3)).astype(np.int32)
    xyz[:8] = 7
    marks, n_marks = np.zeros((n, 19, 2), np.uint32), np.zeros(n, np.int32)
    tris, n_tris = np.zeros((n, 12, 3, 2), np.uint32), np.zeros(n, np.int32)
    hl.h_cubes(n, ip(sdf), ip(valid), ip(xyz), ip(marks), ip(n_marks), ip(tris), ip(n_tris))
    corners, ntri, edges = M._tables()
    cid = lambda c: int(c[0] + 2 * c[1] + 4 * c[2])                       # cube corner id of an offset
    total = 0
    for i in range(n):
        want = []                                                         # the cube's triangles by the rule: (lo, hi) corner ids
        if valid[i]:
            for k in range(6):
                m = sum(int(sdf[i, cid(corners[k][j])] < 0) << j for j in range(4))
                for t in range(ntri[k, m]):
                    want.append([(cid(corners[k][lo]), cid(corners[k][hi])) for lo, hi in edges[k, m, t]])
        assert n_tris[i] == len(want)
        assert tris[i, :len(want)].tolist() == [[list(e) for e in t] for t in want]
        touched = set()
        for t in want:
            for lo, hi in t:
                p = xyz[i] + np.array([lo & 1, lo >> 1 & 1, lo >> 2])
                lp = int(p[0] % 8 + 8 * (p[1] % 8) + 64 * (p[2] % 8))
                touched.add((int(p[0] // 8 + 2 * (p[1] // 8) + 4 * (p[2] // 8)), lp * 7 + (hi & ~lo) - 1))
        got = [tuple(int(v) for v in e) for e in marks[i, :n_marks[i]]]
        assert len(set(got)) == len(got) and set(got) == touched, (i, got, touched)
        total += len(got)
    assert total > 10000
    # the vertex from the edge's lower end == tfm_vertex from any cube that holds the edge
    m = 20000
    neg, pos = rng.integers(-32768, 0, m).astype(np.int32), rng.integers(0, 32768, m).astype(np.int32)
    pos[:50] = 0
    swap = rng.random(m) < 0.5
    sp, sq = np.where(swap, pos, neg).astype(np.int32), np.where(swap, neg, pos).astype(np.int32)
    dc = rng.integers(1, 8, m).astype(np.uint32)
    lo = (rng.integers(0, 8, m).astype(np.uint32) & ~dc).astype(np.uint32)
    hi = (lo | dc).astype(np.uint32)
    p = rng.integers(-262144, 262144, (m, 3)).astype(np.int32)
    g = (p - np.stack([lo & 1, lo >> 1 & 1, lo >> 2], -1).astype(np.int32)).astype(np.int32)     # that cube's corner 0
    a, b = np.empty((m, 3), np.float32), np.empty((m, 3), np.float32)
    vs = ctypes.c_float(M.VOXEL_SIZE)
    V = ctypes.c_void_p
    hl.h_edge_vertex.argtypes = [ctypes.c_int, V, V, V, V, ctypes.c_float, V]
    hl.h_vertex.argtypes = [ctypes.c_int, V, V, V, V, V, ctypes.c_float, V]
    hl.h_edge_vertex(m, ip(dc), ip(sp), ip(sq), ip(p), vs, ip(a))
    hl.h_vertex(m, ip(lo), ip(hi), ip(sp), ip(sq), ip(g), vs, ip(b))
    assert a.tobytes() == b.tobytes()
    t = (sp.astype(np.float32) / (sp - sq).astype(np.float32)).astype(np.float32)
    d = np.stack([dc & 1, dc >> 1 & 1, dc >> 2], -1)
    pf = p.astype(np.float32)
    want = np.where(d == 1, ((pf + t[:, None]).astype(np.float32) * np.float32(M.VOXEL_SIZE)).astype(np.float32),
                    (pf * np.float32(M.VOXEL_SIZE)).astype(np.float32))
    assert a.tobytes() == want.astype(np.float32).tobytes()


def test_ply_indexed_round_trip(tmp_path):
    """write_ply_indexed keeps the vertex table as it is -- order, and vertices equal in position -- with and
    without attributes; read_ply and read_ply_attr read the files."""
    from topfusion_amd import io
    c = X.dense_case()
    v, f, nr, co = c["vertices"], c["indices"], c["normals"], c["colours"]
    assert len(np.unique(v.view(np.uint32), axis=0)) < len(v)            # duplicates by position are present
    path = tmp_path / "full.ply"
    io.write_ply_indexed(path, v, f, normals=nr, colours=co)
    gv, gf, gn, gc = io.read_ply_attr(path)
    assert gv.tobytes() == v.tobytes() and gn.tobytes() == nr.tobytes() and gc.tobytes() == co.tobytes()
    assert gf.dtype == np.int32 and np.array_equal(gf, f.astype(np.int32))
    path = tmp_path / "plain.ply"
    io.write_ply_indexed(path, v, f)
    pv, pf = io.read_ply(path)
    assert pv.tobytes() == v.tobytes() and np.array_equal(pf, f.astype(np.int32))
    av, af, an, ac = io.read_ply_attr(path)
    assert av.tobytes() == v.tobytes() and np.array_equal(af, pf) and an is None and ac is None
    path = tmp_path / "colours.ply"
    io.write_ply_indexed(path, v, f, colours=co)
    cv, cf, cn, cc = io.read_ply_attr(path)
    assert cv.tobytes() == v.tobytes() and cn is None and cc.tobytes() == co.tobytes()
    # the welding writer on the same soup has fewer vertices: it merges edges that share a position
    io.write_ply(tmp_path / "welded.ply", c["tris"])
    assert len(io.read_ply(tmp_path / "welded.ply")[0]) < len(v)
    path = tmp_path / "empty.ply"
    io.write_ply_indexed(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), normals=np.zeros((0, 3), np.float32))
    ev, ef, en, ec = io.read_ply_attr(path)
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and en.shape == (0, 3) and ec is None
    import pytest
    from topfusion_amd import _lib as L
    with pytest.raises(L.TfError):                                        # an index past the table
        io.write_ply_indexed(tmp_path / "bad.ply", v[:10], f)
