"""CPU conditions of the scene query tests' inputs (tests/scene_query_cases.py) and of the query surface that needs
no GPU: the goldens give one expected value per point, the guard's points fall on both sides of it, the made scenes
hold what they are meant to, every run of 64 points mixes its classes, and the Python and C++ layers declare the calls."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pin_scenes as P
import scene_query_cases as Q
from parity_util import assert_bit_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", P.SCENES)
def test_goldens_give_one_value_per_point(name):
    """The reference's reads do not depend on the IndexCache they are given: the fresh-cache and carried-cache columns
    agree in every value column (only vm differs), the two interpolated reads agree, and no normal is NaN -- so a
    per-point query has one expected record."""
    g = P.read_pin(P.golden_path(name, "sdf_read"))
    assert_bit_exact(f"{name} scene CRC32", g["crc"], P.scene(name)["crc"])
    n = len(P.sdf_points(name))
    for k in ("uninterp", "interp", "conf_sdf", "conf"):
        two = g[k].reshape(n, 2)
        assert_bit_exact(f"{name} {k}: fresh against carried cache", two[:, 0], two[:, 1])
    assert_bit_exact(f"{name} interp against conf_sdf", g["interp"], g["conf_sdf"])
    vm = g["vm"].reshape(n, 2)
    assert (vm[:, 0] != vm[:, 1]).any() and set(np.unique(vm[:, 1][vm[:, 0] != vm[:, 1]])) == {1}
    assert not np.isnan(g["normal"]).any()
    e = Q.golden_expected(name)
    assert e["entry"].min() == -1 and (e["entry"] >= P.N_BUCKETS).sum() >= Q.MIN_PER_CLASS      # missing, and chained in excess entries
    assert Q.in_range(P.sdf_points(name)).all()


def test_expected_is_the_golden_where_both_exist(oracle_mod):
    """scene_query_cases.expected over the oracle reproduces the reference's record at the pin points (one scene)."""
    from test_oracle_stage_pin import oracle_params
    name = "random"
    s = P.scene(name)
    o = oracle_mod.Oracle(oracle_mod.default_params(**oracle_params()))
    o.upload_hash(s["hash"])
    o.upload_vba(s["vba"], s["vba_rgb"])
    got, want = Q.expected(o, P.sdf_points(name)), Q.golden_expected(name)
    for k in Q.OUTS:
        assert_bit_exact(f"{name} {k}", got[k], want[k])


def test_sizes_cover_the_wave_and_workgroup_edges():
    assert Q.SIZES == (0, 1, 63, 64, 65, 255, 256, 257)


def test_metres_round_trip_is_not_the_identity():
    """The metre points are not all mapped back onto the voxel points they came from (the conversion's rounding is
    part of what is tested), and all stay in range."""
    for name in P.SCENES:
        v = Q.metres_to_voxels(Q.metre_points(name), P.VOXEL_SIZE)
        assert Q.in_range(v).all()
        assert (v != P.sdf_points(name)).any(1).sum() >= Q.MIN_PER_CLASS
        assert (np.floor(v) != np.floor(P.sdf_points(name))).any(1).sum() >= 1       # some land in another voxel


def test_guard_points():
    pts, ok = Q.guard_points()
    assert len(pts) == 4 * 3 * len(Q.GUARD_VALUES)
    special = pts[::4]
    want_ok = np.tile(np.array([0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0], bool), 3)
    assert np.array_equal(ok[::4], want_ok)
    assert ok.reshape(-1, 4)[:, 1:].all()
    assert float(Q._BEYOND) == 262136.015625 and float(Q._BEYOND32) == 262136.03125 and Q._BEYOND > Q.LIMIT
    for ax in range(3):
        col = special[ax * len(Q.GUARD_VALUES):(ax + 1) * len(Q.GUARD_VALUES), ax]
        assert np.array_equal(col.view(np.uint32), Q.GUARD_VALUES.view(np.uint32))
    for r in range(0, len(pts), 64):                       # every wave holds points of both kinds
        assert ok[r:r + 64].any() and not ok[r:r + 64].all()


def test_far_scene_and_points():
    s = Q.far_scene()
    b, h = s["blocks"], s["hash"]
    ing = Q._in_grid(b)
    assert ing.sum() >= 64 and (~ing).sum() >= 64
    assert (np.abs(b[~ing]) >= 128).any(1).all()
    assert s["swapped"][ing].sum() >= 4 and s["swapped"][~ing].sum() >= 4
    assert (h["ptr"] == -1).sum() == s["swapped"].sum()
    # the chained pair: one bucket, the second position in an excess entry, both outside the grid and resident
    pair = s["pair"]
    hi = synth_hash(pair)
    assert hi[0] == hi[1] and not Q._in_grid(pair).any()
    e = s["entry"][-2:]
    assert e.min() < P.N_BUCKETS <= e.max() and (h["ptr"][e] >= 0).all()
    pts, cls = Q.far_points()
    assert Q.in_range(pts).all()
    true = Q.far_point_classes(pts)
    for c, tag in enumerate(Q.FAR_CLASSES):
        assert (true == c).sum() >= Q.MIN_PER_CLASS, (tag, (true == c).sum())
    for r in range(0, len(pts), 64):
        assert set(true[r:r + 64]) == {0, 1, 2, 3}, (r, set(true[r:r + 64]))
    # points whose nearest voxel lies in the chained pair's excess entry
    r = np.where(pts < 0, pts - np.float32(0.5), pts + np.float32(0.5)).astype(np.int64) >> 3
    chained = pair[list(s["entry"][-2:]).index(e.max())]
    assert (r == chained).all(1).sum() >= 4
    # interpolation corners across the grid's edge at x = 127 | 128 are not asked for here: the edge blocks serve
    # the pool of resident blocks on both sides
    assert {(127, 0, 12), (128, 0, 12)} <= {tuple(p) for p in b.tolist()}


def synth_hash(pos):
    from topfusion_amd import synth
    pos = np.asarray(pos, np.int64)
    return synth.hash_index(pos[:, 0], pos[:, 1], pos[:, 2], P.N_BUCKETS)


def test_whole_points():
    import view_whole_ref as VW
    pts, cls = Q.whole_points()
    assert Q.in_range(pts).all()
    own, nxt = Q.whole_point_classes(pts)
    # view_whole_ref's classes: 0 active, 1 stored, 2 pending, 3 stale, 4 lost
    resident = np.isin(own, (0, 3))
    assert (resident & (cls == 0)).sum() >= Q.MIN_PER_CLASS
    assert ((own == 1) & (cls == 1)).sum() >= Q.MIN_PER_CLASS
    assert ((own == 2) & (cls == 2)).sum() >= Q.MIN_PER_CLASS
    face = np.array([resident[j] and 1 in nxt[j] for j in range(len(pts))])
    assert (face & (cls == 3)).sum() >= Q.MIN_PER_CLASS
    for r in range(0, len(pts), 64):
        assert resident[r:r + 64].any() and (own[r:r + 64] == 1).any() and (own[r:r + 64] == 2).any() and face[r:r + 64].any()
    t = VW.tiered_scene()
    assert ((t["hash"]["ptr"] == -1) & (t["flags"] == 1)).sum() >= Q.MIN_PER_CLASS


def test_whole_expected_differs_from_resident(oracle_mod):
    """The whole reading's expected record is not the resident one at the stored, pending and face points."""
    import view_ref as V
    import view_whole_ref as VW
    t = VW.tiered_scene()
    pts, cls = Q.whole_points()
    ow = Q.whole_oracle(oracle_mod, t, V.TABLES, V.W0, V.H0)
    orr = V.oracle_for(oracle_mod, V.W0, V.H0)
    orr.upload_hash(t["hash"])
    orr.upload_vba(t["vba"], None)
    w, r = Q.expected(ow, pts, colour=False), Q.expected(orr, pts, colour=False)
    for c in (1, 2, 3):
        m = cls == c
        assert (w["sdf"][m] != r["sdf"][m]).sum() >= Q.MIN_PER_CLASS // 2, Q.WHOLE_CLASSES[c]
    m = cls == 1                                   # (the nearest voxel of a point near a face may lie in a neighbour)
    assert ((w["entry"][m] >= 0) & (r["entry"][m] == -1)).sum() >= Q.MIN_PER_CLASS


@pytest.mark.parametrize("kind", ["oblique", "axis"])
def test_slice_planes(kind):
    for cols, rows in Q.SLICE_SIZES:
        o, u, v = Q.slice_plane(kind, cols, rows)
        pts = Q.slice_points(o, u, v, cols, rows)
        assert pts.shape == (cols * rows, 3) and pts.dtype == np.float32 and Q.in_range(pts).all()
        d = np.linalg.norm(pts.astype(np.float64) - Q.SPHERE_C, axis=1)
        assert d.min() < 56.3 < d.max()                          # the plane cuts the shell
        assert_bit_exact("pixel (0, 0)", pts[0], o)
        x, y = cols - 1, rows - 1
        last = (o + np.float32(x) * u).astype(np.float32) + (np.float32(y) * v).astype(np.float32)
        assert_bit_exact("the last pixel", pts[-1], last.astype(np.float32))
    assert Q.SLICE_SIZES == ((4, 4), (37, 29), (164, 124))


# ---- the surface above the C-ABI --------------------------------------------------------------------------------
def test_ctypes_mirror_declares_the_calls():
    from topfusion_amd import TopFu, _lib
    L = _lib.load()
    for name in ("tf_scene_query", "tf_scene_slice"):
        assert name in _lib.header_functions()
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
    assert len(L.tf_scene_query.argtypes) == 6 and len(L.tf_scene_slice.argtypes) == 9
    assert (_lib.TF_QUERY_VOXELS, _lib.TF_QUERY_METRES) == (0, 1)
    assert [f for f, _ in _lib.TfQueryOut._fields_] == list(Q.OUTS)
    assert ctypes.sizeof(_lib.TfQueryOut) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert callable(TopFu.query) and callable(TopFu.slice)
    # refused before any device is looked for
    out = _lib.TfQueryOut()
    assert L.tf_scene_query(None, None, 0, 0, 0, ctypes.byref(out)) == _lib.TF_INVALID_ARG
    assert L.tf_scene_slice(None, None, None, None, 4, 4, 0, 0, ctypes.byref(out)) == _lib.TF_INVALID_ARG


def test_query_out_layout_matches_header(tmp_path):
    from topfusion_amd import _lib
    fields = [f for f, _ in _lib.TfQueryOut._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tfusion_hip.h"\nint main(void){\n'
    prog += 'printf("%zu\\n", sizeof(tf_query_out));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(tf_query_out, {f}));\n'
    prog += 'printf("%d %d\\n", (int)TF_QUERY_VOXELS, (int)TF_QUERY_METRES);\nreturn 0;}\n'
    c, exe = tmp_path / "l.c", tmp_path / "l"
    c.write_text(prog)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_lib.TfQueryOut)
    for f, off in zip(fields, out[1:]):
        assert getattr(_lib.TfQueryOut, f).offset == int(off), f
    assert out[-2:] == ["0", "1"]


CPP_PROGRAM = r"""
#include <tfusion/topfu.hpp>
#include <tfusion/engines.hpp>
using namespace tfusion;
// compile-only: Scene::query / Scene::slice and TopFu::query / TopFu::slice exist with the documented signatures
void use(Scene<Voxel_s, VoxelBlockHash>& scene, TopFu& fu, const float* dev_points, float* dev_sdf, float* dev_normal)
{
    tf_query_out out = {};
    out.sdf = dev_sdf;
    out.normal = dev_normal;
    const float o[3] = { 0.f, 0.f, 0.f }, u[3] = { 0.01f, 0.f, 0.f }, v[3] = { 0.f, 0.01f, 0.f };
    scene.query(dev_points, 100, TF_QUERY_METRES, true, out);
    scene.slice(o, u, v, 64, 48, TF_QUERY_VOXELS, false, out);
    fu.query(dev_points, 100, TF_QUERY_VOXELS, false, out);
    fu.slice(o, u, v, 64, 48, TF_QUERY_METRES, false, out);
    void (Scene<Voxel_s, VoxelBlockHash>::*q)(const float*, long long, tf_query_units, bool, const tf_query_out&) = &Scene<Voxel_s, VoxelBlockHash>::query;
    void (TopFu::*s)(const float*, const float*, const float*, int, int, tf_query_units, bool, const tf_query_out&) = &TopFu::slice;
    (void)q; (void)s;
}
int main() { return 0; }
"""


def test_cpp_api_compiles(tmp_path):
    """A program against include/tfusion's C++ API that calls the four query bindings compiles (syntax only, host
    compiler, as tests/test_cpp_api.py compiles the demo's uses)."""
    src = tmp_path / "query_api.cpp"
    src.write_text(CPP_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                        "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
