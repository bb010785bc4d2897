"""The CPU oracle's front end and ICP rows against the reference's own kernels run on the host.

tests/golden/front_pin_*.bin hold what imgproc.cu's per-pixel kernels and ComputeIcpHelper::find_coresp of
proj_icp.cu (compiled for the host from the reference tree by oracle/ref_pin/ref_pin_front.cpp, over the
executing CUDA stand-ins of oracle/ref_pin/cuda_exec) compute over the cases of tests/front_pin_cases.py
(layouts there).  Here the oracle's stage functions run over the same inputs and must agree bit for bit;
tests/test_gpu_front_pin.py does the same with the HIP kernels.  Only tests/golden and the repository are
read, except by the freshness test, which runs where the reference tree exists.

The two reduction trees (Block::reduce<256>, icp_final_reduce_kernel) cannot run on the host -- their tail is
warp-synchronous -- and are restated in numpy (front_pin_cases.tree_sums): tfo_icp_reduce must equal that tree
over the reference's rows.
"""
import os
import subprocess

import numpy as np
import pytest

import front_pin_cases as F
import offdefault_cases as C
import pin_scenes as P
from parity_util import assert_bit_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/tfusion/src/cuda"


def front_golden(W, H):
    g = F.golden(F.front_case(W, H))
    assert_bit_exact(f"{W}x{H}: input CRC32", g["crc"], F.front_inputs(W, H)["crc"])
    return g


def img(g, name, h, w, ch=None):
    """A stored image, or an empty one for a level without pixels."""
    shape = (h, w) + ((ch,) if ch else ())
    if h * w == 0:
        assert name not in g
        return None
    return g[name].reshape(shape)


# ---- coverage ------------------------------------------------------------------------------------------------
def test_coverage():
    """The committed goldens meet the coverage conditions they were written under, and the size limit."""
    for W, H in F.FRONT_SIZES:
        F.check_front_coverage(W, H)
        assert F.golden_parts(F.front_case(W, H))
        assert ("points0" in front_golden(W, H)) == ((W, H) not in F.U16_ONLY)
    for W, H in F.ICP_SIZES:
        F.check_icp_coverage(F.golden(F.icp_case(W, H)), W, H)
    for name in os.listdir(P.GOLDEN):
        if name.startswith("front_pin_"):
            assert os.path.getsize(os.path.join(P.GOLDEN, name)) <= P.MAX_GOLDEN_BYTES, name


# ---- the front end --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", F.FRONT_SIZES)
def test_front_end(oracle_mod, W, H):
    """Every front-end golden of a size against the oracle's stage functions."""
    O, g, d = oracle_mod, front_golden(W, H), F.front_depth(W, H)
    assert_bit_exact("compute_dists_kernel", O.compute_dists(d), g["dists"].reshape(H, W))
    for name, ksz, ss, sd in F.BILATERALS:
        assert_bit_exact(f"bilateral_kernel {name}", O.bilateral(d, ksz, ss, sd), g[name].reshape(H, W))
    bil7 = g["bil_k7"].reshape(H, W)
    for name, dist in F.TRUNCATES:
        assert_bit_exact(f"truncate_depth_kernel {name}", O.truncate(bil7, dist), g[name].reshape(H, W))
    assert not g["trunc_0"].any()
    if min(W, H) >= 16:
        assert g["trunc_1.2"].any() and (g["trunc_1.2"] != g["trunc_2.0"]).any() and (g["trunc_2.0"] != g["bil_k7"]).any()
    depth = [g["trunc_2.0"].reshape(H, W)]
    for l in (1, 2):
        h, w = F.level_shape(W, H, l)
        want = img(g, f"pyr{l}", h, w)
        if want is None:
            break
        assert_bit_exact(f"pyramid_kernel step {l}", O.pyr_down(depth[-1]), want)
        depth.append(want)
    if (W, H) in F.U16_ONLY:
        return
    maps = []
    for l, dl in enumerate(depth):
        h, w = dl.shape
        pts, nrm = O.points_normals(dl, *F.intrinsics(W, H, l))
        assert_bit_exact(f"points_normals_kernel points L{l}", pts, g[f"points{l}"].reshape(h, w, 4))
        assert_bit_exact(f"points_normals_kernel normals L{l}", nrm, g[f"normals{l}"].reshape(h, w, 4))
        maps.append((pts, nrm))
    # the w components of the NaN maps: NaN from points_normals, 0 from the resize
    nan0 = np.isnan(g["points0"].reshape(H, W, 4)[..., 0])
    assert nan0.any() and np.isnan(g["points0"].reshape(H, W, 4)[nan0][:, 3]).all()
    pts, nrm = g["points0"].reshape(H, W, 4), g["normals0"].reshape(H, W, 4)
    for l in (1, 2):
        h, w = F.level_shape(W, H, l)
        wp, wn = img(g, f"resized_points{l}", h, w, 4), img(g, f"resized_normals{l}", h, w, 4)
        if wp is None:
            break
        rp, rn = O.resize_points_normals(pts, nrm)
        assert_bit_exact(f"resize_points_normals_kernel points step {l}", rp, wp)
        assert_bit_exact(f"resize_points_normals_kernel normals step {l}", rn, wn)
        nan = np.isnan(wp[..., 0])
        assert (wp[nan][:, 3] == 0).all() and (wp[~nan][:, 3] == 1).all() and (wn[..., 3] == 0).all()
        pts, nrm = wp, wn


# ---- ICP rows ---------------------------------------------------------------------------------------------------
def icp_golden(oracle_mod, W, H):
    """The golden of a size, its input CRC32 checked: the frames, and the one-step affines the oracle reaches
    on its own maps."""
    g = F.golden(F.icp_case(W, H))
    assert_bit_exact(f"icp {W}x{H}: input CRC32", g["crc"], F.icp_inputs(oracle_mod, W, H)["crc"])
    return g


def icp_maps(g, W, H, l):
    h, w = F.level_shape(W, H, l)
    return [g[f"{n}{l}"].reshape(h, w, 4) for n in ("vcurr", "ncurr", "vprev", "nprev")]


@pytest.mark.parametrize("W,H", F.ICP_SIZES)
def test_icp_maps(oracle_mod, W, H):
    """The reference's front end over two frames of a sequence: the maps the ICP cases run on."""
    g = icp_golden(oracle_mod, W, H)
    seq = C.sequence(2, W, H)
    curr, prev = F.oracle_pyramid(oracle_mod, seq[1], W, H), F.oracle_pyramid(oracle_mod, seq[0], W, H)
    for l in range(3):
        vc, nc, vp, npv = icp_maps(g, W, H, l)
        for what, got, want in (("vcurr", curr[l][0], vc), ("ncurr", curr[l][1], nc), ("vprev", prev[l][0], vp), ("nprev", prev[l][1], npv)):
            assert_bit_exact(f"{W}x{H} {what} L{l}", got, want)


@pytest.mark.parametrize("W,H", F.ICP_SIZES)
def test_icp_rows_per_pixel(oracle_mod, W, H):
    """tfo_test_icp_rows (the function tfo_icp_reduce sums) against find_coresp's return code and the row of
    every pixel, under every affine and threshold set: a failure names the pixel."""
    g = icp_golden(oracle_mod, W, H)
    assert_bit_exact("thr", g["thr"], np.array(F.THRESHOLDS, np.float32).reshape(-1))
    for l, t, a in F.keys():
        k = F.key(l, t, a)
        h, w = F.level_shape(W, H, l)
        mc, d2 = F.thresholds(t)
        code, rows = oracle_mod.icp_rows(*icp_maps(g, W, H, l), *F.intrinsics(W, H, l), mc, d2, g["aff_" + k])
        assert_bit_exact(f"{W}x{H} {k} return code", code, g["code_" + k].reshape(h, w))
        assert_bit_exact(f"{W}x{H} {k} row", rows, F.full_rows(g["code_" + k], g["rows_" + k], h, w))
    assert_bit_exact("identity", g["aff_" + F.key(0, 0, 0)].reshape(3, 4), np.eye(3, 4, dtype=np.float32))
    assert_bit_exact("fixed affine", g["aff_" + F.key(1, 1, 2)].reshape(3, 4), F.fixed_affine())


@pytest.mark.parametrize("W,H", F.ICP_SIZES)
def test_icp_sums_against_the_tree(oracle_mod, W, H):
    """tfo_icp_reduce's 27 sums against the numpy tree over the reference's rows."""
    g = icp_golden(oracle_mod, W, H)
    for l, t, a in F.keys():
        k = F.key(l, t, a)
        h, w = F.level_shape(W, H, l)
        mc, d2 = F.thresholds(t)
        sums = oracle_mod.icp_reduce(*icp_maps(g, W, H, l), *F.intrinsics(W, H, l), mc, d2, g["aff_" + k])
        assert_bit_exact(f"{W}x{H} {k} sums", sums, F.tree_sums(F.full_rows(g["code_" + k], g["rows_" + k], h, w)))


def test_tree_past_the_goldens(oracle_mod):
    """644x484: 21 x 61 = 1281 partials, so the final kernel's strided serial sums run up to six rounds.  The
    numpy tree over tfo_test_icp_rows against tfo_icp_reduce (no golden: the rows are pinned at the sizes above)."""
    W, H = 644, 484
    seq = C.sequence(2, W, H)
    curr, prev = F.oracle_pyramid(oracle_mod, seq[1], W, H), F.oracle_pyramid(oracle_mod, seq[0], W, H)
    mc, d2 = F.thresholds(0)
    assert ((W + 31) // 32) * ((H + 7) // 8) == 1281
    for aff in (np.eye(3, 4, dtype=np.float32), F.fixed_affine()):
        args = (curr[0][0], curr[0][1], prev[0][0], prev[0][1], *F.intrinsics(W, H), mc, d2, aff)
        code, rows = oracle_mod.icp_rows(*args)
        assert (code == 0).sum() > W * H // 2
        assert_bit_exact("644x484 sums", oracle_mod.icp_reduce(*args), F.tree_sums(rows))


# ---- freshness, with the sanitizer run ------------------------------------------------------------------------------
def _run_all(exe, out, env=None):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(P.GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    out.mkdir()
    F._golden.clear()
    mg.run_front_pin(str(exe), str(out))
    F._golden.clear()
    names = sorted(os.listdir(out))
    assert names == sorted(n for n in os.listdir(P.GOLDEN) if n.startswith("front_pin_"))
    for n in names:
        with open(out / n, "rb") as a, open(os.path.join(P.GOLDEN, n), "rb") as b:
            assert a.read() == b.read(), f"{n} differs from the committed golden ({exe})"


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")
def test_goldens_are_fresh(tmp_path):
    """Where the reference tree exists: the pin program, rebuilt from it by the Makefile's own recipe into a
    temporary directory, writes the committed goldens byte for byte -- built with -O2, without it, and as a
    stand-alone host program under -fsanitize=address,undefined, whose run over all cases must also end clean."""
    builds = (("O2", []), ("O0", ["REF_FRONT_OPT=-O0"]),
              ("san", ["REF_FRONT_OPT=-O1 -g", "REF_FRONT_EXTRA=-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer"]))
    for name, args in builds:
        ref_out = tmp_path / f"_ref_{name}"
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref_front", f"REF_OUT={ref_out}"] + args,
                           capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        _run_all(ref_out / "ref_pin_front", tmp_path / f"out_{name}")
