"""The HIP front end and the ICP reduction against the reference's own kernels run on the host.

The expected values are the goldens tests/golden/front_pin_*.bin (tests/front_pin_cases.py: what imgproc.cu's
per-pixel kernels and ComputeIcpHelper::find_coresp compute, compiled for the host from the reference tree),
not the oracle's: the stateless tf_imgproc_* functions and the context's own front end (tf_stage_preprocess,
and tf_process_frames for the grid-tail forms) against every front-end golden, and the 27 sums of
tf_icp_estimate against the reference's two reduction trees restated in numpy (front_pin_cases.tree_sums) over
the golden rows.  Existing entry points only; everything bit for bit.
"""
import ctypes

import numpy as np
import pytest

import front_pin_cases as F
import offdefault_cases as C
from parity_util import DeviceFrames, assert_bit_exact
from test_gpu_engines import Pitched, _f, _ok
from test_gpu_icp_window import _icp_result, _Pyramids

pytestmark = pytest.mark.gpu

SCHEDULES = ("persistent", "per_iteration")


def _levels(g, W, H, u16):
    """[(depth, points, normals)] per level the golden of a size holds (maps None at the u16-only sizes)."""
    out = []
    for l, name in enumerate(("trunc_2.0", "pyr1", "pyr2")):
        h, w = F.level_shape(W, H, l)
        if h * w == 0:
            break
        maps = (None, None) if u16 else (g[f"points{l}"].reshape(h, w, 4), g[f"normals{l}"].reshape(h, w, 4))
        out.append((g[name].reshape(h, w),) + maps)
    return out


# ---- the stateless tf_imgproc_* functions ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", F.FRONT_SIZES)
def test_imgproc_against_the_goldens(W, H):
    """All six functions on padded pitches against every front-end golden of a size: the dists, the five
    bilateral settings, the three truncations, two pyramid steps, points and normals of every level with the
    intrinsics divided as the reference divides them, and two resize steps."""
    from topfusion_amd import _lib
    L = _lib.load()
    g, d, u16 = F.golden(F.front_case(W, H)), F.front_depth(W, H), (W, H) in F.U16_ONLY
    bufs = []

    def buf(h, w, dtype, ch=None):
        bufs.append(Pitched(h, w, dtype, ch))
        return bufs[-1]

    src = buf(H, W, np.uint16).put(d)
    dists = buf(H, W, np.float32)
    _ok(L.tf_imgproc_compute_dists(src.ptr, src.step, dists.ptr, dists.step, W, H, None), "compute_dists")
    assert_bit_exact("compute_dists_kernel", dists.get(), g["dists"].reshape(H, W))
    bil = buf(H, W, np.uint16)
    for name, ksz, ss, sd in F.BILATERALS:
        _ok(L.tf_imgproc_bilateral(src.ptr, src.step, bil.ptr, bil.step, W, H, ksz, ss, sd, None), "bilateral")
        assert_bit_exact(f"bilateral_kernel {name}", bil.get(), g[name].reshape(H, W))
    for name, dist in F.TRUNCATES:
        t = buf(H, W, np.uint16).put(g["bil_k7"].reshape(H, W))
        _ok(L.tf_imgproc_truncate(t.ptr, t.step, W, H, dist, None), "truncate")
        assert_bit_exact(f"truncate_depth_kernel {name}", t.get(), g[name].reshape(H, W))
    levels = _levels(g, W, H, u16)
    for l, (dl, pts, nrm) in enumerate(levels):
        h, w = dl.shape
        lvl = buf(h, w, np.uint16).put(dl)
        if l + 1 < len(levels):
            nxt = buf(h // 2, w // 2, np.uint16)
            _ok(L.tf_imgproc_pyr_down(lvl.ptr, lvl.step, w, h, nxt.ptr, nxt.step, 0.04, None), "pyr_down")
            assert_bit_exact(f"pyramid_kernel step {l + 1}", nxt.get(), levels[l + 1][0])
        if u16:
            continue
        p, n = buf(h, w, np.float32, 4), buf(h, w, np.float32, 4)
        intr = np.array(F.intrinsics(W, H, l), np.float32)
        _ok(L.tf_imgproc_point_normals(_f(intr), lvl.ptr, lvl.step, w, h, p.ptr, p.step, n.ptr, n.step, None), "point_normals")
        assert_bit_exact(f"points_normals_kernel points L{l}", p.get(), pts)
        assert_bit_exact(f"points_normals_kernel normals L{l}", n.get(), nrm)
    if not u16:
        pts, nrm = levels[0][1], levels[0][2]
        for l in (1, 2):
            h, w = F.level_shape(W, H, l)
            if h * w == 0:
                break
            pi, ni = buf(pts.shape[0], pts.shape[1], np.float32, 4).put(pts), buf(nrm.shape[0], nrm.shape[1], np.float32, 4).put(nrm)
            po, no = buf(h, w, np.float32, 4), buf(h, w, np.float32, 4)
            _ok(L.tf_imgproc_resize_points_normals(pi.ptr, pi.step, ni.ptr, ni.step, pts.shape[1], pts.shape[0], po.ptr, po.step,
                                                   no.ptr, no.step, None), "resize")
            pts, nrm = g[f"resized_points{l}"].reshape(h, w, 4), g[f"resized_normals{l}"].reshape(h, w, 4)
            assert_bit_exact(f"resize_points_normals_kernel points step {l}", po.get(), pts)
            assert_bit_exact(f"resize_points_normals_kernel normals step {l}", no.get(), nrm)
    _ok(L.tf_imgproc_sync(None), "sync")
    for b in bufs:
        b.free()


# ---- the context's front end (bilateral_block, pyr_normals_block) ---------------------------------------------------------
# (tf_create parameters, the golden that is the context's level-0 depth); the window is at most 7 taps in a context
CONTEXT_SETTINGS = (
    (dict(), "trunc_2.0"),
    (dict(icp_truncate_depth_dist=1.2), "trunc_1.2"),
    (dict(icp_truncate_depth_dist=0.0, bilateral_kernel_size=1), "bil_k1"),
    (dict(icp_truncate_depth_dist=0.0, bilateral_kernel_size=4), "bil_k4"),
    (dict(icp_truncate_depth_dist=0.0), "bil_k7"),
    (dict(icp_truncate_depth_dist=0.0, bilateral_kernel_size=5, bilateral_sigma_spatial=1.5, bilateral_sigma_depth=0.01), "bil_k5_s1.5_0.01"),
)


def _context(W, H, **kw):
    from topfusion_amd import TopFu, default_params
    return TopFu(default_params(**C.params_kw(W, H, **kw)))


def _compare_pyramid(tag, ctx, g, W, H):
    """dists, the three depth levels and the points and normals of every level of a default context."""
    assert_bit_exact(f"{tag} dists", ctx.dists(), g["dists"].reshape(H, W))
    for l, (dl, pts, nrm) in enumerate(_levels(g, W, H, (W, H) in F.U16_ONLY)):
        assert_bit_exact(f"{tag} depth L{l}", ctx.curr_depth(l), dl)
        if pts is not None:
            gp, gn = ctx.curr_maps(l)
            assert_bit_exact(f"{tag} points L{l}", gp, pts)
            assert_bit_exact(f"{tag} normals L{l}", gn, nrm)


@pytest.mark.parametrize("W,H", F.CONTEXT_SIZES)
def test_stage_preprocess_against_the_goldens(W, H):
    """tf_stage_preprocess on contexts created with the goldens' parameters: the whole pyramid of the default
    context, and the level-0 depth under the other windows, sigmas and truncation distances."""
    g, d = F.golden(F.front_case(W, H)), F.front_depth(W, H)
    for kw, name in CONTEXT_SETTINGS:
        ctx = _context(W, H, **kw)
        ctx.stage_preprocess(d)
        if not kw:
            _compare_pyramid(f"{W}x{H}", ctx, g, W, H)
        else:
            assert_bit_exact(f"{W}x{H} {C.setting_id(kw)} dists", ctx.dists(), g["dists"].reshape(H, W))
            assert_bit_exact(f"{W}x{H} {C.setting_id(kw)} depth L0", ctx.curr_depth(0), g[name].reshape(H, W))
        ctx.close()


def test_batched_frames_against_the_goldens():
    """tf_process_frames over four copies of the 100x76 stage image: the later frames' front end runs in the
    grid tails (bilateral_block<false>, pyr_normals_block<256>); the pyramid the last frame leaves is the golden's."""
    W, H, n = 100, 76, 4
    g = F.golden(F.front_case(W, H))
    ctx = _context(W, H)
    dev = DeviceFrames(np.stack([F.front_depth(W, H)] * n))
    ctx.process_frames(dev.ptr, n)
    _compare_pyramid("batched 100x76", ctx, g, W, H)
    ctx.close()
    dev.free()


# ---- ICP sums ---------------------------------------------------------------------------------------------------------------
def _estimate(ctx, pyr, W, H, t, level, iterations):
    """tf_icp_estimate from the identity with `iterations` at `level` only, under threshold set t ->
    (working affine, the 27 sums of the last iteration, iterations run)."""
    from topfusion_amd import _lib
    L = _lib.load()
    dist, angle = F.THRESHOLDS[t]
    iters = [0, 0, 0, 0]
    iters[level] = iterations
    _lib.check(L.tf_icp_set_params(ctx._h, float(np.float32(dist)), float(np.float32(angle)), (ctypes.c_int * 4)(*iters)), "tf_icp_set_params")
    intr = np.array(F.intrinsics(W, H), np.float32)
    aff = np.zeros(12, np.float32)
    ok, n = ctypes.c_int(), ctypes.c_int()
    _lib.check(L.tf_icp_estimate(ctx._h, intr.ctypes.data_as(ctypes.c_void_p), pyr.cl, pyr.pl, 3, aff.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.byref(ok), ctypes.byref(n)), "tf_icp_estimate")
    raff, rsums, rok, rn = _icp_result(ctx)
    assert rn == n.value == iterations, (rn, n.value, iterations)
    return raff, rsums, rok


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("W,H", F.ICP_SIZES)
def test_icp_sums_against_the_tree(monkeypatch, W, H, sched):
    """tf_icp_estimate on the golden's maps as caller pyramids, one iteration at level 0, 1 or 2 under both
    threshold sets: the 27 sums tf_icp_get_result reports equal the numpy tree over the reference's rows under
    the identity, and the affine after that iteration is the stored one-step affine, bit for bit.  With two
    iterations the sums equal the tree over the rows stored for that affine."""
    monkeypatch.setenv("TFUSION_ICP_PERSISTENT", "0" if sched == "per_iteration" else "1")
    g = F.golden(F.icp_case(W, H))
    ctx = _context(W, H)
    assert ctx.icp_persistent() == (sched == "persistent")
    maps = [[g[f"{n}{l}"].reshape(*F.level_shape(W, H, l), 4) for n in ("vcurr", "ncurr", "vprev", "nprev")] for l in range(3)]
    pyr = _Pyramids([(m[0], m[1]) for m in maps], [(m[2], m[3]) for m in maps])

    def tree(l, t, a):
        h, w = F.level_shape(W, H, l)
        return F.tree_sums(F.full_rows(g["code_" + F.key(l, t, a)], g["rows_" + F.key(l, t, a)], h, w))

    for t in range(2):
        for l in range(3):
            tag = f"{W}x{H} {sched} level {l} thresholds {t}"
            aff, sums, ok = _estimate(ctx, pyr, W, H, t, l, 1)
            assert ok == 1, tag
            assert_bit_exact(f"{tag}: sums of iteration 1", sums, tree(l, t, 0))
            assert_bit_exact(f"{tag}: affine after iteration 1", aff, g["aff_" + F.key(l, t, 1)])
            aff, sums, ok = _estimate(ctx, pyr, W, H, t, l, 2)
            assert_bit_exact(f"{tag}: sums of iteration 2", sums, tree(l, t, 1))
    pyr.free()
    ctx.close()
