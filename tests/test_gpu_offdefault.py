"""GPU parity off the defaults: frame sizes that are multiples of 4 but not of 8 (36x28, 100x76, 164x124,
644x484, down to 4x4), odd sizes for the stateless image functions, and contexts created with other
parameters than TopFuParams::default_params -- bilateral window and sigmas, truncation distance (and none),
ICP iteration counts with empty levels, ICP thresholds, mu, maxW, voxel size, view frustum.  Every comparison
against the oracle, bit for bit.

The inputs come from tests/offdefault_cases.py; tests/test_offdefault_cases.py asserts on the CPU that they
reach what they are for (ragged and `big` bilateral tiles, empty bilateral sums, truncated pixels, NaN and valid
level-2 normals, tracked frames and resets, the range image outside its /8 region)."""
import numpy as np
import pytest

import offdefault_cases as C
from parity_util import DeviceFrames, assert_bit_exact
from test_gpu_engines import Pitched, _f, _ok
from test_gpu_parity import _check_schedule, _compare_frame_state, _run_sequence, compare_scene, make_pair

pytestmark = pytest.mark.gpu

SCHEDULES = ("persistent", "per_iteration")


def _schedule(monkeypatch, sched):
    monkeypatch.setenv("TFUSION_ICP_PERSISTENT", "0" if sched == "per_iteration" else "1")


# ---- the front end, stage by stage -------------------------------------------------------------
def _check_front_end(oracle_mod, W, H, **kw):
    """As test_preprocess: stage_preprocess on a context created with `kw`, then dists, the three depth
    levels and the points and normals of every level against the oracle's stage functions called with the
    same parameters."""
    g, _ = make_pair(oracle_mod, W, H, **kw)
    p = g.params()
    d = C.stage_depth(W, H)
    g.stage_preprocess(d)
    assert_bit_exact("dists", g.dists(), oracle_mod.compute_dists(d))
    d0 = oracle_mod.bilateral(d, p.bilateral_kernel_size, p.bilateral_sigma_spatial, p.bilateral_sigma_depth)
    if p.icp_truncate_depth_dist > 0:
        d0 = oracle_mod.truncate(d0, p.icp_truncate_depth_dist)
    d1 = oracle_mod.pyr_down(d0, p.bilateral_sigma_depth)
    d2 = oracle_mod.pyr_down(d1, p.bilateral_sigma_depth)
    for l, dl in enumerate((d0, d1, d2)):
        assert dl.shape == (H >> l, W >> l)
        assert_bit_exact(f"depth{l}", g.curr_depth(l), dl)
        div = np.float32(1 << l)
        pts, nrm = oracle_mod.points_normals(dl, np.float32(p.fx) / div, np.float32(p.fy) / div, np.float32(p.cx) / div,
                                             np.float32(p.cy) / div)
        gp, gn = g.curr_maps(l)
        assert_bit_exact(f"points L{l}", gp, pts)
        assert_bit_exact(f"normals L{l}", gn, nrm)
    g.close()


@pytest.mark.parametrize("W,H", list(C.STAGE_SIZES))
def test_front_end_sizes(oracle_mod, W, H):
    _check_front_end(oracle_mod, W, H)


@pytest.mark.parametrize("kw", C.STAGE_SETTINGS, ids=C.setting_id)
def test_front_end_settings(oracle_mod, kw):
    """100x76 with another bilateral window (1..6: the packed two-taps loop, and the integer loop with a short
    window in the tiles that hold 65535, 60000 or 50000), other sigmas, no truncation, truncation at 1.2 m."""
    _check_front_end(oracle_mod, 100, 76, **kw)


# ---- the stateless tf_imgproc_* functions ------------------------------------------------------
@pytest.mark.parametrize("W,H", C.IMGPROC_SIZES)
def test_imgproc_sizes(oracle_mod, W, H):
    """All six functions on padded pitches, odd sizes included (pyr_down and resize_points_normals write
    W/2 x H/2, and the last source column is never a centre), the bilateral filter with windows of 1, 4, 7
    and 9 taps."""
    from topfusion_amd import _lib, synth
    L = _lib.load()
    d = C.stage_depth(W, H)
    bufs = []

    def buf(h, w, dtype, ch=None):
        bufs.append(Pitched(h, w, dtype, ch))
        return bufs[-1]

    src = buf(H, W, np.uint16).put(d)
    dists = buf(H, W, np.float32)
    _ok(L.tf_imgproc_compute_dists(src.ptr, src.step, dists.ptr, dists.step, W, H, None), "compute_dists")
    assert_bit_exact("computeDists", dists.get(), oracle_mod.compute_dists(d))
    bil = buf(H, W, np.uint16)
    for ksz in C.IMGPROC_KSZ + (7,):                   # (7 last: the later stages take its output)
        _ok(L.tf_imgproc_bilateral(src.ptr, src.step, bil.ptr, bil.step, W, H, ksz, 4.5, 0.04, None), "bilateral")
        want_bil = oracle_mod.bilateral(d, ksz)
        assert_bit_exact(f"depthBilateralFilter ksz {ksz}", bil.get(), want_bil)
    _ok(L.tf_imgproc_bilateral(src.ptr, src.step, bil.ptr, bil.step, W, H, 5, 1.5, 0.01, None), "bilateral")
    assert_bit_exact("depthBilateralFilter sigmas", bil.get(), oracle_mod.bilateral(d, 5, 1.5, 0.01))
    _ok(L.tf_imgproc_bilateral(src.ptr, src.step, bil.ptr, bil.step, W, H, 7, 4.5, 0.04, None), "bilateral")
    _ok(L.tf_imgproc_truncate(bil.ptr, bil.step, W, H, 2.0, None), "truncate")
    d0 = oracle_mod.truncate(want_bil, 2.0)
    assert_bit_exact("depthTruncation", bil.get(), d0)
    raw = buf(H, W, np.uint16).put(d)
    _ok(L.tf_imgproc_truncate(raw.ptr, raw.step, W, H, 1.2, None), "truncate raw")
    assert_bit_exact("depthTruncation (raw, 1.2)", raw.get(), oracle_mod.truncate(d, 1.2))
    # two pyramid steps: the second one's source is the odd-sized level of 100x76 / 37x29 / 101x77
    lvl_buf, lvl = bil, d0
    for step in (1, 2):
        h, w = lvl.shape
        if min(h, w) < 2:
            break
        nxt_buf = buf(h // 2, w // 2, np.uint16)
        _ok(L.tf_imgproc_pyr_down(lvl_buf.ptr, lvl_buf.step, w, h, nxt_buf.ptr, nxt_buf.step, 0.04, None), "pyr_down")
        nxt = oracle_mod.pyr_down(lvl)
        assert_bit_exact(f"depthBuildPyramid step {step}", nxt_buf.get(), nxt)
        lvl_buf, lvl = nxt_buf, nxt
    intr = np.array(synth.intrinsics(W, H), np.float32)
    pts, nrm = buf(H, W, np.float32, 4), buf(H, W, np.float32, 4)
    _ok(L.tf_imgproc_point_normals(_f(intr), bil.ptr, bil.step, W, H, pts.ptr, pts.step, nrm.ptr, nrm.step, None),
        "point_normals")
    op, on = oracle_mod.points_normals(d0, *[np.float32(v) for v in intr])
    assert_bit_exact("computePointNormals points", pts.get(), op)
    assert_bit_exact("computePointNormals normals", nrm.get(), on)
    p_buf, n_buf = pts, nrm
    for step in (1, 2):
        h, w = op.shape[:2]
        if min(h, w) < 2:
            break
        p2, n2 = buf(h // 2, w // 2, np.float32, 4), buf(h // 2, w // 2, np.float32, 4)
        _ok(L.tf_imgproc_resize_points_normals(p_buf.ptr, p_buf.step, n_buf.ptr, n_buf.step, w, h, p2.ptr, p2.step, n2.ptr,
                                               n2.step, None), "resize")
        op, on = oracle_mod.resize_points_normals(op, on)
        assert_bit_exact(f"resizePointsNormals points step {step}", p2.get(), op)
        assert_bit_exact(f"resizePointsNormals normals step {step}", n2.get(), on)
        p_buf, n_buf = p2, n2
    _ok(L.tf_imgproc_sync(None), "sync")
    for b in bufs:
        b.free()


# ---- whole frames ------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("W,H", list(C.SEQUENCES))
def test_sequence_sizes(oracle_mod, monkeypatch, W, H, sched):
    """TopFu::operator() frame by frame at 100x76 and 164x124 (all tracked) and 36x28 (three resets), the
    state identical after every frame: the ICP's 32x8 CTAs and the raycast's 16x16 tiles ragged on both sides,
    W/8 columns against (W-1)/8+1 in the range image."""
    _schedule(monkeypatch, sched)
    g, o = make_pair(oracle_mod, W, H)
    _check_schedule(g, sched)
    n, verdicts = C.SEQUENCES[(W, H)]
    _run_sequence(g, o, W, H, n, need_spill=C.NEED_SPILL[(W, H)])
    assert o.counters()["n_resets"] == verdicts.count("0")
    g.close()


def test_sequence_ed_atomic(oracle_mod, monkeypatch):
    """k_ed_fill's device-scope-atomic path (TFUSION_ED_LDS_MAX_N=0) at 100x76."""
    monkeypatch.setenv("TFUSION_ED_LDS_MAX_N", "0")
    W, H = 100, 76
    g, o = make_pair(oracle_mod, W, H)
    _run_sequence(g, o, W, H, C.SEQUENCES[(W, H)][0], need_spill=C.NEED_SPILL[(W, H)])
    g.close()


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("kw", [dict(), dict(bilateral_kernel_size=5)], ids=C.setting_id)
def test_batched_frames(oracle_mod, monkeypatch, kw, sched):
    """tf_process_frames over 12 device frames at 100x76: later frames' preprocessing runs in the grid tails
    (bilateral_block<false>, pyr_normals_block<256>) with ragged tiles; compared as
    test_batched_frames_overlap compares."""
    _schedule(monkeypatch, sched)
    W, H, n = 100, 76, 12
    g, o = make_pair(oracle_mod, W, H, **kw)
    _check_schedule(g, sched)
    seq = C.sequence(n, W, H)
    dev = DeviceFrames(seq)
    okg = g.process_frames(dev.ptr, n)
    oko = np.array([o(seq[k]) for k in range(n)])
    assert np.array_equal(okg, oko), (okg, oko)
    assert oko[:6].all()                                   # (tests/test_offdefault_cases.py)
    sg, so = g.stats(), o.counters()
    for key in ("frame_counter", "n_resets", "icp_iterations"):
        assert sg[key] == so[key], f"{key}: gpu {sg[key]} oracle {so[key]}"
    assert_bit_exact("batched final pose", g.getCameraPose()[:3, :4], o.pose())
    if oko[-1]:
        assert_bit_exact("batched last renderImage grey", g.frame_grey(), o.frame_grey())
    compare_scene(g, o, "batched")
    assert_bit_exact("batched final raycast", g.raycast_result(), o.raycast_result())
    for l in range(3):
        for a, b, what in zip(g.prev_maps(l), o.prev_maps(l), ("points", "normals")):
            assert_bit_exact(f"batched prev {what} L{l}", a, b)
    g.close()
    dev.free()


def _variant_runs():
    for name, (_, _, both) in C.VARIANTS.items():
        for sched in (SCHEDULES if both else SCHEDULES[:1]):
            yield pytest.param(name, sched, id=f"{name}-{sched}")


@pytest.mark.parametrize("name,sched", list(_variant_runs()))
def test_parameter_variants(oracle_mod, monkeypatch, name, sched):
    """Six frames at 100x76 on a context created with the variant's parameters, frame by frame: verdict,
    counters, pose; at the end the scene, the raycast and the previous maps.  The verdicts are the ones the
    CPU test pins, so each variant is known to track, and to reset where the table says so."""
    _schedule(monkeypatch, sched)
    kw, verdicts, _ = C.VARIANTS[name]
    W, H = C.VARIANT_SIZE
    g, o = make_pair(oracle_mod, W, H, **kw)
    _check_schedule(g, sched)
    seq = C.sequence(C.VARIANT_FRAMES, W, H)
    for k in range(C.VARIANT_FRAMES):
        okg, oko = g(seq[k]), o(seq[k])
        assert okg == oko == (verdicts[k] == "1"), f"frame {k}: ok gpu {okg} oracle {oko} table {verdicts[k]}"
        sg, so = g.last_stats, o.counters()
        for key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries", "icp_iterations", "frame_counter",
                    "n_resets"):
            assert sg[key] == so[key], f"frame {k} {key}: gpu {sg[key]} oracle {so[key]}"
        if k > 0:
            assert sg["noTotalBlocks"] == so["noTotalBlocks"], f"frame {k} noTotalBlocks"
        assert_bit_exact(f"frame {k} pose", g.getCameraPose()[:3, :4], o.pose())
    compare_scene(g, o, name)
    assert_bit_exact(f"{name} final raycast", g.raycast_result(), o.raycast_result())
    for l in range(3):
        for a, b, what in zip(g.prev_maps(l), o.prev_maps(l), ("points", "normals")):
            assert_bit_exact(f"{name} final prev {what} L{l}", a, b)
    g.close()


def test_colour_tracked_frames(oracle_mod):
    """Four tracked frames at 100x76 on a voxel_rgb context (the bilinear sample's W-2 / H-2 bounds move with
    the size), a registered and an unregistered colour camera; compared as test_gpu_colour's
    test_colour_tracked_frames compares."""
    from test_gpu_colour import _colour_view, _compare_scene, _params
    from topfusion_amd import TopFu, synth
    W, H, n = 100, 76, 4
    seq = C.sequence(n, W, H)
    for registered in (True, False):
        pg, po = _params(oracle_mod, W, H, registered=registered)
        g, o = TopFu(pg), oracle_mod.Oracle(po)
        rgbs = np.stack([_colour_view(*synth.orbit_pose(k), W, H, registered=registered) for k in range(n)])
        dev_d, dev_c = DeviceFrames(seq), DeviceFrames(rgbs)
        for k in range(n):
            if k % 2 == 0:
                okg = g(dev_d.ptr + k * W * H * 2, rgb=dev_c.ptr + k * W * H * 4)
            else:
                okg = g(seq[k], rgb=rgbs[k])
            oko = o(seq[k], rgbs[k])
            assert okg and oko, f"frame {k}: gpu {okg} oracle {oko}"
            _compare_frame_state(g, o, f"registered={registered} frame {k}", grey=k > 0)
        co = _compare_scene(g, o, f"registered={registered} final")
        assert int(((co >> 24) > 0).sum()) > 1000
        want = o.render_image_type(2)
        assert_bit_exact(f"registered={registered} renderImage colour", g.renderImage(2), want)
        assert (want[..., 3] == 255).mean() > 0.5
        dev_d.free()
        dev_c.free()
        g.close()
