"""The inputs of tests/test_gpu_offdefault.py, judged by the oracle alone (no GPU): every stage depth image
reaches the branches it was made for, the oracle's verdicts on the sequences and parameter variants are the
ones recorded in tests/offdefault_cases.py (tracked frames, and resets where listed), and the oracle's
integer stages equal a plain numpy restatement, exact."""
import numpy as np
import pytest

import offdefault_cases as C
from parity_util import assert_bit_exact

ALL_SIZES = tuple(C.STAGE_SIZES) + C.ODD_SIZES


@pytest.mark.parametrize("W,H", ALL_SIZES)
def test_integer_stages_equal_numpy(oracle_mod, W, H):
    """compute_dists, truncate (2.0, 1.2 and 65.535 m) and pyr_down (two levels, on the raw and on the
    filtered image) against the restatements of offdefault_cases."""
    d = C.stage_depth(W, H)
    assert_bit_exact("compute_dists", oracle_mod.compute_dists(d), C.np_compute_dists(d))
    b = oracle_mod.bilateral(d)
    for md in (2.0, 1.2, 65.535):
        assert_bit_exact(f"truncate {md} (filtered)", oracle_mod.truncate(b, md), C.np_truncate(b, md))
        assert_bit_exact(f"truncate {md} (raw)", oracle_mod.truncate(d, md), C.np_truncate(d, md))
    for name, img in (("raw", d), ("filtered", oracle_mod.truncate(b, 2.0))):
        lvl = img
        for l in (1, 2):
            if min(lvl.shape) < 2:
                break
            nxt = oracle_mod.pyr_down(lvl)
            assert nxt.shape == (lvl.shape[0] // 2, lvl.shape[1] // 2)
            assert_bit_exact(f"pyr_down {name} L{l}", nxt, C.np_pyr_down(lvl))
            lvl = nxt


@pytest.mark.parametrize("W,H", ALL_SIZES)
def test_stage_depth_reaches_every_class(oracle_mod, W, H):
    d = C.stage_depth(W, H)
    assert d[0, 0] == 65535 and d[H - 1, W - 1] == 60000 and (d[:, min(3, W - 1)] == 50000).sum() == 1
    # compute_dists: >= 2047, 0 and valid
    dd = oracle_mod.compute_dists(d)
    big, zero = d >= 2047, d == 0
    assert big.any() and zero.any() and (~big & ~zero).any()
    assert (dd[big] == -1).all() and (dd[zero] == -1).all() and (dd[~big & ~zero] > 0).all()
    # truncation removes something from the filtered image
    b = oracle_mod.bilateral(d)
    if (W, H) != (5, 3):               # 5x3: no window without 65535 or 60000; its raw image is truncated instead
        assert ((b > 2000) & (oracle_mod.truncate(b, 2.0) == 0)).any()
    assert ((d > 2000) & (oracle_mod.truncate(d, 2.0) == 0)).any()
    # both bilateral sums 0: with one tap the whole last column and row (an empty window) ...
    dead1 = C.bilateral_dead_pixels(d, 1)
    assert dead1[:, W - 1].all() and dead1[H - 1, :].all()
    assert (oracle_mod.bilateral(d, 1)[dead1] == 0).all()
    # ... with seven the 2500 of the last column (below 12 pixels every window holds the 65535 of (0, 0), whose
    # wrapped square weighs +inf: a NaN quotient, not two empty sums)
    dead7 = C.bilateral_dead_pixels(d, 7)
    if W >= 12:
        assert dead7.any() and (d[dead7] > 0).any()
    assert (b[dead7] == 0).all()
    # a tile with a value >= 46341 on the right or bottom border: the integer loop under a clamped window
    for ksz in (7, 5, 1):
        assert C.bilateral_tile_paths(d, ksz)["integer loop on the right or bottom border"] >= 1
    if min(W, H) >= 28:
        paths = C.bilateral_tile_paths(d, 7)
        assert paths["masked unrolled"] >= 1
        assert C.bilateral_tile_paths(d, 5)["packed loop"] == paths["masked unrolled"] + paths["interior unrolled"]
        assert (paths["interior unrolled"] >= 1) == (W >= 100)
        # level-2 normals: NaN and valid
        d2 = oracle_mod.pyr_down(oracle_mod.pyr_down(oracle_mod.truncate(b, 2.0)))
        fx, fy, cx, cy = [np.float32(v) / np.float32(4) for v in C.synth.intrinsics(W, H)]
        _, nrm = oracle_mod.points_normals(d2, fx, fy, cx, cy)
        nan = np.isnan(nrm[..., 0])
        assert nan.any() and (~nan).any()
        assert not nan[:-1, :-1].all() and nan[-1, :].all() and nan[:, -1].all()


def test_truncation_off_shows_on_the_stage_image(oracle_mod):
    """icp_truncate_depth_dist = 0 keeps what 2.0 removes (the 2500 patch), 1.2 removes more."""
    d = C.stage_depth(100, 76)
    b = oracle_mod.bilateral(d)
    n2 = int((oracle_mod.truncate(b, 2.0) == 0).sum())
    assert int((b == 0).sum()) < n2 < int((oracle_mod.truncate(b, 1.2) == 0).sum())


@pytest.mark.parametrize("kw", C.STAGE_SETTINGS, ids=C.setting_id)
def test_stage_settings_change_the_result(oracle_mod, kw):
    """Every front-end setting of the GPU stage test gives another level-0 depth than the defaults do."""
    d = C.stage_depth(100, 76)
    s = dict(C.DEFAULT_BILATERAL, icp_truncate_depth_dist=C.DEFAULT_TRUNCATE)

    def level0(p):
        b = oracle_mod.bilateral(d, p["bilateral_kernel_size"], p["bilateral_sigma_spatial"], p["bilateral_sigma_depth"])
        return oracle_mod.truncate(b, p["icp_truncate_depth_dist"]) if p["icp_truncate_depth_dist"] > 0 else b

    assert not np.array_equal(level0(s), level0(dict(s, **kw)))


@pytest.mark.parametrize("W,H", list(C.SEQUENCES))
def test_sequence_verdicts(oracle_mod, W, H):
    n, want = C.SEQUENCES[(W, H)]
    verdicts, counters, spilled, _ = C.oracle_run(oracle_mod, W, H, n)
    assert verdicts == want
    assert counters[-1]["n_resets"] == want.count("0")
    if (W, H) == (36, 28):
        assert counters[-1]["n_resets"] >= 1 and want.count("1") >= 4
    assert (spilled > 0) == C.NEED_SPILL[(W, H)], spilled
    assert (W // 8, H // 8) != ((W - 1) // 8 + 1, (H - 1) // 8 + 1)


@pytest.mark.parametrize("name", list(C.VARIANTS))
def test_variant_verdicts(oracle_mod, name):
    kw, want, _ = C.VARIANTS[name]
    W, H = C.VARIANT_SIZE
    verdicts, counters, _, o = C.oracle_run(oracle_mod, W, H, C.VARIANT_FRAMES, **kw)
    assert verdicts == want
    assert counters[-1]["n_resets"] == want.count("0")
    if name in C.ITERS_PER_FRAME:
        tracked = [c["icp_iterations"] for k, c in enumerate(counters) if k > 0 and verdicts[k] == "1"]
        assert tracked and all(t == C.ITERS_PER_FRAME[name] for t in tracked), tracked
    if name == "iters_0_0_0_0":
        assert_bit_exact("pose after 0 iterations", o.pose(), np.eye(4, dtype=np.float32)[:3])
    if name == "maxW_3":
        assert int(o.vba()["w"].max()) == 3
        assert int(C.oracle_run(oracle_mod, W, H, C.VARIANT_FRAMES)[3].vba()["w"].max()) == 6
