"""Inputs of tests/test_gpu_offdefault.py, built on the CPU: frame sizes that are multiples of 4 but
not of 8 (and, for the stateless image functions, odd), stage depth images that reach every branch of
the front end at those sizes, and contexts created with other parameters than the defaults.

Nothing here touches the GPU.  tests/test_offdefault_cases.py asserts on the oracle alone that each
input exercises what it is for, so a GPU test cannot pass on an input that exercises nothing; it also
holds the plain numpy restatements of the integer stages the oracle is compared with."""
import numpy as np

from topfusion_amd import synth

# ---- sizes ----------------------------------------------------------------------------------
# (cols, rows): what the size reaches
STAGE_SIZES = {
    (4, 4): "every pixel on a border; levels 2x2 and 1x1",
    (12, 8): "small",
    (36, 28): "one full and one 4-wide bilateral tile column; levels 18x14 and 9x7",
    (100, 76): "W/8 = 12 against 13 range columns; levels 50x38 and 25x19",
    (164, 124): "10.25 x 7.75 raycast tiles; levels 82x62 and 41x31",
    (644, 484): "many interior tiles plus a 4-pixel rim on both sides",
    # all of the above are 4 past a multiple of 32 wide: two more with 28 and 12 pixels in the last tile column
    (60, 36): "a 28-wide last bilateral tile column, a 4-high last pyramid tile row",
    (108, 44): "a 12-wide last tile column; interior tiles; levels 54x22 and 27x11",
}
ODD_SIZES = ((37, 29), (101, 77), (5, 3))
IMGPROC_SIZES = ((36, 28), (100, 76)) + ODD_SIZES
IMGPROC_KSZ = (1, 4, 7, 9)

# the bilateral tile of tf_preproc.h (PRE_TX x PRE_TY, HALO) and the first depth whose difference to 0
# squares past INT_MAX
TILE_X, TILE_Y, HALO, BIG = 32, 8, 3, 46341

DEFAULT_BILATERAL = dict(bilateral_kernel_size=7, bilateral_sigma_spatial=4.5, bilateral_sigma_depth=0.04)
DEFAULT_TRUNCATE = 2.0

# front-end settings repeated at 100x76: tf_create parameters (the oracle's stage functions take the same)
STAGE_SETTINGS = ([dict(bilateral_kernel_size=k) for k in (1, 2, 3, 4, 5, 6)]
                  + [dict(bilateral_sigma_spatial=1.5, bilateral_sigma_depth=0.01),
                     dict(bilateral_sigma_spatial=4.5, bilateral_sigma_depth=0.2),
                     dict(icp_truncate_depth_dist=0.0), dict(icp_truncate_depth_dist=1.2)])


def setting_id(kw):
    return ",".join(f"{k.replace('bilateral_', '').replace('icp_', '')}={v}" for k, v in kw.items()) or "default"


def stage_depth(W, H):
    """The stage depth image of a size: the noisy room corner with holes (seeded random values of the same
    classes below 16 pixels) plus a block of 60000 touching the bottom-right corner (a `big` tile that is
    masked too), 65535 at (0, 0), a lone 50000 three pixels from the left edge, a patch of 2500 (dists -1, and
    truncated), one more 2500 in the last column (every tap of its window underflows) and a patch quantised
    to 100 mm."""
    if min(W, H) >= 16:
        d = synth.room_corner(W, H, noise_mm=2.0, holes=0.02, seed=3).copy()
        b = max(2, min(W, H) // 12)
        d[H // 5:H // 5 + b, W // 2:W // 2 + 2 * b] = 2500
        d[H // 3, W - 1] = 2500                   # the last column's window leaves the pixel itself out
        qy, qx = H // 2, W // 3
        d[qy:qy + 2 * b, qx:qx + 3 * b] = (d[qy:qy + 2 * b, qx:qx + 3 * b] // 100) * 100
        d[H - b:, W - b:] = 60000
        d[4, 3] = 50000                           # row 4: in the halo of the first tile row only
        d[(3 * H) // 4, W // 2] = 0
    else:
        rng = np.random.default_rng(1000 * W + H)
        d = rng.integers(600, 1900, (H, W)).astype(np.uint16)
        d[rng.random((H, W)) < 0.1] = 0
        d[H // 2, 1] = 0
        d[0, W - 1] = 2500                        # the last column's window leaves the pixel itself out
        d[0, 1] = 2500
        d[1, 1] = (d[1, 1] // 100) * 100
        d[H - 1, W - 1] = 60000
        d[H // 2, min(3, W - 1)] = 50000
    d[0, 0] = 65535
    return d


# ---- plain restatements of the integer stages (imgproc.cu:263-280, 70-89, 98-140) ---------------
def np_compute_dists(d):
    v = d.astype(np.int64)
    return np.where((v >= 2047) | (v <= 0), np.float32(-1.0), v.astype(np.float32) * np.float32(0.001)).astype(np.float32)


def np_truncate(d, max_dist):
    md = int(np.float32(max_dist) * np.float32(1000.0)) & 0xFFFF
    out = d.copy()
    out[d > md] = 0
    return out


def np_pyr_down(d, sigma_depth=0.04):
    """Destination (x, y) of a W/2 x H/2 image: the mean (integer division) of the source values within
    3 sigma of the centre (2x, 2y) over the window [2x-2, min(2x+3, W-1)) x [2y-2, min(2y+3, H-1)),
    clamped at 0; pixel by pixel."""
    H, W = d.shape
    s3 = np.float32(np.float32(np.float32(sigma_depth) * np.float32(1000.0)) * np.float32(3.0))
    src = d.astype(np.int64)
    out = np.zeros((H // 2, W // 2), np.uint16)
    for y in range(H // 2):
        for x in range(W // 2):
            c = src[2 * y, 2 * x]
            win = src[max(2 * y - 2, 0):min(2 * y + 3, H - 1), max(2 * x - 2, 0):min(2 * x + 3, W - 1)]
            keep = win[np.abs(win - c).astype(np.float32) < s3]
            out[y, x] = 0 if keep.size == 0 else int(keep.sum()) // keep.size
    return out


# ---- what the bilateral pass does with an image, derived on the CPU -------------------------------
def bilateral_dead_pixels(d, ksz=7, sigma_spatial=4.5, sigma_depth=0.04):
    """Pixels whose two bilateral sums are both 0 in float32: every tap of the clamped window
    [max(x-k/2, 0), min(x-k/2+k, W-1)) (bilateral_kernel, imgproc.cu:25-46) has an exponent below -100 --
    the canonical exp returns 0 below -86.7 -- or the window is empty.  float64, with the reference's
    wrapping integer square."""
    H, W = d.shape
    v = d.astype(np.int64)
    ss = 0.5 / (sigma_spatial * sigma_spatial)
    sd = 0.5 / ((sigma_depth * 1000.0) ** 2)
    ys, xs = np.mgrid[0:H, 0:W]
    dead = np.ones((H, W), bool)
    half = ksz // 2
    for dy in range(-half, -half + ksz):
        for dx in range(-half, -half + ksz):
            cy, cx = ys + dy, xs + dx
            ok = (cy >= 0) & (cy < H - 1) & (cx >= 0) & (cx < W - 1)
            tap = v[np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)]
            sq = ((v - tap) ** 2) & 0xFFFFFFFF
            sq = np.where(sq >= 1 << 31, sq - (1 << 32), sq)               # (int)(unsigned * unsigned)
            arg = (dx * dx + dy * dy) * ss + sq * sd
            dead &= ~ok | (arg > 100.0)
    return dead


def bilateral_tile_paths(d, ksz=7, fast=True):
    """How many 32x8 tiles of the image take each path of bilateral_block (tf_preproc.h): `big` when the
    tile or its 3-pixel halo (inside the image) holds a depth >= 46341; the unrolled window needs FAST, ksz 7
    and no big value, and is unmasked where every window of the tile is whole."""
    H, W = d.shape
    n = {"interior unrolled": 0, "masked unrolled": 0, "packed loop": 0, "integer loop": 0,
         "integer loop on the right or bottom border": 0}
    for y0 in range(0, H, TILE_Y):
        for x0 in range(0, W, TILE_X):
            big = bool((d[max(y0 - HALO, 0):y0 + TILE_Y + HALO, max(x0 - HALO, 0):x0 + TILE_X + HALO] >= BIG).any())
            whole = x0 >= HALO and y0 >= HALO and x0 + TILE_X + HALO <= W - 1 and y0 + TILE_Y + HALO <= H - 1
            if fast and not big and ksz == 7:
                n["interior unrolled" if whole else "masked unrolled"] += 1
            elif not big:
                n["packed loop"] += 1
            else:
                n["integer loop"] += 1
                if x0 + TILE_X >= W or y0 + TILE_Y >= H:
                    n["integer loop on the right or bottom border"] += 1
    return n


# ---- sequences --------------------------------------------------------------------------------
# (cols, rows): frames of synth.orbit_sequence(n, cols, rows, seed=7); the oracle's verdicts, one digit per
# frame; whether a frame fills the range image outside its /8 region (_run_sequence's need_spill)
SEQUENCES = {
    (100, 76): (8, "11111111"),
    (164, 124): (8, "11111111"),
    (36, 28): (8, "11011010"),
}
NEED_SPILL = {(100, 76): True, (164, 124): True, (36, 28): True}

VARIANT_SIZE, VARIANT_FRAMES = (100, 76), 6
# name: (parameters, the oracle's verdicts, both ICP schedules)
VARIANTS = {
    "iters_3_0_2_0": (dict(icp_iter_num=(3, 0, 2, 0)), "111111", True),
    "iters_6_0_0_0": (dict(icp_iter_num=(6, 0, 0, 0)), "111111", True),
    "iters_0_3_0_0": (dict(icp_iter_num=(0, 3, 0, 0)), "111111", True),
    "iters_0_0_4_0": (dict(icp_iter_num=(0, 0, 4, 0)), "111110", True),
    "iters_0_0_0_0": (dict(icp_iter_num=(0, 0, 0, 0)), "111111", True),
    "dist_thres_0.03": (dict(icp_dist_thres=0.03), "110101", False),
    "angle_thres_0.2": (dict(icp_angle_thres=0.2), "111111", False),
    "maxW_3": (dict(maxW=3), "111111", False),
    "mu_0.035": (dict(mu=0.035), "111111", False),
    "frustum_0.6_1.6": (dict(viewFrustum_min=0.6, viewFrustum_max=1.6), "111101", False),
    "voxel_0.01_mu_0.04": (dict(voxelSize=0.01, mu=0.04), "111111", False),
    "ksz_5": (dict(bilateral_kernel_size=5), "111111", False),
    "ksz_1": (dict(bilateral_kernel_size=1), "111111", False),
    "sigmas_1.5_0.01": (dict(bilateral_sigma_spatial=1.5, bilateral_sigma_depth=0.01), "111111", False),
    "truncate_1.2": (dict(icp_truncate_depth_dist=1.2), "111011", False),
}
ITERS_PER_FRAME = {"iters_3_0_2_0": 5, "iters_6_0_0_0": 6, "iters_0_3_0_0": 3, "iters_0_0_4_0": 4, "iters_0_0_0_0": 0}


def params_kw(W, H, **kw):
    fx, fy, cx, cy = synth.intrinsics(W, H)
    return dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, **kw)


_seq = {}


def sequence(n, W, H):
    if (n, W, H) not in _seq:
        s = synth.orbit_sequence(n, W, H, seed=7)
        s.setflags(write=False)
        _seq[(n, W, H)] = s
    return _seq[(n, W, H)]


def oracle_run(O, W, H, n, **kw):
    """The oracle over the first n orbit frames -> (verdict digits, per-frame counters, pixels of the range
    image above 0.05 outside its /8 region summed over the tracked frames, the oracle)."""
    o = O.Oracle(O.default_params(**params_kw(W, H, **kw)))
    seq = sequence(n, W, H)
    verdicts, counters, spilled = "", [], 0
    rc, rr = (W - 1) // 8 + 1, (H - 1) // 8 + 1
    for k in range(n):
        ok = o(seq[k])
        verdicts += "1" if ok else "0"
        counters.append(o.counters())
        if k > 0 and ok:
            spill = o.range_image()
            spill[:rr, :rc] = 0
            spilled += int((spill[..., 1] > np.float32(0.05)).sum())
    return verdicts, counters, spilled, o
