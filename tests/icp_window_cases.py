"""Inputs of tests/test_gpu_icp_window.py, built on the CPU.

A small seeded family of point / normal pyramids for estimateTransform on caller maps, made so
that the det check (projective_icp.cpp:197-203) fails at a chosen place of the launch: the
previous frame is a plane facing the camera with a band of a second, slanted plane (the off-plane
pixels, which make the system regular), the current frame the same scene seen from a moved
camera.  The maps of a level are valid only inside a window; at a chosen level the previous
maps' window is a narrow strip, so that the correspondences there drop out as the pose moves
(A = 0, det = 0), or is empty, so that the level's first iteration fails.  The levels of a
pyramid are independent inputs of tf_icp_estimate, which is what lets a case choose its level.

Nothing here knows where a case fails: `oracle_estimate` runs the oracle's estimateTransform loop
and `position` names the place of the failing iteration."""
import ctypes

import numpy as np

W, H = 96, 72
ITERS = (3, 3, 3, 0)            # level 0, 1, 2, 3 (setIterationsNum): 9 iterations, levels 2 -> 1 -> 0
DIST, ANGLE = 0.1, np.float32(np.deg2rad(30.0))      # setDistThreshold, setAngleThreshold (radians)
CLASSES = ("iteration 0", "middle of a level", "last of a level", "first of the next level", "last of the launch")


def intrinsics(l):
    s = np.float32(1 << l)
    return (np.float32(80.0) / s, np.float32(80.0) / s, np.float32(W / 2 - 0.5) / s, np.float32(H / 2 - 0.5) / s)


def _render(l, planes, R, t, window):
    """Points / normals (h, w, 4) of the planes (world n . p = d, each with an image mask function)
    seen from the camera p_world = R p_cam + t, valid inside window = (x0, x1, y0, y1) only."""
    h, w = H >> l, W >> l
    fx, fy, cx, cy = [float(v) for v in intrinsics(l)]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    ray = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1)
    pts = np.full((h, w, 4), np.nan, np.float32)
    nrm = np.full((h, w, 4), np.nan, np.float32)
    for n, d, mask in planes:
        nc = R.T @ n
        dc = d - float(n @ t)
        den = ray @ nc
        z = np.where(np.abs(den) > 1e-9, dc / np.where(den == 0, 1, den), np.nan)
        m = mask(xs / w, ys / h) & np.isfinite(z) & (z > 0.1)
        p = ray * z[..., None]
        pts[m, :3] = p[m]
        pts[m, 3] = 0
        nrm[m, :3] = nc
        nrm[m, 3] = 0
    x0, x1, y0, y1 = window
    out = np.ones((h, w), bool)
    out[int(y0 * h):int(y1 * h), int(x0 * w):int(x1 * w)] = False
    pts[out] = np.nan
    nrm[out] = np.nan
    return pts, nrm


def _rot(rv):
    th = float(np.linalg.norm(rv))
    if th == 0:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_case(seed):
    """-> (curr, prev): per level l = 0..2 a (points, normals) pair."""
    rng = np.random.default_rng(1000 + seed)
    n0 = np.array([0.0, 0.0, -1.0])
    a, b = rng.uniform(-0.5, 0.5, 2)
    n1 = np.array([a, b, -1.0])
    n1 /= np.linalg.norm(n1)
    n2 = np.array([-b, a, -1.0])
    n2 /= np.linalg.norm(n2)
    planes = [(n0, -1.0, lambda u, v: (u < 0.55)),
              (n1, float(n1 @ np.array([0.0, 0.0, 1.0])), lambda u, v: (u >= 0.55) & (v < 0.5)),
              (n2, float(n2 @ np.array([0.0, 0.0, 1.0])), lambda u, v: (u >= 0.55) & (v >= 0.5))]
    scale = rng.choice([0.2, 0.5, 1.0, 1.6])
    R = _rot(rng.normal(0, 0.02, 3) * scale)
    t = rng.normal(0, 0.03, 3) * scale
    special = int(rng.integers(0, 4))                 # the level whose previous maps are cut down (3: none)
    kind = int(rng.integers(0, 3))                    # 0: empty, 1: a strip of the facing plane, 2: a strip at the band's edge
    curr, prev = [], []
    for l in range(3):
        cw = (0.1, 0.9, 0.1, 0.9)
        pw = (0.0, 1.0, 0.0, 1.0)
        if l == special:
            if kind == 0:
                pw = (0.0, 0.0, 0.0, 0.0)
            elif kind == 1:
                x = rng.uniform(0.15, 0.4)
                pw = (x, x + rng.uniform(0.05, 0.12), 0.1, 0.9)
                cw = (x, x + 0.1, 0.2, 0.8)
            else:
                x = rng.uniform(0.5, 0.56)
                pw = (x, x + rng.uniform(0.05, 0.1), 0.0, 1.0)
                cw = (x - 0.02, x + 0.12, 0.1, 0.9)
        prev.append(_render(l, planes, np.eye(3), np.zeros(3), pw))
        curr.append(_render(l, planes, R, t, cw))
    return curr, prev


def cosf(x):
    libm = ctypes.CDLL("libm.so.6")
    libm.cosf.argtypes = [ctypes.c_float]
    libm.cosf.restype = ctypes.c_float
    return libm.cosf(x)


def oracle_estimate(O, curr, prev, iters=ITERS, dist=DIST, angle=ANGLE, intr=intrinsics):
    """estimateTransform (projective_icp.cpp:169-213) by the oracle's reduction and step.
    -> (ok, iterations run, affine[12], the last iteration's 27 sums)."""
    affine = np.eye(4, dtype=np.float32)[:3].copy().reshape(12)
    n, sums = 0, np.zeros(27, np.float32)
    used = max([l + 1 for l in range(4) if iters[l]] or [0])
    for l in range(used - 1, -1, -1):
        fx, fy, cx, cy = intr(l)
        for _ in range(iters[l]):
            sums = O.icp_reduce(curr[l][0], curr[l][1], prev[l][0], prev[l][1], fx, fy, cx, cy, cosf(float(angle)),
                                np.float32(dist) * np.float32(dist), affine)
            n += 1
            ok, nxt, _ = O.icp_step(sums, affine)
            if not ok:
                return False, n, affine, sums
            affine = nxt
    return True, n, affine, sums


def position(n_run, iters=ITERS):
    """The class (index into CLASSES) of a det failure at iteration n_run - 1 (0-based)."""
    k = n_run - 1
    order = [iters[l] for l in range(3, -1, -1) if iters[l]]
    total = sum(order)
    if k == 0:
        return 0
    if k == total - 1:
        return 4
    first = 0
    for cnt in order:
        if k == first and first > 0:
            return 3
        if k == first + cnt - 1:
            return 2
        if first < k < first + cnt - 1:
            return 1
        first += cnt
    raise AssertionError(k)

