"""The lane-parallel cv::solve(DECOMP_SVD)'s fast (c, s) chain (tf_icp_tail.h, icp_sv_cs): the
second v_rsq_f64 seeded from the unrefined first one, V formed without the serial 1 / u, the
rounding-margin check taken beside the row update and the exact sequence only where it fails.
Through tf_icp_solve_systems against the oracle's serial tfo_cv_solve_svd6 / tfo_cv_det6, every
bit of x and det, both OpenCV variants.

The systems are a diagonal plus one coupling A[i][j], so that every other pair has p = 0 and the
first rotation's inputs are known in closed form (float64, exact products, one rounding per sum):

    p = A[i][i] A[i][j] + A[i][j] A[j][j],  a = A[i][i]^2 + A[i][j]^2,  b = A[i][j]^2 + A[j][j]^2,
    beta = a - b,  |2p| / |beta| = 2 A[i][j] / |A[i][i] - A[j][j]|

 * beta > 0 and beta < 0 with |2p| / |beta| = 2^-20 .. 2^20 (nominal: the diagonal difference is
   rounded to float), and beta = 0 (equal diagonal entries) with A[i][j] / A[i][i] = 2^-20 .. 2^-1;
   each at the scales 1e-18, 1e-9, 1, 1e9, 1e18 (X = (2p)^2 + beta^2 over about 2^+-240) and each
   above the 2^-22 rotation threshold (asserted where the systems are built);
 * U or V of that first rotation near a float rounding boundary, found by a seeded search over
   2^21 candidates with the exact sequence in float64: within 2^15 double ulps of a midpoint
   between two floats (inside the 2^16 margin: the exact sequence must run) and between 2^17 and
   2^19 ulps from one (the fast path decides, close to the margin), 24 of each for U and for V
   and for each sign of beta;
 * 300 random ICP-like systems and 300 of rank 1..5 (the generators of
   test_gpu_icp_final_sweep.py): chains of many rotations.

Bit-exactness only: whether the exact sequence ran is read from tools/micro/svd_lanes_stats."""
import ctypes

import numpy as np
import pytest

from parity_util import DeviceBuffer, DeviceFrames, assert_bit_exact

pytestmark = pytest.mark.gpu

IU = [(a, c) for a in range(6) for c in range(a, 7)]          # the 27 sums: A's upper triangle row by row, b last
PAIRS = [(i, j) for i in range(6) for j in range(i + 1, 6)]
SCALES = (1e-18, 1e-9, 1.0, 1e9, 1e18)
F32 = np.float32


def _pack(A, b):
    return np.array([b[a] if c == 6 else A[a, c] for a, c in IU], F32)


def first_rotation(di, dj, c):
    """(2p, beta, a, b) of the pair's first rotation as the sums form them, float64."""
    di, dj, c = (np.asarray(t, np.float64) for t in (di, dj, c))
    p = di * c + c * dj
    a = di * di + c * c
    b = c * c + dj * dj
    return 2 * p, a - b, a, b


def rotates(di, dj, c):
    p2, _, a, b = first_rotation(di, dj, c)
    return np.abs(p2 / 2) > 2.0 ** -22 * np.sqrt(a * b) * (1 + 2.0 ** -30)


def exact_uv(p2, beta):
    """The exact sequence's doubles ahead of their float roundings (icp_sv_cs_exact)."""
    gamma = np.hypot(p2, beta)
    U = np.where(beta < 0, np.sqrt((gamma - beta) * 0.5 / gamma), np.sqrt((gamma + beta) / (gamma * 2)))
    u = U.astype(F32).astype(np.float64)
    V = p2 / (gamma * u * 2)
    return U, V


def boundary_ulps(v):
    """Distance of a double from the nearest midpoint between two (normal) floats, in double ulps."""
    low = (np.abs(v).view(np.uint64) & np.uint64(0x1fffffff)).astype(np.int64)
    return np.abs(low - 0x10000000)


def _system(rng, i, j, di, dj, c, scale):
    """diag + one coupling; the other rows well apart from both and from each other."""
    A = np.zeros((6, 6), F32)
    for r in range(6):
        A[r, r] = F32(scale) * F32(3 + r) * F32(0.75 + 0.5 * rng.random())
    A[i, i], A[j, j] = di, dj
    A[i, j] = A[j, i] = c
    return _pack(A, ((rng.random(6) - 0.5) * scale).astype(F32))


def cs_chain_inputs():
    rng = np.random.default_rng(20261019)
    out = []
    n = 0
    # ---- |2p| / |beta| = 2^k, both signs of beta
    for scale in SCALES:
        for k in range(-20, 21):
            for sign in (1, -1):
                for _ in range(4):
                    i, j = PAIRS[n % 15]
                    n += 1
                    big = F32(scale * (1 + rng.random()))
                    if k <= 0:                      # the difference a fraction of the entry, the coupling small
                        small = F32(big * F32(1 - (0.4 + 0.4 * rng.random())))
                        c = F32(np.ldexp(float(big) - float(small), k - 1))
                    else:                           # the coupling a fraction of the entry, the difference small
                        c = F32(big * F32(0.1 + 0.3 * rng.random()))
                        small = F32(float(big) - np.ldexp(float(c), 1 - k))
                    di, dj = (big, small) if sign > 0 else (small, big)
                    assert di != dj and rotates(di, dj, c), (scale, k, sign)
                    out.append(_system(rng, i, j, di, dj, c, scale))
    # ---- beta = 0
    for scale in SCALES:
        for k in range(-20, 0):
            for _ in range(3):
                i, j = PAIRS[n % 15]
                n += 1
                d = F32(scale * (1 + rng.random()))
                c = F32(np.ldexp(float(d) * (0.75 + 0.5 * rng.random()), k))
                assert first_rotation(d, d, c)[1] == 0 and rotates(d, d, c), (scale, k)
                out.append(_system(rng, i, j, d, d, c, scale))
    # ---- U or V near a float rounding boundary
    N = 1 << 21
    scale = np.exp(rng.uniform(np.log(1e-18), np.log(1e18), N))
    di = (scale * (1 + rng.random(N))).astype(F32)
    dj = (scale * (1 + rng.random(N))).astype(F32)
    c = (scale * np.exp2(rng.uniform(-12, 0, N))).astype(F32)
    p2, beta, _, _ = first_rotation(di, dj, c)
    U, V = exact_uv(p2, beta)
    bu, bv = boundary_ulps(U), boundary_ulps(V)
    ok = rotates(di, dj, c) & (beta != 0)
    picked = np.zeros(N, bool)
    for dist in (bu, bv):
        for sel in (dist < (1 << 15) - 64, (dist > (1 << 17) + 64) & (dist < (1 << 19) - 64)):
            for neg in (False, True):
                idx = np.flatnonzero(ok & sel & ((beta < 0) == neg) & ~picked)[:24]
                assert idx.size == 24, idx.size
                picked[idx] = True
                for q in idx:
                    i, j = PAIRS[n % 15]
                    n += 1
                    out.append(_system(rng, i, j, di[q], dj[q], c[q], float(scale[q])))
    # ---- chains of many rotations
    v = rng.random((300, 30, 7), dtype=F32) - 0.5                   # random ICP-like
    v[:, :, :3] *= 2
    v[:, :, 6] *= F32(0.02)
    out.extend(np.stack([np.einsum("nr,nr->n", v[:, :, a], v[:, :, c]) for a, c in IU], axis=1).astype(F32))
    for rank in range(1, 6):                                       # rank deficient
        for _ in range(60):
            w = rng.random((rank, 7), dtype=F32) - 0.5
            out.append(np.array([np.dot(w[:, a], w[:, c]) for a, c in IU], F32))
    return np.ascontiguousarray(np.stack(out), F32)


@pytest.fixture(scope="module")
def systems(oracle_mod):
    """The systems and the oracle's x (one cv::solve for both OpenCV variants: they differ in
    cv::determinant only) -- computed once, shared, read only."""
    sums = cs_chain_inputs()
    n = sums.shape[0]
    Lo = oracle_mod.lib()
    A = np.zeros((n, 6, 6), F32)
    b = np.zeros((n, 6), F32)
    for q, (a, c) in enumerate(IU):
        if c == 6:
            b[:, a] = sums[:, q]
        else:
            A[:, a, c] = A[:, c, a] = sums[:, q]
    ox = np.zeros((n, 6), F32)
    for q in range(n):
        Lo.tfo_cv_solve_svd6(A[q].ctypes.data, b[q].ctypes.data, ox[q].ctypes.data)
    for arr in (sums, A, ox):
        arr.setflags(write=False)
    return sums, A, ox


@pytest.mark.parametrize("algebra", ["opencv4", "opencv2"])
def test_cs_chain_bit_exact(oracle_mod, systems, algebra):
    from topfusion_amd import _lib as L
    sums, A, ox = systems
    n = sums.shape[0]
    code = {"opencv2": 2, "opencv4": 4}[algebra]
    d_in = DeviceFrames(sums)
    d_x = DeviceBuffer(n * 6 * 4)
    d_det = DeviceBuffer(n * 8)
    L.check(L.load().tf_icp_solve_systems(code, d_in.ptr, n, d_x.ptr, d_det.ptr, None), "tf_icp_solve_systems")
    d_x.sync()
    x = np.empty((n, 6), F32)
    det = np.empty(n, np.float64)
    assert d_x._hip.hipMemcpy(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_x.ptr), ctypes.c_size_t(x.nbytes), 2) == 0
    assert d_x._hip.hipMemcpy(det.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d_det.ptr), ctypes.c_size_t(det.nbytes), 2) == 0
    Lo = oracle_mod.lib()
    od = np.array([Lo.tfo_cv_det6(A[q].ctypes.data, code) for q in range(n)], np.float64)
    for buf in (d_in, d_x, d_det):
        buf.free()
    assert_bit_exact(f"{algebra} solve x", x, ox)
    assert_bit_exact(f"{algebra} det", det, od)


if __name__ == "__main__":                                         # the systems as a file for tools/svd_lanes_proto.c
    import os
    import sys
    cs_chain_inputs().tofile(sys.argv[1])
    print(os.path.abspath(sys.argv[1]))
