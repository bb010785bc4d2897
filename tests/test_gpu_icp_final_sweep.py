"""The lane-parallel cv::solve(DECOMP_SVD)'s batched final-sweep test (tf_icp_tail.h,
icp_sv_oneshot): after level 2 of a period whose head pairs (0,1) (0,2) (0,3) (1,2) rotated nothing,
the sweep's other 11 pairs are tested at once on the current state, and the sweeps end there when
none would rotate.  Through tf_icp_solve_systems against the oracle's serial tfo_cv_solve_svd6 /
tfo_cv_det6, every bit of x and det, on systems built to take each way through that test:

 * A = 0 and diagonal A at four scales: sweep 0's head is clean and the try hits at once;
 * exactly one coupled pair A[i][j] = e sqrt(A[i][i] A[j][j]) for each of the 15 pairs, e from 2^0
   down to 2^-36 in factors of 2^-4 with a random mantissa -- across the 2^-22 rotation threshold.
   One of the 11 pairs gives a clean head and a failing batched test (the miss path), a head pair
   never reaches the try, and below the threshold the try hits;
 * the same on equal diagonal entries d with A[i][j] = 2^-23 d and a few float steps either side:
   p / sqrt(ab) = 2 A[i][j] / d (1 + O(2^-46)) there, inside the 2^-41 band in which icp_sv_test
   leaves its fast compare for the exact test;
 * 2 000 random ICP-like systems and the rank 1..5 systems of test_gpu_pose_algebra's generator
   (a zero singular value's finish after the sweeps, whichever way they ended).

tools/svd_lanes_proto.c -oneshot models the same schedule on the CPU (on these systems: 0
differing, tries > hits > 0)."""
import ctypes
import os

import numpy as np
import pytest

from parity_util import DeviceBuffer, DeviceFrames, assert_bit_exact

pytestmark = pytest.mark.gpu

IU = [(a, c) for a in range(6) for c in range(a, 7)]          # the 27 sums: A's upper triangle row by row, b last
PAIRS = [(i, j) for i in range(6) for j in range(i + 1, 6)]
SCALES = (1.0, 1e-6, 1e6, 37.0)


def _pack(A, b):
    return np.array([b[a] if c == 6 else A[a, c] for a, c in IU], np.float32)


def final_sweep_inputs():
    rng = np.random.default_rng(20261019)
    out = [np.zeros(27, np.float32)]                               # A = 0 (b = 0)
    b0 = (rng.random(6, dtype=np.float32) - 0.5)
    out.append(_pack(np.zeros((6, 6), np.float32), b0))            # A = 0, b != 0
    for scale in SCALES:                                           # diagonal
        for _ in range(4):
            d = ((0.5 + rng.random(6, dtype=np.float32)) * np.float32(scale)).astype(np.float32)
            out.append(_pack(np.diag(d), (rng.random(6, dtype=np.float32) - 0.5) * np.float32(scale)))
    for scale in SCALES:                                           # one coupled pair
        for i, j in PAIRS:
            for step in range(10):                                 # e = 2^0 .. 2^-36
                d = ((0.5 + rng.random(6, dtype=np.float32)) * np.float32(scale)).astype(np.float32)
                A = np.diag(d)
                e = np.float32(np.ldexp(0.5 + 0.5 * rng.random(), -4 * step))
                A[i, j] = A[j, i] = e * np.sqrt(d[i] * d[j], dtype=np.float32)
                out.append(_pack(A, (rng.random(6, dtype=np.float32) - 0.5) * np.float32(scale)))
    for scale in SCALES:                                           # one coupled pair at the threshold itself
        for i, j in PAIRS:
            for dd in (np.float32(scale), np.float32(scale) * np.float32(1.3125)):
                c0 = np.float32(dd * np.float32(2.0 ** -23))
                for k in (-2, -1, 0, 1, 2):
                    c = c0
                    for _ in range(abs(k)):
                        c = np.nextafter(c, np.float32(np.inf if k > 0 else 0), dtype=np.float32)
                    A = np.diag(np.full(6, dd, np.float32))
                    # the other rows well apart, so that only (i, j) is near a decision
                    for r in range(6):
                        if r not in (i, j):
                            A[r, r] = dd * np.float32(2 + r)
                    A[i, j] = A[j, i] = c
                    out.append(_pack(A, (rng.random(6, dtype=np.float32) - 0.5) * np.float32(scale)))
    v = rng.random((2000, 30, 7), dtype=np.float32) - 0.5            # random ICP-like
    v[:, :, :3] *= 2
    v[:, :, 6] *= np.float32(0.02)
    out.extend(np.stack([np.einsum("nr,nr->n", v[:, :, a], v[:, :, c]) for a, c in IU], axis=1).astype(np.float32))
    for rank in range(1, 6):                                       # rank deficient
        for _ in range(20):
            w = rng.random((rank, 7), dtype=np.float32) - 0.5
            out.append(np.array([np.dot(w[:, a], w[:, c]) for a, c in IU], np.float32))
    return np.ascontiguousarray(np.stack(out), np.float32)


@pytest.fixture(scope="module")
def systems(oracle_mod):
    """The systems and the oracle's x (one cv::solve for both OpenCV variants: they differ in
    cv::determinant only) -- computed once, shared, read only."""
    sums = final_sweep_inputs()
    n = sums.shape[0]
    Lo = oracle_mod.lib()
    A = np.zeros((n, 6, 6), np.float32)
    b = np.zeros((n, 6), np.float32)
    for q, (a, c) in enumerate(IU):
        if c == 6:
            b[:, a] = sums[:, q]
        else:
            A[:, a, c] = A[:, c, a] = sums[:, q]
    ox = np.zeros((n, 6), np.float32)
    for q in range(n):
        Lo.tfo_cv_solve_svd6(A[q].ctypes.data, b[q].ctypes.data, ox[q].ctypes.data)
    for arr in (sums, A, ox):
        arr.setflags(write=False)
    return sums, A, ox


@pytest.mark.parametrize("algebra", ["opencv4", "opencv2"])
def test_final_sweep_bit_exact(oracle_mod, systems, algebra):
    from topfusion_amd import _lib as L
    sums, A, ox = systems
    n = sums.shape[0]
    code = {"opencv2": 2, "opencv4": 4}[algebra]
    d_in = DeviceFrames(sums)
    d_x = DeviceBuffer(n * 6 * 4)
    d_det = DeviceBuffer(n * 8)
    L.check(L.load().tf_icp_solve_systems(code, d_in.ptr, n, d_x.ptr, d_det.ptr, None), "tf_icp_solve_systems")
    d_x.sync()
    x = np.empty((n, 6), np.float32)
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
    import sys
    final_sweep_inputs().tofile(sys.argv[1])
    print(os.path.abspath(sys.argv[1]))
