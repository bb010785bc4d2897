#!/usr/bin/env python3
"""Time of mesh extraction on the bench's scene (DESIGN.md §Mesh extraction, measurement).

Fuses the C2 orbit (bench.py's flagship workload: the synthetic room + sphere orbit at 640x480) for
one 32-frame window, then times tf_mesh_extract with HIP events recorded on the context stream
around the call: the count-only run (count + prefix) and the full run (count + prefix + emit into a
buffer that holds every triangle).  Prints the live blocks, the triangles, the milliseconds of both
runs (median of --reps after --warmup) and the bytes per second each achieves against its floor:

    count: live blocks x 2 KiB read once
    full : live blocks x 2 KiB read once per pass (count, emit) + 36 B per triangle written

and that figure's ratio to the HBM peak.  One JSON line at the end.

    python tools/mesh_time.py [--frames 32] [--reps 20] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM_GBS = 8000.0        # MI355X HBM3E peak, as bench.py takes it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    from topfusion_amd import TopFu, default_params, synth, _lib as L
    W, H = args.cols, args.rows
    fx, fy, cx, cy = synth.intrinsics(W, H)
    tf = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy), device=0)
    frames = synth.orbit_device(args.frames, W, H, seed=7)
    ok = tf.process_frames(frames.ptr, args.frames)
    live = int((tf.hash()["ptr"] >= 0).sum())
    n = tf.mesh_count()

    lib, hip = L.load(), L.hip_runtime()
    hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventDestroy.argtypes = [ctypes.c_void_p]
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    stream = ctypes.c_void_p(tf.stream())
    dev = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev), max(16, n * 36)) == 0, "hipMalloc"

    def timed(buf, cap):
        got = ctypes.c_longlong()
        ms = []
        for i in range(args.warmup + args.reps):
            assert hip.hipEventRecord(e0, stream) == 0
            L.check(lib.tf_mesh_extract(tf._h, buf, cap, ctypes.byref(got)), "tf_mesh_extract")
            assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
            t = ctypes.c_float()
            assert hip.hipEventElapsedTime(ctypes.byref(t), e0, e1) == 0
            assert got.value == n
            if i >= args.warmup:
                ms.append(t.value)
        return float(np.median(ms)), float(np.min(ms))

    count_ms, count_min = timed(None, 0)
    full_ms, full_min = timed(dev, n)
    hip.hipFree(dev)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    floor_count = live * 2048
    floor_full = 2 * live * 2048 + 36 * n
    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9
    out = {"tool": "mesh_time", "frames": args.frames, "frames_ok": int(ok.sum()), "cols": W, "rows": H,
           "hash_entries": tf.n_total, "live_blocks": live, "triangles": n,
           "count_ms": round(count_ms, 4), "count_ms_min": round(count_min, 4),
           "full_ms": round(full_ms, 4), "full_ms_min": round(full_min, 4),
           "floor_bytes_count": floor_count, "floor_bytes_full": floor_full,
           "count_gbs": round(gbs(floor_count, count_ms), 2), "full_gbs": round(gbs(floor_full, full_ms), 2),
           "count_frac_of_hbm_peak": round(gbs(floor_count, count_ms) / PEAK_HBM_GBS, 5),
           "full_frac_of_hbm_peak": round(gbs(floor_full, full_ms) / PEAK_HBM_GBS, 5),
           "peak_hbm_gbs": PEAK_HBM_GBS, "reps": args.reps,
           "timing": "HIP events on the context stream around the synchronous tf_mesh_extract call (median)"}
    print(f"live blocks {live}  triangles {n}")
    print(f"count only: {count_ms:.3f} ms  ({out['count_gbs']} GB/s of the floor's bytes, {100 * out['count_frac_of_hbm_peak']:.2f} % of peak)")
    print(f"full      : {full_ms:.3f} ms  ({out['full_gbs']} GB/s of the floor's bytes, {100 * out['full_frac_of_hbm_peak']:.2f} % of peak)")
    print(json.dumps(out))
    frames.free()
    tf.close()


if __name__ == "__main__":
    main()
