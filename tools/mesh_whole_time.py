#!/usr/bin/env python3
"""Time of the whole-map mesh extraction on a swapping scene (DESIGN.md §Mesh extraction, the whole map).

Fuses the C5E hall walk (bench.py --config C5E --swapping: the seed-13 walk through the tiled hall at
640x480, 10 mm voxels, reference capacities) for --frames frames through tf_scene_fuse_frames with the
swapping engine on, so that a few hundred blocks stay resident and the rest of the map lies in the
GlobalCache.  Then times, with HIP events recorded on the context stream around the call (tools/mesh_time.py's
method: median of --reps after --warmup), the resident reading (tf_mesh_extract) and the whole reading
(tf_mesh_extract_whole), each count-only and full (positions), and the whole reading with normals.

Per measurement: the resolving entries by row of the resolution table (active / combined / stored), the
triangles, the bytes written, the milliseconds, and the bytes per second achieved against the floor

    2 passes (count, emit; 1 for count-only) x resolving blocks x 2 KiB + 36 B per triangle (72 with normals)

(a combined block reads two tiers: it counts twice).  One JSON line at the end; --out appends the report to a file.

    python tools/mesh_whole_time.py [--frames 5000] [--reps 20] [--warmup 3] [--out profiles/mesh_whole_time.txt]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM_GBS = 8000.0        # MI355X HBM3E peak, as bench.py takes it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=1000, help="frames per tf_scene_fuse_frames call")
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--swap-transfer-blocks", type=int, default=0x1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    from topfusion_amd import TopFu, default_params, synth, _lib as L
    W, H = args.cols, args.rows
    fx, fy, cx, cy = synth.intrinsics(W, H)
    t0 = time.perf_counter()
    stream, R, t = synth.hall_device(args.frames, W, H, 13)
    w2c = synth.world_to_camera_rt(R, t)
    tf = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=args.voxel, use_swapping=1,
                              swap_transfer_blocks=args.swap_transfer_blocks), device=0)
    for k in range(0, args.frames, args.batch):
        tf.fuse_frames(stream.frame_ptr(k), w2c[k:min(k + args.batch, args.frames)])
    h, state, flags = tf.hash(), tf.swap_state(), tf.swap_stored_flags()
    fuse_s = time.perf_counter() - t0
    p, f = h["ptr"], flags != 0
    rows = {"active": int(((p >= 0) & (~f | (state == 2))).sum()), "combined": int(((p >= 0) & f & (state != 2)).sum()),
            "stored": int(((p == -1) & f).sum())}
    resident_blocks = int((p >= 0).sum())
    whole_blocks = rows["active"] + 2 * rows["combined"] + rows["stored"]      # block reads of one pass
    n_res, n_whole = tf.mesh_count(), tf.mesh_count(whole=True)

    lib, hip = L.load(), L.hip_runtime()
    hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventDestroy.argtypes = [ctypes.c_void_p]
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    cstream = ctypes.c_void_p(tf.stream())
    dev_t, dev_n = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev_t), max(16, n_whole * 36)) == 0, "hipMalloc"
    assert hip.hipMalloc(ctypes.byref(dev_n), max(16, n_whole * 36)) == 0, "hipMalloc"

    def timed_call(call, expect):
        got = ctypes.c_longlong()
        ms = []
        for i in range(args.warmup + args.reps):
            assert hip.hipEventRecord(e0, cstream) == 0
            call(got)
            assert hip.hipEventRecord(e1, cstream) == 0 and hip.hipEventSynchronize(e1) == 0
            el = ctypes.c_float()
            assert hip.hipEventElapsedTime(ctypes.byref(el), e0, e1) == 0
            assert got.value == expect, (got.value, expect)
            if i >= args.warmup:
                ms.append(el.value)
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    resident = lambda buf, cap: (lambda got: L.check(lib.tf_mesh_extract(tf._h, buf, cap, ctypes.byref(got)), "tf_mesh_extract"))
    whole = lambda bt, bn, cap: (lambda got: L.check(lib.tf_mesh_extract_whole(tf._h, bt, bn, cap, ctypes.byref(got)), "tf_mesh_extract_whole"))
    runs = [("resident count only", resident(None, 0), n_res, 1, resident_blocks, 0),
            ("resident full      ", resident(dev_t, n_res), n_res, 2, resident_blocks, 36),
            ("whole count only   ", whole(None, None, 0), n_whole, 1, whole_blocks, 0),
            ("whole full         ", whole(dev_t, None, n_whole), n_whole, 2, whole_blocks, 36),
            ("whole full, normals", whole(dev_t, dev_n, n_whole), n_whole, 2, whole_blocks, 72)]
    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9
    lines = [f"mesh_whole_time: C5E hall walk, {args.frames} frames fused with swapping in {fuse_s:.1f} s (render + fuse), {W}x{H}, "
             f"{args.voxel * 1000:g} mm voxels, {tf.n_total} hash entries, {tf.params().n_blocks} VBA blocks, "
             f"<= {args.swap_transfer_blocks} blocks per transfer",
             f"resolving entries: active {rows['active']}  combined {rows['combined']}  stored {rows['stored']}   "
             f"(resident reading: {resident_blocks} blocks)",
             f"triangles: resident {n_res}  whole {n_whole}"]
    out = {"tool": "mesh_whole_time", "frames": args.frames, "cols": W, "rows": H, "voxel": args.voxel, "hash_entries": tf.n_total,
           "entries": rows, "resident_blocks": resident_blocks, "triangles_resident": n_res, "triangles_whole": n_whole,
           "reps": args.reps, "peak_hbm_gbs": PEAK_HBM_GBS, "runs": {},
           "timing": "HIP events on the context stream around the synchronous call (median, min, max)"}
    for label, call, n, passes, blocks, per_tri in runs:
        ms, mn, mx = timed_call(call, n)
        floor, written = passes * blocks * 2048 + per_tri * n, per_tri * n
        g = gbs(floor, ms)
        lines.append(f"{label}: {n} triangles, {written} B written, {ms:.3f} ms (min {mn:.3f}, max {mx:.3f}); floor {floor} B -> "
                     f"{g:.1f} GB/s, {100 * g / PEAK_HBM_GBS:.2f} % of peak")
        out["runs"][label.strip()] = {"triangles": n, "bytes_written": written, "ms": round(ms, 4), "ms_min": round(mn, 4),
                                      "ms_max": round(mx, 4), "floor_bytes": floor, "gbs": round(g, 2)}
    for d in (dev_t, dev_n):
        hip.hipFree(d)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text)
    stream.free()
    tf.close()


if __name__ == "__main__":
    main()
