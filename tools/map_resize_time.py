#!/usr/bin/env python3
"""Time of a resized load on a swapping scene (DESIGN.md §5 Resized load, measurement).

Fuses the C5E hall walk of tools/map_ckpt_time.py (the seed-13 walk through the tiled hall at 640x480, 10 mm voxels,
swapping on) for --frames frames and saves the map.  The saving context has a quarter of the reference's buckets
(2^18; a swapping context's table must stay below 2^22 entries, so four times the reference's 2^20 cannot be
created), the reference's excess list and blocks.  Then, in the same run:

    resized   tf_map_load_resized into a context with four times the buckets (the reference's 2^20) and twice the blocks
    strict    tf_map_load of the same file into a context of the saving one's capacities

Every time is the host clock around the synchronous call, median of --reps after --warmup; the library's own split of
each call (tf_scene_ckpt_times; for the resized load the placement kernels are part of index_kernels) comes from a
second pair of contexts created with TFUSION_CKPT_TIMING=1.  The resized context's whole-map mesh must have the saving
context's triangle count.  One JSON line at the end; --out appends the report to a file.

    python tools/map_resize_time.py [--frames 5000] [--reps 5] [--dir DIR] [--out profiles/map_resize_time.txt]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=1000, help="frames per tf_scene_fuse_frames call")
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--swap-transfer-blocks", type=int, default=0x1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default=None, help="where the file goes (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    import topfusion_amd
    from topfusion_amd import TopFu, default_params, synth
    W, H = args.cols, args.rows
    fx, fy, cx, cy = synth.intrinsics(W, H)
    base = default_params()
    small = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=args.voxel, use_swapping=1,
                 swap_transfer_blocks=args.swap_transfer_blocks, n_buckets=base.n_buckets // 4)
    large = dict(small, n_buckets=base.n_buckets, n_blocks=2 * base.n_blocks)
    stream, R, t = synth.hall_device(args.frames, W, H, 13)
    w2c = synth.world_to_camera_rt(R, t)
    tf = TopFu(default_params(**small), device=0)
    for k in range(0, args.frames, args.batch):
        rec = tf.fuse_frames(stream.frame_ptr(k), w2c[k:min(k + args.batch, args.frames)])
        assert not rec["alloc_failed_type1"].any() and not rec["alloc_failed_type2"].any()
    stream.free()
    n_whole = tf.mesh_count(whole=True)

    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "map.tfmap")
        tf.save_map(path)
        info = topfusion_amd.map_file_info(path)
        resized, strict = TopFu(default_params(**large), device=0), TopFu(default_params(**small), device=0)
        report = {}
        resized_ms = median_ms(lambda: report.update(resized.load_map_resized(path)), args.reps, args.warmup)
        strict_ms = median_ms(lambda: strict.load_map(path), args.reps, args.warmup)
        assert resized.mesh_count(whole=True) == n_whole == strict.mesh_count(whole=True)      # both tiers are in place
        assert report["blocks"] == info["n_blocks_stored"] and report["records_carried"] + report["records_dropped"] == info["n_records"]
        resized.close()
        strict.close()
        os.environ["TFUSION_CKPT_TIMING"] = "1"
        resized_t, strict_t = TopFu(default_params(**large), device=0), TopFu(default_params(**small), device=0)
        for _ in range(args.warmup + 2):
            resized_t.load_map_resized(path)
            strict_t.load_map(path)
        split = {"resized": resized_t.scene_ckpt_times(), "strict": strict_t.scene_ckpt_times()}
        resized_t.close()
        strict_t.close()

    lines = [f"map_resize_time: C5E hall walk, {args.frames} frames fused with swapping, {W}x{H}, {args.voxel * 1000:g} mm voxels; saved from "
             f"{small['n_buckets']} buckets + {base.n_excess} excess, {base.n_blocks} blocks; loaded resized into {large['n_buckets']} buckets "
             f"+ {base.n_excess} excess, {large['n_blocks']} blocks",
             f"file: {info['file_bytes']} bytes, {info['n_records']} records, {info['n_blocks_stored']} active + {info['n_cache_blocks']} "
             f"stored blocks, {n_whole} whole-map triangles (the resized context's too)",
             "report: " + ", ".join(f"{k} {v}" for k, v in report.items())]
    out = {"tool": "map_resize_time", "frames": args.frames, "cols": W, "rows": H, "voxel": args.voxel, "file_bytes": info["file_bytes"],
           "records": info["n_records"], "from": [small["n_buckets"], base.n_excess, base.n_blocks],
           "into": [large["n_buckets"], base.n_excess, large["n_blocks"]], "report": report, "reps": args.reps,
           "resized_ms": round(resized_ms[0], 3), "resized_ms_min": round(resized_ms[1], 3), "strict_ms": round(strict_ms[0], 3),
           "strict_ms_min": round(strict_ms[1], 3),
           "timing": "host clock around the synchronous calls (median); the split from contexts with TFUSION_CKPT_TIMING=1 (HIP events around the kernels)"}
    for name, call, whole in (("resized", "tf_map_load_resized", resized_ms), ("strict", "tf_map_load", strict_ms)):
        s = split[name]
        out.update({f"{name}_{k}": round(v, 4) for k, v in s.items()})
        lines.append(f"{name} ({call}): {whole[0]:.2f} ms (min {whole[1]:.2f})  -- a call with timed kernels {s['call']:.2f} ms: index kernels "
                     f"{s['index_kernels']:.3f}{' (placement, apply, visible list, block grid)' if name == 'resized' else ''}, block kernels "
                     f"{s['block_kernels']:.3f}, copies {s['copies']:.2f}, validation {s['check']:.3f}, file {s['file']:.2f}")
    lines.append(f"the resized load is {resized_ms[0] / strict_ms[0]:.3f} x the strict one; its index kernels are "
                 f"{split['resized']['index_kernels'] / max(split['resized']['block_kernels'], 1e-9):.2f} x its block kernels")
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text)
    tf.close()


if __name__ == "__main__":
    main()
