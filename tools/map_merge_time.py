#!/usr/bin/env python3
"""Time of a map merge on the bench's scene (DESIGN.md §5 Map merge, measurement).

Fuses the C2 orbit (bench.py's flagship workload: the synthetic room + sphere orbit at 640x480, 5 mm) for one
32-frame window and saves the scene.  Then, in the same run, tf_map_merge of that file into

    reset     a context after ResetScene: every record is inserted
    same      the context that holds the saved scene: every record combines
    shifted   the same with a block offset of (1, 0, 0): part combines, part is inserted

each beside tf_scene_load of the file into a context of its own.  Before every timed merge the target is put back
(reset, or a load of the file: untimed).  Every time is the host clock around the synchronous call, median of --reps
after --warmup; the library's own split of each call (tf_scene_ckpt_times: the placement kernels in index_kernels,
the copy / combine kernel in block_kernels) comes from contexts created with TFUSION_CKPT_TIMING=1.  One JSON line at
the end; --out appends the report to a file.

    python tools/map_merge_time.py [--frames 32] [--reps 7] [--dir DIR] [--out profiles/map_merge_time.txt]
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

CASES = (("reset", (0, 0, 0)), ("same", (0, 0, 0)), ("shifted", (1, 0, 0)))


def median_ms(fn, reps, warmup, before=None):
    ms = []
    for i in range(warmup + reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the file goes (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    import topfusion_amd
    from topfusion_amd import TopFu, default_params, synth
    W, H = args.cols, args.rows
    fx, fy, cx, cy = synth.intrinsics(W, H)
    params = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy)
    tf = TopFu(default_params(**params), device=0)
    frames = synth.orbit_device(args.frames, W, H, seed=7)
    tf.process_frames(frames.ptr, args.frames)
    frames.free()

    def run(timed):
        """{case: (report, (median, min) ms, split)} and the load's, on contexts created now."""
        g, loader = TopFu(default_params(**params), device=0), TopFu(default_params(**params), device=0)
        out = {}
        for name, off in CASES:
            report = {}
            put_back = g.reset if name == "reset" else (lambda: g.load_scene(path))
            ms = median_ms(lambda: report.update(g.merge_map(path, off)), args.reps, args.warmup, put_back)
            out[name] = (dict(report), ms, g.scene_ckpt_times() if timed else None)
        ms = median_ms(lambda: loader.load_scene(path), args.reps, args.warmup)
        out["load"] = (None, ms, loader.scene_ckpt_times() if timed else None)
        g.close()
        loader.close()
        return out

    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "scene.tfscene")
        tf.save_scene(path)
        info = topfusion_amd.scene_file_info(path)
        plain = run(False)
        os.environ["TFUSION_CKPT_TIMING"] = "1"
        timed = run(True)
        del os.environ["TFUSION_CKPT_TIMING"]

    n = info["n_blocks_stored"]
    assert plain["reset"][0]["records_inserted"] == n and plain["same"][0]["records_combined"] == n
    assert plain["shifted"][0]["records_combined"] + plain["shifted"][0]["records_inserted"] == n
    lines = [f"map_merge_time: C2 orbit, {args.frames} frames tracked, {W}x{H}, 5 mm voxels; the scene saved and merged into a reset "
             f"context, into the context that holds it, and into that one a block further along x",
             f"file: {info['file_bytes']} bytes, {info['n_records']} records, {n} blocks"]
    out = {"tool": "map_merge_time", "frames": args.frames, "cols": W, "rows": H, "file_bytes": info["file_bytes"],
           "records": info["n_records"], "blocks": n, "reps": args.reps,
           "timing": "host clock around the synchronous calls (median); the split from contexts with TFUSION_CKPT_TIMING=1 (HIP events around the kernels)"}
    load_ms = plain["load"][1][0]
    for name in ("reset", "same", "shifted", "load"):
        report, ms, _ = plain[name]
        s = timed[name][2]
        call = "tf_scene_load" if name == "load" else "tf_map_merge"
        if report:
            lines.append(f"{name} report: " + ", ".join(f"{k} {v}" for k, v in report.items()))
            out[f"{name}_report"] = report
        gbs = s["block_kernel_bytes"] / max(s["block_kernels"], 1e-9) / 1e6
        lines.append(f"{name} ({call}): {ms[0]:.2f} ms (min {ms[1]:.2f}), {ms[0] / load_ms:.3f} x the load  -- a call with timed kernels "
                     f"{s['call']:.2f} ms: index kernels {s['index_kernels']:.3f}, block kernels {s['block_kernels']:.3f} "
                     f"({gbs:.0f} GB/s read + written), copies {s['copies']:.2f}, validation {s['check']:.3f}, file {s['file']:.2f}")
        out[f"{name}_ms"], out[f"{name}_ms_min"] = round(ms[0], 3), round(ms[1], 3)
        out.update({f"{name}_{k}": round(v, 4) for k, v in s.items()})
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text)
    tf.close()


if __name__ == "__main__":
    main()
