#!/usr/bin/env python3
"""Times of the free views' whole reading (TF_VIEW_WHOLE, DESIGN.md §5 Free views) beside the resident one; writes
profiles/view_whole_time.txt.

Every time is a host clock around a synchronous C-ABI call (each ends in a wait for the context stream): the median
of --reps calls after --warmup, with the minimum beside it -- tools/view_time.py's method.  Timed under both
readings: tf_view_find_visible (the scan) and tf_view_render (scan, expected depths, raycast, greyscale shading; the
time includes View.render's download of the image).

Scenes:
  C5E  the hall walk after --hall-frames engine-level frames with the swapping engine on (10 mm voxels): a few
       hundred blocks resident, the rest of the map in the GlobalCache.  Poses: the tracked one (the last frame's),
       an old one (the middle frame's: where the camera was, all of it stored by now) and an overview (the middle of
       the camera path, the middle frame's orientation, half the focal length), each at 640x480 with a
       max_render_blocks that holds its tiles.
  C2   the orbit after --frames tracked frames, its map uploaded into a swapping context: nothing is stored, so the
       whole reading's kernels run over resident blocks only -- the price of the whole instantiation.

    python tools/view_whole_time.py [--frames 300] [--hall-frames 5000] [--reps 30] [--warmup 5] [--bench-lines FILE]

--bench-lines FILE: JSON lines of bench.py C2 runs, each tagged {"lib": "parent" | "this", ...}, appended as the
"tracker unchanged" table.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from view_time import rt34, timed   # noqa: E402

TILE_CAP = 1 << 22


def both_readings(tag, tf, c2w, intr, reps, warmup, cols=640, rows=480):
    from oracle import oracle as O
    w2c = O.rigid_inv(c2w)
    out = []
    for whole in (False, True):
        with tf.view(cols, rows, max_render_blocks=TILE_CAP, whole=whole) as v:
            v.render(c2w, 0, intr)
            st = v.stats()
            hits = int((v.raycast_result()[..., 3] > 0).sum())
            s_med, s_lo = timed(lambda: v.find_visible(w2c, intr), reps, warmup)
            r_med, r_lo = timed(lambda: v.render(c2w, 0, intr), reps, warmup)
        out.append(f"{tag:<22} {'whole' if whole else 'resident':<8} visible {st['noVisibleEntries']:>7}  tiles {st['noTotalBlocks']:>8}  "
                   f"hit pixels {hits:>7}  find_visible {s_med:8.4f} ms (min {s_lo:.4f})  render {r_med:8.4f} ms (min {r_lo:.4f})")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--hall-frames", type=int, default=5000)
    ap.add_argument("--swap-transfer-blocks", type=int, default=0x1000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_whole_time.txt"))
    args = ap.parse_args()
    from topfusion_amd import TopFu, default_params, synth, _lib as L
    lines = ["free views, the whole reading: tools/view_whole_time.py  (times: host clock around synchronous calls, median of "
             f"{args.reps} after {args.warmup} warm-up calls; render includes the image's download)", ""]
    W, H = 640, 480
    fx, fy, cx, cy = synth.intrinsics(W, H)

    # ---- C5E with swapping
    n = args.hall_frames
    stream, R, t = synth.hall_device(n, W, H, 13)
    w2c_all = synth.world_to_camera_rt(R, t)
    tf = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=0.01, use_swapping=1,
                              swap_transfer_blocks=args.swap_transfer_blocks), device=0)
    for b0 in range(0, n, 1000):
        tf.fuse_frames(stream.frame_ptr(b0), w2c_all[b0:min(n, b0 + 1000)])
    h, state, flags = tf.hash(), tf.swap_state(), tf.swap_stored_flags()
    p, f = h["ptr"], flags != 0
    lines.append(f"C5E hall walk after {n} frames with swapping, 640x480, 10 mm, {tf.n_total} hash entries: resident {int((p >= 0).sum())} "
                 f"(pending merge {int(((p >= 0) & f & (state != 2)).sum())}), stored only {int(((p == -1) & f).sum())}")

    def pose(k):
        m = np.zeros((3, 4), np.float32)
        m[:, :3], m[:, 3] = R[k], t[k]
        return m
    over = pose(n // 2)
    over[:, 3] = np.asarray(t, np.float64).mean(axis=0)
    wide = np.array([fx / 2, fy / 2, cx, cy], np.float32)
    lines += both_readings("C5E tracked pose", tf, pose(n - 1), None, args.reps, args.warmup)
    lines += both_readings("C5E old pose", tf, pose(n // 2), None, args.reps, args.warmup)
    lines += both_readings("C5E overview (f / 2)", tf, over, wide, args.reps, args.warmup)
    stream.free()
    tf.close()
    lines.append("")

    # ---- C2: nothing stored, the whole kernels over resident blocks
    tf = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy), device=0)
    frames = synth.orbit_device(args.frames, W, H, seed=7)
    ok = tf.process_frames(frames.ptr, args.frames)
    c2w = rt34(tf.getCameraPose())
    hash_, vba = tf.hash(), tf.vba()
    tf.close()
    sw = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, use_swapping=1), device=0)
    sw.upload(L.TF_BUF_HASH, hash_)
    sw.upload(L.TF_BUF_VBA, vba)
    lines.append(f"C2 orbit after {args.frames} frames ({int(ok.sum())} tracked), 640x480, 5 mm, its map in a swapping context with nothing "
                 f"stored; live blocks {int((hash_['ptr'] >= 0).sum())}")
    lines += both_readings("C2 tracked pose", sw, c2w, None, args.reps, args.warmup)
    lines += both_readings("C2 tracked pose 1280", sw, c2w, np.array([2 * fx, 2 * fy, 2 * cx, 2 * cy], np.float32), args.reps, args.warmup, 1280, 960)
    sw.close()
    lines.append("")

    if args.bench_lines and os.path.exists(args.bench_lines):
        lines.append("tracker unchanged: bench.py --gpus 1 --config C2 --no-cpu-baseline (else its own defaults), three runs of this commit and three of the "
                     "parent commit's library, alternating, in one session")
        by = {}
        for ln in open(args.bench_lines):
            ln = ln.strip()
            if ln.startswith("{"):
                r = json.loads(ln)
                by.setdefault(r.get("lib", "?"), []).append(r)
        for lib, rs in sorted(by.items()):
            vals = [r.get("value") for r in rs]
            lines.append(f"  {lib:<7} {rs[0].get('metric', 'value')} ({rs[0].get('unit', '')}): " + "  ".join(f"{x:.2f}" for x in vals) +
                         f"   range [{min(vals):.2f}, {max(vals):.2f}]")
        if len(by) == 2:
            (_, ra), (_, rb) = sorted(by.items())
            va, vb = [r["value"] for r in ra], [r["value"] for r in rb]
            lines.append("  the two ranges " + ("overlap" if max(min(va), min(vb)) <= min(max(va), max(vb)) else "DO NOT overlap"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
