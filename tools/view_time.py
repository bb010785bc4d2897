#!/usr/bin/env python3
"""Times of the free views (tf_view_*, DESIGN.md §5 Free views) on the bench's scenes; writes profiles/view_time.txt.

Every time is a host clock around a synchronous C-ABI call (each ends in a wait for the context stream): the
median of --reps calls after --warmup, with the minimum beside it.

  scan    tf_view_find_visible: FindVisibleBlocks over the whole hash.  Bytes: 16 B per entry read by the count
          pass, 8 B per 64 entries of kept ballots written and read again, 4 B per visible entry written;
          the rate those bytes reach in the call's time, beside the HBM peak bench.py uses.  The call is two
          launches and a prefix, a 16-byte read-back the host waits for, then the emit launch: its time is
          latency as much as traffic, which the table of synthetic fills (1 %, 10 %, 50 % live) shows.
  render  tf_view_render at the tracked pose and size, beside tf_vis_expected_depths + tf_vis_render_image on
          the same context (the same raycast and shading; the view adds the scan and carries the longer list);
          then at 1280x960 and at 160x120.

Scenes: the C2 orbit after --frames tracked frames; the C5E hall walk after --hall-frames engine-level frames
(10 mm voxels, the VBA saturated); a context of C3's capacities (2^21 - 1 blocks, 2^22 + 2^20 entries) whose table
is filled synthetically, for the scan alone.

    python tools/view_time.py [--frames 300] [--hall-frames 5000] [--reps 30] [--warmup 5] [--bench-lines FILE]

--bench-lines FILE: JSON lines of bench.py C2 runs, each tagged {"lib": "parent" | "this", ...}, appended as the
"tracker unchanged" table.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM_GBS = 8000.0        # MI355X HBM3E peak, as bench.py takes it


def timed(call, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        t = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            ms.append(t)
    return float(np.median(ms)), float(np.min(ms))


def rt34(m):
    return np.ascontiguousarray(np.asarray(m, np.float32)[:3, :4])


def scan_line(tag, tf, view, w2c, reps, warmup, intr=None):
    n = view.find_visible(w2c, intr)
    med, lo = timed(lambda: view.find_visible(w2c, intr), reps, warmup)
    nbytes = 16 * tf.n_total + 2 * 8 * ((tf.n_total + 63) // 64) + 4 * n
    gbs = nbytes / (med * 1e-3) / 1e9
    return (f"{tag:<34} entries {tf.n_total:>8}  visible {n:>8}  {med:8.4f} ms (min {lo:.4f})  {nbytes / 1e6:8.2f} MB  "
            f"{gbs:8.1f} GB/s  {100 * gbs / PEAK_HBM_GBS:5.2f} % of {PEAK_HBM_GBS:.0f} GB/s"), dict(tag=tag, n=n, ms=med, ms_min=lo, bytes=nbytes)


def render_lines(tag, tf, c2w, w2c, reps, warmup, sizes):
    from topfusion_amd import _lib as L
    import ctypes
    lib = L.load()
    out = []
    p = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(ctypes.c_void_p)

    def tracker_path():
        L.check(lib.tf_vis_expected_depths(tf._h, None, p(w2c)), "tf_vis_expected_depths")
        L.check(lib.tf_vis_render_image(tf._h, None, p(c2w), 0, 1, None, 0), "tf_vis_render_image")
    med, lo = timed(tracker_path, reps, warmup)
    nv = tf.stats()["noVisibleEntries"]
    out.append(f"{tag} tf_vis_expected_depths + tf_vis_render_image {tf.W}x{tf.H} (tracker's list, {nv} entries): {med:.4f} ms (min {lo:.4f})")
    for cols, rows in sizes:
        s = cols / tf.W
        intr = np.array([tf.params_.fx * s, tf.params_.fy * s, tf.params_.cx * s, tf.params_.cy * s], np.float32)
        with tf.view(cols, rows) as v:
            med, lo = timed(lambda: v.render(c2w, 0, None if cols == tf.W else intr), reps, warmup)
            st = v.stats()
        out.append(f"{tag} tf_view_render {cols}x{rows} ({st['noVisibleEntries']} entries, {st['noTotalBlocks']} tiles): "
                   f"{med:.4f} ms (min {lo:.4f})  [includes the (rows, cols, 4) download of View.render]")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--hall-frames", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_time.txt"))
    args = ap.parse_args()
    from topfusion_amd import TopFu, default_params, synth
    from oracle import oracle as O
    lines = ["free views: tools/view_time.py  (times: host clock around synchronous calls, median of "
             f"{args.reps} after {args.warmup} warm-up calls)", ""]
    sizes = [(640, 480), (1280, 960), (160, 120)]

    # ---- C2: the orbit, tracked
    W, H = 640, 480
    fx, fy, cx, cy = synth.intrinsics(W, H)
    tf = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy), device=0)
    frames = synth.orbit_device(args.frames, W, H, seed=7)
    ok = tf.process_frames(frames.ptr, args.frames)
    c2w = rt34(tf.getCameraPose())
    w2c = O.rigid_inv(c2w)
    lines.append(f"C2 orbit after {args.frames} frames ({int(ok.sum())} tracked), 640x480, 5 mm; live blocks {int((tf.hash()['ptr'] >= 0).sum())}")
    with tf.view() as v:
        l, _ = scan_line("scan C2 (tracked pose, 640x480)", tf, v, w2c, args.reps, args.warmup)
    lines.append(l)
    lines += render_lines("render C2", tf, c2w, w2c, args.reps, args.warmup, sizes)
    frames.free() if hasattr(frames, "free") else None
    tf.close()
    lines.append("")

    # ---- C5E: the hall walk, engine level
    n = args.hall_frames
    stream, R, t = synth.hall_device(n, W, H, 13)
    w2c_all = synth.world_to_camera_rt(R, t)
    tf = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=0.01), device=0)
    for b0 in range(0, n, 1000):
        b1 = min(n, b0 + 1000)
        tf.fuse_frames(stream.frame_ptr(b0), w2c_all[b0:b1])
    c2w = np.zeros((3, 4), np.float32)
    c2w[:, :3], c2w[:, 3] = R[n - 1], t[n - 1]
    w2c = O.rigid_inv(c2w)
    lines.append(f"C5E hall walk after {n} frames, 640x480, 10 mm; live blocks {int((tf.hash()['ptr'] >= 0).sum())} of {tf.params_.n_blocks}")
    with tf.view() as v:
        l, _ = scan_line("scan C5E (last pose, 640x480)", tf, v, w2c, args.reps, args.warmup)
    lines.append(l)
    lines += render_lines("render C5E", tf, c2w, w2c, args.reps, args.warmup, sizes)
    tf.close()
    lines.append("")

    # ---- a 2^21-block context: the scan alone over a synthetic table
    from topfusion_amd.topfu import HASH_DTYPE
    from topfusion_amd import _lib as L
    cap = dict(n_buckets=1 << 22, n_excess=1 << 20, n_blocks=(1 << 21) - 1, vis_capacity=1 << 21, max_render_blocks=1 << 20)
    tf = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=0.002, **cap), device=0)
    lines.append(f"2^21-block context ({tf.n_total} entries, {16 * tf.n_total / 1e6:.1f} MB of table), synthetic fills: live entries at "
                 "random indices, positions uniform in a box of 3.3 x 3.3 x 2.6 m in front of the camera")
    rng = np.random.default_rng(5)
    I = np.eye(4, dtype=np.float32)[:3]
    for frac in (0.0, 0.01, 0.10, 0.50):
        h = np.zeros(tf.n_total, HASH_DTYPE)
        h["ptr"] = -2
        m = int(frac * tf.n_total)
        if m:
            idx = rng.choice(tf.n_total, m, replace=False)
            h["x"][idx] = rng.integers(-100, 100, m)
            h["y"][idx] = rng.integers(-100, 100, m)
            h["z"][idx] = rng.integers(20, 180, m)
            h["ptr"][idx] = np.arange(m) % tf.params_.n_blocks
        tf.upload(L.TF_BUF_HASH, h)
        with tf.view() as v:
            l, _ = scan_line(f"scan 2^21-block, {100 * frac:.0f} % live", tf, v, I, args.reps, args.warmup)
        lines.append(l)
    tf.close()
    lines.append("")

    if args.bench_lines and os.path.exists(args.bench_lines):
        lines.append("tracker unchanged: bench.py --gpus 1 --config C2 (its own defaults: --steps 20 --warmup 5), three runs of this "
                     "commit and three of the parent commit's library, alternating, in one session")
        by = {}
        for ln in open(args.bench_lines):
            ln = ln.strip()
            if not ln.startswith("{"):
                continue
            r = json.loads(ln)
            by.setdefault(r.get("lib", "?"), []).append(r)
        for lib, rs in sorted(by.items()):
            vals = [r.get("value") for r in rs]
            lines.append(f"  {lib:<7} {rs[0].get('metric', 'value')} ({rs[0].get('unit', '')}): " + "  ".join(f"{x:.2f}" for x in vals) +
                         f"   range [{min(vals):.2f}, {max(vals):.2f}]")
        if len(by) == 2:
            (a, ra), (b, rb) = sorted(by.items())
            va, vb = [r["value"] for r in ra], [r["value"] for r in rb]
            lines.append("  the two ranges " + ("overlap" if max(min(va), min(vb)) <= min(max(va), max(vb)) else "DO NOT overlap"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
