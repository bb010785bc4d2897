#!/usr/bin/env python3
"""Times of the scene queries (tf_scene_query / tf_scene_slice, DESIGN.md §5 Scene queries) on the bench's scenes;
writes profiles/scene_query_time.txt.

Every time is a host clock around a synchronous C-ABI call over device buffers allocated before (each call ends in a
wait for the context stream): the median of --reps calls after --warmup, with the minimum beside it.  No host copy of
points or results is inside a timed call.

  per output group (one kernel each): the four SDF reads together, sdf alone, the gradient, the colour;
  points: 2^20 taken from the raycast result of the tracked pose (coherent: neighbours in the array are neighbours
          on the surface), and 2^20 hashed uniformly over the bounding box of the live blocks (incoherent);
  slices: 640x480 and 1280x960 through the middle of that box;
  scale:  tf_view_raycast at 640x480 from the tracked pose on the same context.

Scenes: the C2 orbit after --frames tracked frames (its map copied into a voxel_rgb context for the colour kernel: the
colour plane's values do not matter to the time); the C5E hall walk after --hall-frames engine-level frames with
swapping (10 mm voxels), both readings.

    python tools/scene_query_time.py [--frames 300] [--hall-frames 5000] [--reps 30] [--warmup 5] [--bench-lines FILE]

--bench-lines FILE: JSON lines of bench.py C2 runs, each tagged {"lib": "parent" | "this", ...}, appended as the
"tracker unchanged" table.
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

N_POINTS = 1 << 20
GROUPS = (("four SDF reads", ("sdf_nearest", "entry", "sdf", "confidence")), ("sdf alone", ("sdf",)), ("gradient", ("normal",)),
          ("colour", ("colour",)))
BYTES = dict(sdf_nearest=4, entry=4, sdf=4, confidence=4, normal=12, colour=4)


def timed(call, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        t = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            ms.append(t)
    return float(np.median(ms)), float(np.min(ms))


def _mix32(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    for s, m in ((16, 0x7FEB352D), (15, 0x846CA68B)):
        x ^= x >> np.uint64(s)
        x = (x * np.uint64(m)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(16))


class DevBufs:
    """Device memory for one batch: the points and every output, through the library's own HIP runtime."""
    def __init__(self, L, n):
        self.L, self.hip, self.n = L, L.hip_runtime(), n
        self.ptrs = {}
        for k, b in dict(BYTES, points=12).items():
            p = ctypes.c_void_p()
            if self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(n * b)) != 0:
                raise RuntimeError("hipMalloc")
            self.ptrs[k] = p

    def put_points(self, pts):
        a = np.ascontiguousarray(pts, np.float32)
        assert a.shape == (self.n, 3)
        assert self.hip.hipMemcpy(self.ptrs["points"], a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1) == 0

    def out(self, names):
        qo = self.L.TfQueryOut()
        for k in names:
            setattr(qo, k, self.ptrs[k].value)
        return qo

    def free(self):
        for p in self.ptrs.values():
            self.hip.hipFree(p)


def query_lines(tag, tf, bufs, whole, reps, warmup, groups, slice_args=None):
    L = bufs.L
    lib = L.load()
    reading = L.TF_VIEW_WHOLE if whole else L.TF_VIEW_RESIDENT
    out = []
    for name, outs in groups:
        qo = bufs.out(outs)
        if slice_args is None:
            n = bufs.n
            call = lambda: L.check(lib.tf_scene_query(tf._h, bufs.ptrs["points"], n, L.TF_QUERY_VOXELS, reading, ctypes.byref(qo)), "tf_scene_query")
        else:
            o, u, v, cols, rows = slice_args
            n = cols * rows
            f = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            call = lambda: L.check(lib.tf_scene_slice(tf._h, f(o), f(u), f(v), cols, rows, L.TF_QUERY_VOXELS, reading, ctypes.byref(qo)), "tf_scene_slice")
        med, lo = timed(call, reps, warmup)
        wr = n * sum(BYTES[k] for k in outs)
        out.append(f"  {tag:<44} {name:<15} {n:>8} points  {med:8.4f} ms (min {lo:.4f})  {n / (med * 1e-3) / 1e6:9.1f} Mpoints/s  "
                   f"{wr / 1e6:6.1f} MB written")
    return out


def scene_points(tf, c2w):
    """(coherent, incoherent, box lo, box hi) in voxel units: the raycast result's hits tiled to N_POINTS, and points
    hashed uniformly over the bounding box of the live blocks."""
    h = tf.hash()
    live = h[h["ptr"] >= 0]
    lo = np.array([live["x"].min(), live["y"].min(), live["z"].min()], np.float64) * 8
    hi = (np.array([live["x"].max(), live["y"].max(), live["z"].max()], np.float64) + 1) * 8
    with tf.view() as v:
        from oracle import oracle as O
        v.find_visible(O.rigid_inv(c2w))
        v.expected_depths(O.rigid_inv(c2w))
        v.raycast(c2w)
        ray = v.raycast_result().reshape(-1, 4)
    hits = ray[ray[:, 3] > 0][:, :3]
    assert len(hits) > 1000, "the raycast found no surface"
    coherent = np.resize(hits, (N_POINTS, 3)).astype(np.float32)
    i = np.arange(N_POINTS, dtype=np.uint64)
    r = np.stack([_mix32(i * np.uint64(3) + np.uint64(k) + np.uint64(0x9E3779B9)) for k in range(3)], -1).astype(np.float64) / 2.0 ** 32
    incoherent = (lo + r * (hi - lo)).astype(np.float32)
    return coherent, incoherent, lo, hi


def slice_of(lo, hi, cols, rows):
    mid = (lo + hi) / 2
    u = np.array([(hi[0] - lo[0]) / cols, 0, 0], np.float32)
    v = np.array([0, (hi[1] - lo[1]) / rows, 0], np.float32)
    return np.array([lo[0], lo[1], mid[2]], np.float32), u, v, cols, rows


def raycast_line(tag, tf, c2w, reps, warmup):
    from oracle import oracle as O
    with tf.view() as v:
        v.find_visible(O.rigid_inv(c2w))
        v.expected_depths(O.rigid_inv(c2w))
        med, lo = timed(lambda: v.raycast(c2w), reps, warmup)
    return f"  {tag:<44} {'tf_view_raycast':<15} {tf.W * tf.H:>8} rays    {med:8.4f} ms (min {lo:.4f})   (for scale)"


def rt34(m):
    return np.ascontiguousarray(np.asarray(m, np.float32)[:3, :4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--hall-frames", type=int, default=5000)
    ap.add_argument("--swap-transfer-blocks", type=int, default=0x1000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_query_time.txt"))
    args = ap.parse_args()
    from topfusion_amd import TopFu, default_params, synth, _lib as L
    lines = ["scene queries: tools/scene_query_time.py  (times: host clock around synchronous calls over device buffers, median of "
             f"{args.reps} after {args.warmup} warm-up calls; voxel units)", ""]
    W, H = 640, 480
    fx, fy, cx, cy = synth.intrinsics(W, H)
    bufs = DevBufs(L, N_POINTS)
    big = DevBufs(L, 1280 * 960)

    # ---- C2: the orbit, tracked; its map in a voxel_rgb context
    tf = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy), device=0)
    frames = synth.orbit_device(args.frames, W, H, seed=7)
    ok = tf.process_frames(frames.ptr, args.frames)
    c2w = rt34(tf.getCameraPose())
    hash_, vba = tf.hash(), tf.vba()
    tf.close()
    frames.free() if hasattr(frames, "free") else None
    tf = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxel_rgb=1), device=0)
    tf.upload(L.TF_BUF_HASH, hash_)
    tf.upload(L.TF_BUF_VBA, vba)
    lines.append(f"C2 orbit after {args.frames} frames ({int(ok.sum())} tracked), 640x480, 5 mm; live blocks {int((hash_['ptr'] >= 0).sum())}; "
                 "the map in a voxel_rgb context (zero colour plane)")
    coherent, incoherent, lo, hi = scene_points(tf, c2w)
    for tag, pts in (("C2 coherent (raycast result)", coherent), ("C2 incoherent (uniform over the box)", incoherent)):
        bufs.put_points(pts)
        lines += query_lines(tag, tf, bufs, False, args.reps, args.warmup, GROUPS)
    for cols, rows in ((640, 480), (1280, 960)):
        lines += query_lines(f"C2 slice {cols}x{rows}", tf, big, False, args.reps, args.warmup, GROUPS, slice_of(lo, hi, cols, rows))
    lines.append(raycast_line("C2 tracked pose 640x480", tf, c2w, args.reps, args.warmup))
    tf.close()
    lines.append("")

    # ---- C5E with swapping, both readings
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
    c2w = np.zeros((3, 4), np.float32)
    c2w[:, :3], c2w[:, 3] = R[n - 1], t[n - 1]
    coherent, incoherent, lo, hi = scene_points(tf, c2w)
    groups = GROUPS[:3]                                   # a swapping scene has no colour plane
    for whole in (False, True):
        rd = "whole" if whole else "resident"
        for tag, pts in ((f"C5E coherent, {rd}", coherent), (f"C5E incoherent, {rd}", incoherent)):
            bufs.put_points(pts)
            lines += query_lines(tag, tf, bufs, whole, args.reps, args.warmup, groups)
        lines += query_lines(f"C5E slice 640x480, {rd}", tf, big, whole, args.reps, args.warmup, groups, slice_of(lo, hi, 640, 480))
    lines.append(raycast_line("C5E last pose 640x480 (resident)", tf, c2w, args.reps, args.warmup))
    stream.free()
    tf.close()
    bufs.free()
    big.free()
    lines.append("")

    if args.bench_lines and os.path.exists(args.bench_lines):
        lines.append("tracker unchanged: bench.py --gpus 1 --config C2 --no-cpu-baseline, three runs of this commit and three of the "
                     "parent commit's library, alternating, in one session")
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
