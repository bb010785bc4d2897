#!/usr/bin/env python3
"""Size and time of map checkpoints on a swapping scene (DESIGN.md §5 Map checkpoints, measurement).

Fuses the C5E hall walk (bench.py --config C5E --swapping: the seed-13 walk through the tiled hall at 640x480,
10 mm voxels, reference capacities) for --frames frames through tf_scene_fuse_frames with the swapping engine
on, as tools/mesh_whole_time.py does: a few hundred blocks stay resident, the rest of the map lies in the
GlobalCache.  Then, in the same run and into the same directory:

    save       tf_map_save of that context              load       tf_map_load into a second context
    swap_save  tf_swap_save of the same context: the only file such a scene could produce before (n_total x 2049
               bytes whatever is stored; no hash, lists, counters, states, pose or maps: nothing resumes from it)
    swap_load  tf_swap_load of that file into the second context

The file's size is checked against the formula 304 + 24 R + 2048 (b + s) + 4 (V + A + E) + M with the counts of
the header.  Every time is the host clock around the synchronous call, median of --reps after --warmup (the
first save / load allocates the context's staging buffers); the GlobalCache dump is 2.4 GB a call, so it gets
--swap-reps.  The library's own split of a map call (tf_scene_ckpt_times) comes from a second pair of contexts
created with TFUSION_CKPT_TIMING=1 (HIP events and a wait around the kernels).  One JSON line at the end; --out
appends the report to a file.

    python tools/map_ckpt_time.py [--frames 5000] [--reps 5] [--swap-reps 2] [--dir DIR] [--out profiles/map_ckpt_time.txt]
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

PEAK_HBM_GBS = 8000.0        # MI355X HBM3E peak, as bench.py takes it


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
    ap.add_argument("--swap-reps", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    import topfusion_amd
    from topfusion_amd import TopFu, default_params, synth
    W, H = args.cols, args.rows
    fx, fy, cx, cy = synth.intrinsics(W, H)
    params = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=args.voxel, use_swapping=1,
                  swap_transfer_blocks=args.swap_transfer_blocks)
    t0 = time.perf_counter()
    stream, R, t = synth.hall_device(args.frames, W, H, 13)
    w2c = synth.world_to_camera_rt(R, t)
    tf = TopFu(default_params(**params), device=0)
    for k in range(0, args.frames, args.batch):
        tf.fuse_frames(stream.frame_ptr(k), w2c[k:min(k + args.batch, args.frames)])
    h, flags = tf.hash(), tf.swap_stored_flags()
    fuse_s = time.perf_counter() - t0
    stream.free()
    resident, stored = int((h["ptr"] >= 0).sum()), int((flags != 0).sum())
    other = TopFu(default_params(**params), device=0)
    n_whole = tf.mesh_count(whole=True)

    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path, cache = os.path.join(d, "map.tfmap"), os.path.join(d, "cache.bin")
        save_ms = median_ms(lambda: tf.save_map(path), args.reps, args.warmup)
        info = topfusion_amd.map_file_info(path)
        file_bytes = os.path.getsize(path)
        maps = sum(2 * 16 * (W >> l) * (H >> l) for l in range(3))
        formula = (304 + 24 * info["n_records"] + 2048 * (info["n_blocks_stored"] + info["n_cache_blocks"]) +
                   4 * (info["noVisibleEntries"] + info["lastFreeBlockId"] + 1 + info["lastFreeExcessListId"] + 1) + maps)
        assert file_bytes == info["file_bytes"] == formula, (file_bytes, info["file_bytes"], formula)
        assert (info["n_blocks_stored"], info["n_cache_blocks"]) == (resident, stored)
        load_ms = median_ms(lambda: other.load_map(path), args.reps, args.warmup)
        assert other.hash().tobytes() == h.tobytes() and other.swap_stored_flags().tobytes() == flags.tobytes()
        assert other.mesh_count(whole=True) == n_whole                     # both tiers are in place
        swap_save_ms = median_ms(lambda: tf.swap_save(cache), args.swap_reps, 1)
        cache_bytes = os.path.getsize(cache)
        assert cache_bytes == tf.n_total * 2049
        swap_load_ms = median_ms(lambda: other.swap_load(cache), args.swap_reps, 1)
        os.remove(cache)
        # the split, on contexts that time their kernels (the same state: loaded from the file)
        os.environ["TFUSION_CKPT_TIMING"] = "1"
        tf_t = TopFu.from_map(path, device=0)
        other_t = TopFu(default_params(**params), device=0)
        path_t = os.path.join(d, "map_t.tfmap")
        for _ in range(args.warmup + 2):
            tf_t.save_map(path_t)
            other_t.load_map(path_t)
        split = {"save": tf_t.scene_ckpt_times(), "load": other_t.scene_ckpt_times()}
        with open(path, "rb") as fa, open(path_t, "rb") as fb:
            assert fa.read() == fb.read()                                   # a save after a load reproduces the file
        tf_t.close()
        other_t.close()

    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    lines = [f"map_ckpt_time: C5E hall walk, {args.frames} frames fused with swapping in {fuse_s:.1f} s (render + fuse), {W}x{H}, "
             f"{args.voxel * 1000:g} mm voxels, {tf.n_total} hash entries, {tf.params().n_blocks} VBA blocks, "
             f"<= {args.swap_transfer_blocks} blocks per transfer",
             f"state: {info['n_records']} records, {resident} active + {stored} stored blocks, {n_whole} whole-map triangles",
             f"map file {file_bytes} bytes == 304 + 24 R + 2048 (b + s) + 4 (V + A + E) + M = {formula}; GlobalCache dump "
             f"{cache_bytes} bytes ({tf.n_total} x 2049): the map file is {file_bytes / cache_bytes:.4f} x"]
    out = {"tool": "map_ckpt_time", "frames": args.frames, "cols": W, "rows": H, "voxel": args.voxel, "hash_entries": tf.n_total,
           "n_blocks": tf.params().n_blocks, "records": info["n_records"], "active_blocks": resident, "stored_blocks": stored,
           "triangles_whole": n_whole, "file_bytes": file_bytes, "formula_bytes": formula, "cache_dump_bytes": cache_bytes,
           "save_ms": round(save_ms[0], 3), "save_ms_min": round(save_ms[1], 3), "load_ms": round(load_ms[0], 3),
           "load_ms_min": round(load_ms[1], 3), "swap_save_ms": round(swap_save_ms[0], 3), "swap_save_ms_min": round(swap_save_ms[1], 3),
           "swap_load_ms": round(swap_load_ms[0], 3), "swap_load_ms_min": round(swap_load_ms[1], 3), "reps": args.reps,
           "swap_reps": args.swap_reps, "peak_hbm_gbs": PEAK_HBM_GBS,
           "timing": "host clock around the synchronous calls (median); the split from contexts with TFUSION_CKPT_TIMING=1 (HIP events around the kernels)"}
    for name, whole in (("save", save_ms), ("load", load_ms)):
        s = split[name]
        kgbs = gbs(s["block_kernel_bytes"], s["block_kernels"])
        out.update({f"{name}_{k}": round(v, 4) for k, v in s.items()})
        out[f"{name}_block_kernel_gbs"] = round(kgbs, 1)
        lines.append(f"{name}: {whole[0]:.2f} ms (min {whole[1]:.2f})  -- a call with timed kernels {s['call']:.2f} ms: index kernels "
                     f"{s['index_kernels']:.3f}, block kernels (both payloads) {s['block_kernels']:.3f} ({kgbs:.0f} GB/s read + written, "
                     f"{100 * kgbs / PEAK_HBM_GBS:.1f} % of peak; {100 * s['block_kernels'] / s['call']:.1f} % of the call), copies "
                     f"{s['copies']:.2f}, record check + checksum {s['check']:.3f}, file {s['file']:.2f}")
    lines.append(f"tf_swap_save (flags + the whole store, D2H + write): {swap_save_ms[0]:.1f} ms (min {swap_save_ms[1]:.1f})  -- "
                 f"tf_map_save is {save_ms[0] / swap_save_ms[0]:.4f} x")
    lines.append(f"tf_swap_load (read + H2D): {swap_load_ms[0]:.1f} ms (min {swap_load_ms[1]:.1f})  -- tf_map_load is "
                 f"{load_ms[0] / swap_load_ms[0]:.4f} x")
    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text)
    tf.close()
    other.close()


if __name__ == "__main__":
    main()
