#!/usr/bin/env python3
"""Time of scene checkpoints on the bench's scene (DESIGN.md §5 Scene checkpoints, measurement).

Fuses the C2 orbit (bench.py's flagship workload: the synthetic room + sphere orbit at 640x480, 5 mm) for
one 32-frame window, then times, in the same run and into the same directory:

    save      tf_scene_save of that context           load      tf_scene_load into a second context
    dump      what the parent commit can do for the same scene: tf_download of TF_BUF_HASH + TF_BUF_VBA into
              host memory and a write of both to one file
    restore   the reverse: a read of that file, tf_upload of both (neither restores the free lists, the
              visible list, the pose or the tracker's maps)

Every figure is the median of --reps calls after --warmup (the first save / load allocates the context's
staging buffers).  The library's own split of a call (tf_scene_ckpt_times) comes from a second pair of
contexts created with TFUSION_CKPT_TIMING=1, which puts HIP events and a wait around the kernels: the
index kernels and the block gather / scatter kernels, with the block kernels' bytes (read + written) per
second against the HBM peak; the D2H / H2D copies; the record check and checksum; the file time.  One
JSON line at the end.

    python tools/scene_ckpt_time.py [--frames 32] [--reps 10] [--warmup 2] [--dir DIR]
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
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    args = ap.parse_args()

    import topfusion_amd
    from topfusion_amd import TopFu, default_params, synth, _lib as L
    W, H = args.cols, args.rows
    fx, fy, cx, cy = synth.intrinsics(W, H)
    params = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy)
    tf = TopFu(default_params(**params), device=0)
    frames = synth.orbit_device(args.frames, W, H, seed=7)
    ok = tf.process_frames(frames.ptr, args.frames)
    other = TopFu(default_params(**params), device=0)

    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        scene, dump = os.path.join(d, "scene.tfscene"), os.path.join(d, "tables.bin")
        split = {}

        def save():
            tf.save_scene(scene)

        def load():
            other.load_scene(scene)

        def dump_tables():
            h, v = tf.download(L.TF_BUF_HASH), tf.download(L.TF_BUF_VBA)
            with open(dump, "wb") as f:
                f.write(h)
                f.write(v)

        nh, nv = tf.nbytes(L.TF_BUF_HASH), tf.nbytes(L.TF_BUF_VBA)

        def restore_tables():
            with open(dump, "rb") as f:
                h = np.frombuffer(f.read(nh), np.uint8)
                v = np.frombuffer(f.read(nv), np.uint8)
            other.upload(L.TF_BUF_HASH, h)
            other.upload(L.TF_BUF_VBA, v)

        save_ms = median_ms(save, args.reps, args.warmup)
        info = topfusion_amd.scene_file_info(scene)
        load_ms = median_ms(load, args.reps, args.warmup)
        assert other.hash().tobytes() == tf.hash().tobytes() and other.vba().tobytes() == tf.vba().tobytes()
        dump_ms = median_ms(dump_tables, args.reps, args.warmup)
        restore_ms = median_ms(restore_tables, args.reps, args.warmup)
        dump_bytes = os.path.getsize(dump)
        # the split, on contexts that time their kernels (the same state: loaded from the file)
        os.environ["TFUSION_CKPT_TIMING"] = "1"
        tf_t = TopFu.from_scene(scene, device=0)
        other_t = TopFu(default_params(**params), device=0)
        scene_t = os.path.join(d, "scene_t.tfscene")
        for _ in range(args.warmup + 3):
            tf_t.save_scene(scene_t)
            other_t.load_scene(scene_t)
        split["save"], split["load"] = tf_t.scene_ckpt_times(), other_t.scene_ckpt_times()
        with open(scene, "rb") as fa, open(scene_t, "rb") as fb:
            assert fa.read() == fb.read()
        tf_t.close()
        other_t.close()

    n_blocks = tf.params_.n_blocks
    fill = info["n_blocks_stored"] / n_blocks
    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    out = {"tool": "scene_ckpt_time", "frames": args.frames, "frames_ok": int(ok.sum()), "cols": W, "rows": H,
           "hash_entries": tf.n_total, "n_blocks": n_blocks, "records": info["n_records"], "blocks": info["n_blocks_stored"],
           "file_bytes": info["file_bytes"], "dump_bytes": dump_bytes, "vba_fill": round(fill, 5),
           "save_ms": round(save_ms[0], 3), "save_ms_min": round(save_ms[1], 3), "load_ms": round(load_ms[0], 3),
           "load_ms_min": round(load_ms[1], 3), "dump_ms": round(dump_ms[0], 3), "dump_ms_min": round(dump_ms[1], 3),
           "restore_ms": round(restore_ms[0], 3), "restore_ms_min": round(restore_ms[1], 3), "peak_hbm_gbs": PEAK_HBM_GBS,
           "reps": args.reps, "timing": "host clock around the synchronous calls (median); the split from contexts with TFUSION_CKPT_TIMING=1 (HIP events around the kernels)"}
    print(f"records {info['n_records']}  blocks {info['n_blocks_stored']} of {n_blocks} ({100 * fill:.1f} % of the VBA)  "
          f"file {info['file_bytes']} bytes  -- hash + VBA dump {dump_bytes} bytes ({info['file_bytes'] / dump_bytes:.3f} x)")
    for name, whole in (("save", save_ms), ("load", load_ms)):
        s = split[name]
        kgbs = gbs(s["block_kernel_bytes"], s["block_kernels"])
        out.update({f"{name}_{k}": round(v, 4) for k, v in s.items()})
        out[f"{name}_block_kernel_gbs"] = round(kgbs, 1)
        print(f"{name}: {whole[0]:.2f} ms (min {whole[1]:.2f})  -- a call with timed kernels {s['call']:.2f} ms: index kernels {s['index_kernels']:.3f}, "
              f"block kernels {s['block_kernels']:.3f} ({kgbs:.0f} GB/s read + written, {100 * kgbs / PEAK_HBM_GBS:.1f} % of peak; "
              f"{100 * s['block_kernels'] / s['call']:.1f} % of the call), copies {s['copies']:.2f}, record check + checksum {s['check']:.3f}, "
              f"file {s['file']:.2f}")
    print(f"dump (tf_download hash + VBA, write): {dump_ms[0]:.2f} ms (min {dump_ms[1]:.2f})  -- save is {save_ms[0] / dump_ms[0]:.2f} x")
    print(f"restore (read, tf_upload hash + VBA): {restore_ms[0]:.2f} ms (min {restore_ms[1]:.2f})  -- load is {load_ms[0] / restore_ms[0]:.2f} x")
    print(json.dumps(out))
    frames.free()
    tf.close()
    other.close()


if __name__ == "__main__":
    main()
