#!/usr/bin/env python3
"""The whole map's indexed mesh against its soup on a swapping scene (DESIGN.md §Mesh extraction, the whole map, indexed).

The scene is tools/mesh_whole_time.py's: the C5E hall walk (seed 13, 640x480, 10 mm voxels, reference capacities)
fused for --frames frames through tf_scene_fuse_frames with the swapping engine on.  One run then measures, for the
soup (tf_mesh_extract_whole: the parent's path) and the indexed form (tf_mesh_extract_indexed_whole) side by side:

  * nv and nt, and the bytes that leave the device, without and with normals;
  * the extraction time: HIP events on the context stream around the synchronous call and the host clock around it
    (the indexed call waits once in the middle for the number of resolving entries), median of --reps after --warmup,
    in --rounds rounds that alternate soup and indexed so that each has the other's spread beside it;
  * the scratch the indexed form holds: one int per hash entry, group counts, 896 B per resolving entry;
  * the save: save_mesh(whole=True) (download the soup, weld on the host, write) against save_mesh_indexed_whole (chunked),
    the host clock, the file sizes, and the growth of the process's peak resident set over each call -- the chunked one
    first, since a peak only grows.

One JSON line at the end; --out appends the report to a file.

    python tools/mesh_indexed_whole_time.py [--frames 5000] [--reps 20] [--warmup 3] [--rounds 2] [--no-save] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import resource
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EDGE_ROW_BYTES = 2 * 448         # edge bits and their prefixes per resolving entry (TFM_EDGE_WORDS words each)


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
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-save", action="store_true", help="skip the two file saves")
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()

    from topfusion_amd import TopFu, default_params, synth, _lib as L
    W, H = args.cols, args.rows
    fx, fy, cx, cy = synth.intrinsics(W, H)
    stream, R, t = synth.hall_device(args.frames, W, H, 13)
    w2c = synth.world_to_camera_rt(R, t)
    tf = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=args.voxel, use_swapping=1,
                              swap_transfer_blocks=args.swap_transfer_blocks), device=0)
    for k in range(0, args.frames, args.batch):
        tf.fuse_frames(stream.frame_ptr(k), w2c[k:min(k + args.batch, args.frames)])
    h, flags = tf.hash(), tf.swap_stored_flags()
    p, f = h["ptr"], flags != 0
    resident_blocks, stored_blocks = int((p >= 0).sum()), int(((p == -1) & f).sum())
    resolving = resident_blocks + stored_blocks
    nt_soup = tf.mesh_count(whole=True)
    nv, nt = tf.mesh_indexed_whole_count()
    assert nt == nt_soup, (nt, nt_soup)
    n_groups = (tf.n_total + 511) // 512
    scratch = {"slot_table": 4 * (tf.n_total + n_groups + 1), "edge_rows": EDGE_ROW_BYTES * max(resolving, 1),
               "vertex_counts": 8 * (tf.n_total + n_groups) + 8 * (tf.n_total + 1)}

    lib, hip = L.load(), L.hip_runtime()
    hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventDestroy.argtypes = [ctypes.c_void_p]
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    cstream = ctypes.c_void_p(tf.stream())
    bufs = {}
    for name, size in (("tris", nt * 36), ("tri_normals", nt * 36), ("verts", nv * 12), ("normals", nv * 12), ("indices", nt * 12)):
        bufs[name] = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(bufs[name]), max(16, size)) == 0, "hipMalloc"

    def timed_call(call):
        ev, host = [], []
        for i in range(args.warmup + args.reps):
            assert hip.hipEventRecord(e0, cstream) == 0
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            assert hip.hipEventRecord(e1, cstream) == 0 and hip.hipEventSynchronize(e1) == 0
            el = ctypes.c_float()
            assert hip.hipEventElapsedTime(ctypes.byref(el), e0, e1) == 0
            if i >= args.warmup:
                ev.append(el.value)
                host.append((t1 - t0) * 1e3)
        return float(np.median(ev)), float(np.min(ev)), float(np.max(ev)), float(np.median(host))

    gv, gt = ctypes.c_longlong(), ctypes.c_longlong()

    def soup(bt, bn, cap):
        def call():
            L.check(lib.tf_mesh_extract_whole(tf._h, bt, bn, cap, ctypes.byref(gt)), "tf_mesh_extract_whole")
            assert gt.value == nt
        return call

    def indexed(bv, bn, vcap, bi, tcap):
        def call():
            L.check(lib.tf_mesh_extract_indexed_whole(tf._h, bv, bn, vcap, bi, tcap, ctypes.byref(gv), ctypes.byref(gt)),
                    "tf_mesh_extract_indexed_whole")
            assert (gv.value, gt.value) == (nv, nt)
        return call

    runs = [("soup count only      ", soup(None, None, 0), 0),
            ("indexed count only   ", indexed(None, None, 0, None, 0), 0),
            ("soup positions       ", soup(bufs["tris"], None, nt), 36 * nt),
            ("indexed positions    ", indexed(bufs["verts"], None, nv, bufs["indices"], nt), 12 * nv + 12 * nt),
            ("soup with normals    ", soup(bufs["tris"], bufs["tri_normals"], nt), 72 * nt),
            ("indexed with normals ", indexed(bufs["verts"], bufs["normals"], nv, bufs["indices"], nt), 24 * nv + 12 * nt)]
    lines = [f"mesh_indexed_whole_time: C5E hall walk, {args.frames} frames fused with swapping, {W}x{H}, {args.voxel * 1000:g} mm voxels, "
             f"{tf.n_total} hash entries, {tf.params().n_blocks} VBA blocks; {resident_blocks} blocks resident, {stored_blocks} stored only, "
             f"{resolving} entries resolve",
             f"whole mesh: nt = {nt} triangles, nv = {nv} vertices ({nv / max(nt, 1):.3f} per triangle)",
             f"bytes leaving the device, positions: soup {36 * nt}  indexed {12 * nv + 12 * nt}  ({(12 * nv + 12 * nt) / max(36 * nt, 1):.3f} of the soup)",
             f"bytes leaving the device, with normals: soup {72 * nt}  indexed {24 * nv + 12 * nt}  ({(24 * nv + 12 * nt) / max(72 * nt, 1):.3f} of the soup)",
             f"indexed scratch held: {sum(scratch.values())} B = slot table {scratch['slot_table']} + edge bits and prefixes {scratch['edge_rows']} "
             f"({EDGE_ROW_BYTES} B x {resolving}) + vertex counts and bases {scratch['vertex_counts']} (shared with the resident form); "
             f"keyed by hash entry the edge rows alone would be {EDGE_ROW_BYTES * tf.n_total} B",
             f"extraction, ms per synchronous call: HIP events median (min, max) | host clock median; {args.reps} calls after {args.warmup}, "
             f"{args.rounds} rounds alternating soup and indexed"]
    out = {"tool": "mesh_indexed_whole_time", "frames": args.frames, "hash_entries": tf.n_total, "resident_blocks": resident_blocks,
           "stored_blocks": stored_blocks, "nv": nv, "nt": nt, "scratch_bytes": scratch, "reps": args.reps, "runs": {}, "save": {}}
    for rnd in range(args.rounds):
        for label, call, written in runs:
            ms, mn, mx, host = timed_call(call)
            lines.append(f"round {rnd + 1}  {label}: {written} B written, {ms:.3f} ms (min {mn:.3f}, max {mx:.3f}) | host {host:.3f} ms")
            out["runs"].setdefault(label.strip(), []).append({"bytes_written": written, "ms": round(ms, 4), "ms_min": round(mn, 4),
                                                              "ms_max": round(mx, 4), "host_ms": round(host, 4)})
    for d in bufs.values():
        hip.hipFree(d)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)

    if not args.no_save:
        rss = lambda: resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024      # (Linux: KiB)
        chunk = int(os.environ.get("TFUSION_MESH_CHUNK_BYTES", 8 << 20))
        with tempfile.TemporaryDirectory() as tmp:
            for label, path, save in (("indexed, chunked (save_mesh_indexed_whole)", os.path.join(tmp, "indexed.ply"),
                                       lambda q: tf.save_mesh_indexed_whole(q)),
                                      ("soup, welded on the host (save_mesh(whole=True))", os.path.join(tmp, "soup.ply"),
                                       lambda q: tf.save_mesh(q, whole=True))):
                before = rss()
                t0 = time.perf_counter()
                save(path)
                dt = time.perf_counter() - t0
                grew, size = rss() - before, os.path.getsize(path)
                lines.append(f"save {label}: {dt:.2f} s, file {size} B, peak resident set grew by {grew} B")
                out["save"][label.split(",")[0]] = {"seconds": round(dt, 3), "file_bytes": size, "peak_rss_growth_bytes": grew}
        lines.append(f"the chunked writer holds {chunk} B of pinned staging (TFUSION_MESH_CHUNK_BYTES) and a 65536 B record buffer, whatever the mesh")
        out["save"]["chunk_bytes"] = chunk

    text = "\n".join(lines) + "\n" + json.dumps(out) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text)
    stream.free()
    tf.close()


if __name__ == "__main__":
    main()
