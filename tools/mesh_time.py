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

--attr adds tf_mesh_extract_attr on the same window, in the same run: normals only, normals + positions
(both on the same context) and positions + normals + colours on a voxel_rgb context fused with the
synthetic RGB stream of the colour tests (synth.render_colour at the orbit's poses), beside that
context's own positions-only time.  Floor: live blocks x 2 KiB per pass + (36 + 36 + 12) B per triangle
for what is written.  --parent-lib PATH (a libtfusion_hip.so built from the parent commit) runs the
plain measurement once more in a child process on that library and records its positions-only time.

--indexed adds tf_mesh_extract_indexed on the same window, in the same run: the count passes alone, then
positions, positions + normals, and (on the voxel_rgb context) all attributes, each beside the soup
extraction of the same outputs timed in this run, with the bytes each form writes -- what a caller then
downloads.  Floor: live blocks x 2 KiB per pass (count, mark, vertices, indices) + 448 B of edge bits per
VBA block cleared + 12 B per triangle + (12 + 12 + 4) B per vertex for what is written.

    python tools/mesh_time.py [--frames 32] [--reps 20] [--warmup 3] [--attr] [--indexed] [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import subprocess
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
    ap.add_argument("--attr", action="store_true", help="also time tf_mesh_extract_attr")
    ap.add_argument("--indexed", action="store_true", help="also time tf_mesh_extract_indexed beside the soup calls")
    ap.add_argument("--parent-lib", default=None, help="a parent-commit libtfusion_hip.so to time positions-only extraction on")
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

    def timed_call(call, expect=None):
        got = ctypes.c_longlong()
        ms = []
        for i in range(args.warmup + args.reps):
            assert hip.hipEventRecord(e0, stream) == 0
            call(got)
            assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
            t = ctypes.c_float()
            assert hip.hipEventElapsedTime(ctypes.byref(t), e0, e1) == 0
            assert got.value == (n if expect is None else expect)
            if i >= args.warmup:
                ms.append(t.value)
        return float(np.median(ms)), float(np.min(ms))

    def timed(buf, cap):
        return timed_call(lambda got: L.check(lib.tf_mesh_extract(tf._h, buf, cap, ctypes.byref(got)), "tf_mesh_extract"))

    count_ms, count_min = timed(None, 0)
    full_ms, full_min = timed(dev, n)
    attr = {}
    if args.attr:
        attr = time_attr(args, tf, n, live, dev, timed_call, full_ms)
    if args.indexed:
        idx = time_indexed(args, tf, n, live, dev, timed_call, full_ms)
        attr.setdefault("lines", []).extend(idx.pop("lines"))
        attr.update(idx)
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
    for line in attr.pop("lines", []):
        print(line)
    out.update(attr)
    if args.parent_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--frames", str(args.frames), "--cols", str(W), "--rows", str(H),
               "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, env=dict(os.environ, TFUSION_HIP_LIB=os.path.abspath(args.parent_lib)), capture_output=True, text=True,
                           check=True)
        parent = json.loads(r.stdout.strip().splitlines()[-1])
        assert parent["triangles"] == n and parent["live_blocks"] == live
        out["parent_full_ms"], out["parent_full_ms_min"], out["parent_count_ms"] = parent["full_ms"], parent["full_ms_min"], parent["count_ms"]
        print(f"parent commit's library, same box: count only {parent['count_ms']:.3f} ms, full (positions only) {parent['full_ms']:.3f} ms"
              f"  -- this build: {count_ms:.3f} / {full_ms:.3f} ms")
    print(json.dumps(out))
    frames.free()
    tf.close()


def time_attr(args, tf, n, live, dev_tris, timed_call, full_ms):
    """tf_mesh_extract_attr: normals only and normals + positions on `tf`; then a voxel_rgb context fused
    with the same depth frames and the synthetic RGB stream: positions only (tf_mesh_extract) and all
    three outputs.  Returns the JSON fields and the printed lines."""
    from topfusion_amd import TopFu, default_params, synth, _lib as L
    lib, hip = L.load(), L.hip_runtime()
    W, H = args.cols, args.rows

    def dev_alloc(nbytes):
        d = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(d), max(16, nbytes)) == 0, "hipMalloc"
        return d

    dev_nrm, dev_col = dev_alloc(n * 36), dev_alloc(n * 12)

    def attr_call(ctx, t, nr, co):
        return lambda got: L.check(lib.tf_mesh_extract_attr(ctx._h, t, nr, co, n, ctypes.byref(got)), "tf_mesh_extract_attr")

    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9
    fields, lines = {}, []

    def report(key, label, ms, mn, per_tri, base_ms, tris=n):
        floor = 2 * live * 2048 + per_tri * tris
        fields.update({f"{key}_ms": round(ms, 4), f"{key}_ms_min": round(mn, 4), f"floor_bytes_{key}": floor,
                       f"{key}_gbs": round(gbs(floor, ms), 2), f"{key}_over_positions_only": round(ms / base_ms, 3)})
        lines.append(f"{label}: {ms:.3f} ms  ({fields[key + '_gbs']} GB/s of the floor's bytes, {100 * gbs(floor, ms) / PEAK_HBM_GBS:.2f} % of peak; "
                     f"{ms / base_ms:.2f} x positions only, bytes written {per_tri} / 36 = {per_tri / 36:.2f} x)")

    ms, mn = timed_call(attr_call(tf, None, dev_nrm, None))
    report("normals", "normals only           ", ms, mn, 36, full_ms)
    ms, mn = timed_call(attr_call(tf, dev_tris, dev_nrm, None))
    report("pos_normals", "positions + normals    ", ms, mn, 72, full_ms)

    tc = colour_context(args)
    nc = tc.mesh_count()
    assert nc <= n, (nc, n)                                    # (the buffers hold n; colour does not move the geometry)
    plane = tc.vba_rgb()
    fields.update({"rgb_ctx_triangles": nc, "coloured_voxels": int((plane >> 24 > 0).sum())})
    ms_pos, mn_pos = timed_call(lambda got: L.check(lib.tf_mesh_extract(tc._h, dev_tris, n, ctypes.byref(got)), "tf_mesh_extract"), nc)
    fields.update({"rgb_ctx_full_ms": round(ms_pos, 4), "rgb_ctx_full_ms_min": round(mn_pos, 4)})
    lines.append(f"colour context ({nc} triangles), positions only (tf_mesh_extract): {ms_pos:.3f} ms")
    ms, mn = timed_call(attr_call(tc, dev_tris, dev_nrm, dev_col), nc)
    report("all", "positions + normals + colours", ms, mn, 84, ms_pos, nc)
    for d in (dev_nrm, dev_col):
        hip.hipFree(d)
    tc.close()
    fields["lines"] = lines
    return fields


def colour_context(args):
    """A voxel_rgb context fused with the same depth frames and the colour tests' RGB stream (a registered
    colour camera)."""
    from topfusion_amd import TopFu, default_params, synth, _lib as L
    hip = L.hip_runtime()
    W, H = args.cols, args.rows
    fx, fy, cx, cy = synth.intrinsics(W, H)
    tc = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxel_rgb=1), device=0)
    frames = synth.orbit_device(args.frames, W, H, seed=7)
    rgbs = np.stack([synth.render_colour(*synth.orbit_pose(k), W, H) for k in range(args.frames)])
    dev_rgb = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev_rgb), rgbs.nbytes) == 0, "hipMalloc"
    assert hip.hipMemcpy(dev_rgb, rgbs.ctypes.data_as(ctypes.c_void_p), rgbs.nbytes, 1) == 0
    tc.process_frames(frames.ptr, args.frames, rgb_frames=dev_rgb.value)
    tc.mesh_count()                                           # (synchronises: the frames are done with their inputs)
    hip.hipFree(dev_rgb)
    frames.free()
    return tc


def time_indexed(args, tf, n, live, dev_tris, timed_call, full_ms):
    """tf_mesh_extract_indexed beside the soup calls with the same outputs: count only, positions, positions +
    normals on `tf`; all attributes on a voxel_rgb context.  Returns the JSON fields and the printed lines."""
    from topfusion_amd import _lib as L
    lib, hip = L.load(), L.hip_runtime()

    def dev_alloc(nbytes):
        d = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(d), max(16, nbytes)) == 0, "hipMalloc"
        return d

    nv, nt = tf.mesh_indexed_count()
    assert nt == n
    dev_v, dev_vn, dev_vc, dev_i = dev_alloc(nv * 12), dev_alloc(nv * 12), dev_alloc(nv * 4), dev_alloc(nt * 12)
    dev_nrm, dev_col = dev_alloc(n * 36), dev_alloc(n * 12)
    n_blocks = tf.params_.n_blocks
    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9
    fields, lines = {"indexed_vertices": nv, "indexed_triangles": nt}, []
    lines.append(f"indexed: {nv} vertices, {nt} triangles ({3 * nt / nv:.2f} triangle corners per vertex)")

    def indexed_call(ctx, v, vn, vc, vcap, i, icap, want_nv):
        def call(got):
            gv = ctypes.c_longlong()
            L.check(lib.tf_mesh_extract_indexed(ctx._h, v, vn, vc, vcap, i, icap, ctypes.byref(gv), ctypes.byref(got)),
                    "tf_mesh_extract_indexed")
            assert gv.value == want_nv
        return call

    def report(key, label, ms, mn, soup_ms, per_vertex, per_tri_soup, verts, tris):
        written, soup = 12 * tris + per_vertex * verts, per_tri_soup * tris
        floor = 4 * live * 2048 + n_blocks * 448 + written
        fields.update({f"indexed_{key}_ms": round(ms, 4), f"indexed_{key}_ms_min": round(mn, 4), f"soup_{key}_ms": round(soup_ms, 4),
                       f"indexed_{key}_bytes": written, f"soup_{key}_bytes": soup, f"floor_bytes_indexed_{key}": floor,
                       f"indexed_{key}_gbs": round(gbs(floor, ms), 2)})
        lines.append(f"indexed {label}: {ms:.3f} ms against the soup's {soup_ms:.3f} ms ({ms / soup_ms:.2f} x); bytes written "
                     f"{written} against {soup} ({written / tris:.1f} against {per_tri_soup} B per triangle, {written / soup:.2f} x); "
                     f"{fields[f'indexed_{key}_gbs']} GB/s of the floor's bytes, {100 * gbs(floor, ms) / PEAK_HBM_GBS:.2f} % of peak")

    ms, mn = timed_call(indexed_call(tf, None, None, None, 0, None, 0, nv))
    fields.update({"indexed_count_ms": round(ms, 4), "indexed_count_ms_min": round(mn, 4)})
    lines.append(f"indexed count only (triangle count + edge marks + vertex count): {ms:.3f} ms")
    ms, mn = timed_call(indexed_call(tf, dev_v, None, None, nv, dev_i, nt, nv))
    report("pos", "positions            ", ms, mn, full_ms, 12, 36, nv, nt)
    soup_ms, _ = timed_call(lambda got: L.check(lib.tf_mesh_extract_attr(tf._h, dev_tris, dev_nrm, None, n, ctypes.byref(got)),
                                                "tf_mesh_extract_attr"))
    ms, mn = timed_call(indexed_call(tf, dev_v, dev_vn, None, nv, dev_i, nt, nv))
    report("pos_normals", "positions + normals  ", ms, mn, soup_ms, 24, 72, nv, nt)

    tc = colour_context(args)
    cv, ct = tc.mesh_indexed_count()
    assert ct <= n and cv <= nv, (ct, n, cv, nv)             # (the buffers hold n / nv; colour does not move the geometry)
    soup_ms, _ = timed_call(lambda got: L.check(lib.tf_mesh_extract_attr(tc._h, dev_tris, dev_nrm, dev_col, n, ctypes.byref(got)),
                                                "tf_mesh_extract_attr"), ct)
    ms, mn = timed_call(indexed_call(tc, dev_v, dev_vn, dev_vc, nv, dev_i, nt, cv), ct)
    report("all", "all attributes       ", ms, mn, soup_ms, 28, 84, cv, ct)
    for d in (dev_v, dev_vn, dev_vc, dev_i, dev_nrm, dev_col):
        hip.hipFree(d)
    tc.close()
    fields["lines"] = lines
    return fields


if __name__ == "__main__":
    main()
