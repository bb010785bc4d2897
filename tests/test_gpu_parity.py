"""GPU parity: every stage of the HIP path against the CPU oracle, bit for bit.

All comparisons are bit-exact (NaN == NaN): integer/index work (hash table, visible list,
counters, allocation order, voxel weights) and the floating point work, because both
sides implement the same canonical arithmetic.  The reference's
CUDA build cannot be run anywhere available, so the oracle is the judge.
"""
import numpy as np
import pytest

from parity_util import assert_bit_exact, assert_struct_exact, hash_block_set
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

I_RT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def make_pair(oracle_mod, cols=640, rows=480, **kw):
    from topfusion_amd import TopFu, default_params
    fx, fy, cx, cy = synth.intrinsics(cols, rows)
    args = dict(cols=cols, rows=rows, fx=fx, fy=fy, cx=cx, cy=cy, **kw)
    return TopFu(default_params(**args)), oracle_mod.Oracle(oracle_mod.default_params(**args))


def compare_scene(g, o, tag=""):
    hg, ho = g.hash(), o.hash()
    assert hash_block_set(hg) == hash_block_set(ho), f"{tag} allocated block sets differ"
    assert_struct_exact(f"{tag} hash", hg, ho, ["x", "y", "z", "offset", "ptr"])
    sg, so = g.stats(), o.counters()
    for k in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries"):
        assert sg[k] == so[k], f"{tag} {k}: gpu {sg[k]} oracle {so[k]}"
    assert_bit_exact(f"{tag} visible_ids", g.visible_ids(), o.visible_ids())
    assert_bit_exact(f"{tag} visible_type", g.visible_type(), o.visible_type())
    vg, vo = g.vba(), o.vba()
    assert_struct_exact(f"{tag} vba", vg, vo, ["sdf", "w"])


def test_preprocess(oracle_mod):
    g, o = make_pair(oracle_mod)
    d = synth.room_corner(noise_mm=2.0, holes=0.02, seed=3)
    d[100:110, 200:260] = 2500          # > 2047 mm (dists -1) and > 2 m (truncated)
    d[300, 300] = 65535
    g.stage_preprocess(d)
    assert_bit_exact("dists", g.dists(), oracle_mod.compute_dists(d))
    d0 = oracle_mod.truncate(oracle_mod.bilateral(d), 2.0)
    assert_bit_exact("depth0", g.curr_depth(0), d0)
    d1 = oracle_mod.pyr_down(d0)
    d2 = oracle_mod.pyr_down(d1)
    assert_bit_exact("depth1", g.curr_depth(1), d1)
    assert_bit_exact("depth2", g.curr_depth(2), d2)
    p = g.params()
    for l, dl in enumerate((d0, d1, d2)):
        div = float(1 << l)
        pts, nrm = oracle_mod.points_normals(dl, np.float32(p.fx) / np.float32(div), np.float32(p.fy) / np.float32(div),
                                             np.float32(p.cx) / np.float32(div), np.float32(p.cy) / np.float32(div))
        gp, gn = g.curr_maps(l)
        assert_bit_exact(f"points L{l}", gp, pts)
        assert_bit_exact(f"normals L{l}", gn, nrm)


def test_frame0_alloc_integrate(oracle_mod):
    g, o = make_pair(oracle_mod)
    d = synth.room_corner()
    assert g(d) is True
    assert o(d) is True
    compare_scene(g, o, "frame0")


def test_stage_raycast_maps_grey(oracle_mod):
    g, o = make_pair(oracle_mod)
    d = synth.room_corner()
    g(d)
    o(d)
    # CreateExpectedDepths / raycast / ICP maps / grey render at a slightly moved pose
    R, t = synth.orbit_pose(3)
    pose = np.zeros((3, 4), np.float32)
    pose[:, :3] = R
    pose[:, 3] = t
    inv = np.zeros((3, 4), np.float32)
    from oracle import oracle as O
    a = np.ascontiguousarray(pose.reshape(12))
    O.lib().tfo_rigid_inv(O.ptr(a), O.ptr(inv.reshape(12)))
    g.stage_expected_depths(inv)
    o.expected_depths(inv)
    assert_bit_exact("range", g.range_image(), o.range_image())
    assert g.stats()["noTotalBlocks"] == o.counters()["noTotalBlocks"]
    g.stage_raycast(pose, 1)
    o.raycast(pose, 1)
    assert_bit_exact("raycast", g.raycast_result(), o.raycast_result())
    assert_bit_exact("visible_type after raycast<true>", g.visible_type(), o.visible_type())
    g.stage_icp_maps(pose)
    op, on = o.render_icp(pose)
    gp, gn = g.prev_maps(0)
    assert_bit_exact("icp points L0", gp, op)
    assert_bit_exact("icp normals L0", gn, on)
    p1, n1 = oracle_mod.resize_points_normals(op, on)
    p2, n2 = oracle_mod.resize_points_normals(p1, n1)
    gp1, gn1 = g.prev_maps(1)
    gp2, gn2 = g.prev_maps(2)
    assert_bit_exact("icp points L1", gp1, p1)
    assert_bit_exact("icp normals L1", gn1, n1)
    assert_bit_exact("icp points L2", gp2, p2)
    assert_bit_exact("icp normals L2", gn2, n2)
    assert_bit_exact("grey", g.stage_render_grey(pose), o.render_grey(pose))


def test_icp_stage(oracle_mod, icp_schedule):
    g, o = make_pair(oracle_mod)
    _check_schedule(g, icp_schedule)
    seq = synth.orbit_sequence(2, seed=5)
    # prev = frame-0 camera maps, curr = frame-1 maps (the reference's frame-1 situation)
    g.stage_preprocess(seq[0])
    g.stage_swap_pyramids()
    g.stage_preprocess(seq[1])
    ok, aff, iters = g.stage_icp()
    o(seq[0])
    p = g.params()
    # oracle loop, exactly estimateTransform
    affine = I_RT.copy().reshape(12)
    oiters = 0
    ook = True
    for l, n_it in ((2, 4), (1, 5), (0, 10)):
        div = np.float32(1 << l)
        vc, nc = g.curr_maps(l)
        vp, npv = o.prev_maps(l)
        for _ in range(n_it):
            s = oracle_mod.icp_reduce(vc, nc, vp, npv, np.float32(p.fx) / div, np.float32(p.fy) / div,
                                      np.float32(p.cx) / div, np.float32(p.cy) / div,
                                      _cosf(p.icp_angle_thres),
                                      np.float32(p.icp_dist_thres) * np.float32(p.icp_dist_thres), affine)
            oiters += 1
            ok_i, affine, _ = oracle_mod.icp_step(s, affine)
            if not ok_i:
                ook = False
                break
        if not ook:
            break
    assert ok == ook
    assert iters == oiters
    assert_bit_exact("icp affine", aff.reshape(12), affine)


@pytest.fixture(params=["persistent", "per_iteration"])
def icp_schedule(request, monkeypatch):
    """Run a test under both ICP schedules: the persistent one-launch-per-frame kernel (the
    default) and the per-iteration fallback tf_create picks when the persistent grid cannot be
    co-resident (forced with TFUSION_ICP_PERSISTENT=0)."""
    monkeypatch.setenv("TFUSION_ICP_PERSISTENT", "0" if request.param == "per_iteration" else "1")
    return request.param


def _check_schedule(g, sched):
    assert g.icp_persistent() == (sched != "per_iteration")


def _cosf(x):
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.cosf.argtypes = [ctypes.c_float]
    libm.cosf.restype = ctypes.c_float
    return libm.cosf(x)


@pytest.mark.parametrize("cols,rows,nframes", [(640, 480, 6), (320, 240, 16)])
def test_sequence(oracle_mod, cols, rows, nframes, icp_schedule):
    """Whole TopFu::operator() frames: state identical after every frame."""
    g, o = make_pair(oracle_mod, cols, rows)
    _check_schedule(g, icp_schedule)
    _run_sequence(g, o, cols, rows, nframes)


def test_sequence_ed_atomic(oracle_mod, monkeypatch):
    """k_ed_fill's device-scope-atomic path (taken past ED_LDS_MAX_N visible entries, forced
    here with a threshold of 0): the whole range image after every frame, spill area included.
    (Thresholds inside a list's length, and crossed between two calls: tests/test_gpu_ed_edges.py.)"""
    monkeypatch.setenv("TFUSION_ED_LDS_MAX_N", "0")
    g, o = make_pair(oracle_mod, 320, 240)
    _run_sequence(g, o, 320, 240, 16)


@pytest.mark.parametrize("lds_max_n", ["16384", "0"])
def test_sequence_render_block_cap(oracle_mod, monkeypatch, lds_max_n):
    """MAX_RENDERING_BLOCKS engaged (a cap of 48 tiles): blocks whose tiles do not fit are
    dropped in visible-list order (VisualisationHelper.cu:70-74), on both k_ed_fill paths.
    (Caps that land exactly on a block, a chunk boundary and the last entry: tests/test_gpu_ed_edges.py.)"""
    monkeypatch.setenv("TFUSION_ED_LDS_MAX_N", lds_max_n)
    g, o = make_pair(oracle_mod, 320, 240, max_render_blocks=48)
    capped = _run_sequence(g, o, 320, 240, 8, need_spill=False)
    assert capped > 0, "the cap never engaged"


def _run_sequence(g, o, cols, rows, nframes, need_spill=True):
    seq = synth.orbit_sequence(nframes, cols, rows, seed=7)
    spilled = capped = 0
    for k in range(nframes):
        okg = g(seq[k])
        oko = o(seq[k])
        assert okg == oko, f"frame {k}: ok gpu {okg} oracle {oko}"
        sg, so = g.last_stats, o.counters()
        for key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries", "icp_iterations", "frame_counter"):
            assert sg[key] == so[key], f"frame {k} {key}: gpu {sg[key]} oracle {so[key]}"
        if k > 0:
            assert sg["noTotalBlocks"] == so["noTotalBlocks"], f"frame {k} noTotalBlocks"
            capped += int(oko and so["noTotalBlocks"] == o.params.max_render_blocks)
        assert_bit_exact(f"frame {k} pose", g.getCameraPose()[:3, :4], o.pose())
        if k > 0 and oko:
            assert_bit_exact(f"frame {k} renderImage grey", g.frame_grey(), o.frame_grey())
            # the whole range image, including the pixels outside the /8 region that boxes
            # clamped to the full-resolution W-1 / H-1 spill into
            rg = g.range_image()
            assert_bit_exact(f"frame {k} range image", rg, o.range_image())
            rc, rr = (cols - 1) // 8 + 1, (rows - 1) // 8 + 1
            spill = rg.copy()
            spill[:rr, :rc] = 0
            spilled += int((spill[..., 1] > np.float32(0.05)).sum())
    assert spilled > 0 or not need_spill, "no frame filled the range image outside its /8 region"
    compare_scene(g, o, "final")
    assert_bit_exact("final raycast", g.raycast_result(), o.raycast_result())
    for l in range(3):
        gp, gn = g.prev_maps(l)
        op, on = o.prev_maps(l)
        assert_bit_exact(f"final prev points L{l}", gp, op)
        assert_bit_exact(f"final prev normals L{l}", gn, on)
    return capped


def test_sequence_c3_geometry(oracle_mod):
    """C3 geometry: 1280x960, 2 mm voxels, capacities past the reference's; the
    persistent ICP re-reads the current maps of the CTA slots beyond its register-resident ones."""
    cols, rows = 1280, 960
    g, o = make_pair(oracle_mod, cols, rows, voxelSize=0.002, n_blocks=1 << 17)
    seq = synth.orbit_sequence(3, cols, rows, seed=7)
    for k in range(3):
        okg, oko = g(seq[k]), o(seq[k])
        assert okg == oko, f"frame {k}: ok gpu {okg} oracle {oko}"
        sg, so = g.last_stats, o.counters()
        for key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries", "icp_iterations"):
            assert sg[key] == so[key], f"frame {k} {key}: gpu {sg[key]} oracle {so[key]}"
        assert_bit_exact(f"frame {k} pose", g.getCameraPose()[:3, :4], o.pose())
    assert o.params.n_blocks - 1 - o.counters()["lastFreeBlockId"] > 20000      # a C3-sized scene
    compare_scene(g, o, "C3 final")
    assert_bit_exact("C3 final raycast", g.raycast_result(), o.raycast_result())


def test_icp_failure_reset(oracle_mod, icp_schedule):
    """A frame without correspondences fails the det check -> reset (topfu.cpp:263-264)."""
    g, o = make_pair(oracle_mod, 320, 240)
    _check_schedule(g, icp_schedule)
    seq = synth.orbit_sequence(3, 320, 240, seed=9)
    empty = np.zeros_like(seq[0])
    frames = [seq[0], seq[1], empty, seq[2], seq[0]]
    for k, f in enumerate(frames):
        okg, oko = g(f), o(f)
        assert okg == oko, f"frame {k}: gpu {okg} oracle {oko}"
        sg, so = g.last_stats, o.counters()
        for key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries", "icp_iterations", "frame_counter",
                    "n_resets"):
            assert sg[key] == so[key], f"frame {k} {key}: gpu {sg[key]} oracle {so[key]}"
    compare_scene(g, o, "after reset")


def test_small_hash_excess_chains(oracle_mod):
    """Tiny bucket array: heavy collisions exercise excess chains and ordered excess slots."""
    g, o = make_pair(oracle_mod, 320, 240, n_buckets=4096, n_excess=8192, n_blocks=16384, vis_capacity=65536)
    seq = synth.orbit_sequence(4, 320, 240, seed=11)
    for k in range(4):
        assert g(seq[k]) == o(seq[k])
    compare_scene(g, o, "excess")
    assert (g.hash()["offset"] > 0).sum() > 0


def test_capacity_exhaustion(oracle_mod):
    """VBA smaller than the request count: the serial-order fallback must match."""
    g, o = make_pair(oracle_mod, 320, 240, n_buckets=4096, n_excess=256, n_blocks=600, vis_capacity=65536)
    seq = synth.orbit_sequence(3, 320, 240, seed=13)
    for k in range(3):
        assert g(seq[k]) == o(seq[k])
        sg, so = g.last_stats, o.counters()
        assert sg["lastFreeBlockId"] == so["lastFreeBlockId"]
        assert sg["lastFreeExcessListId"] == so["lastFreeExcessListId"]
    compare_scene(g, o, "exhausted")


def test_batched_frames_overlap(oracle_mod, icp_schedule):
    """The device-driven batch path (tf_process_frames): frames enqueued back to back with no
    host sync, CreateICPMaps' raycast and renderImage in one launch, later frames'
    preprocessing in this frame's grid tails (two-frame lookahead with ping-pong level-0 depth,
    across the 32-frame group boundary and the ICP-failure resets too), CreateExpectedDepths'
    projection inside k_integrate's grid, the frame end (ResetScene on ICP failure) inside
    k_icp_maps' grid and setToType3 + the renderImage snapshot in the persistent ICP grid's
    tail.  Per-frame results, the last frame's grey image, the final pose and the whole scene
    match the oracle run frame by frame."""
    from parity_util import DeviceFrames
    from topfusion_amd import TopFu, default_params
    cols, rows, n = 320, 240, 40          # 40 frames > one 32-frame enqueue group
    fx, fy, cx, cy = synth.intrinsics(cols, rows)
    args = dict(cols=cols, rows=rows, fx=fx, fy=fy, cx=cx, cy=cy)
    g = TopFu(default_params(**args))
    _check_schedule(g, icp_schedule)
    o = oracle_mod.Oracle(oracle_mod.default_params(**args))
    seq = synth.orbit_sequence(n, cols, rows, seed=7)
    dev = DeviceFrames(seq)
    okg = g.process_frames(dev.ptr, n)
    oko = np.array([o(seq[k]) for k in range(n)])
    assert np.array_equal(okg, oko), (okg, oko)
    assert (~oko).sum() >= 1, "sequence should include an ICP-failure reset"
    sg, so = g.stats(), o.counters()
    for key in ("frame_counter", "n_resets", "icp_iterations"):
        assert sg[key] == so[key], f"{key}: gpu {sg[key]} oracle {so[key]}"
    assert_bit_exact("batched final pose", g.getCameraPose()[:3, :4], o.pose())
    if oko[-1]:
        assert_bit_exact("batched last renderImage grey", g.frame_grey(), o.frame_grey())
    compare_scene(g, o, "batched")
    assert_bit_exact("batched final raycast", g.raycast_result(), o.raycast_result())
    g.close()
    dev.free()


def _compare_frame_state(g, o, tag, grey=True):
    assert_bit_exact(f"{tag} range image", g.range_image(), o.range_image())
    sg, so = g.stats(), o.counters()
    for key in ("frame_counter", "n_resets", "icp_iterations", "lastFreeBlockId", "lastFreeExcessListId",
                "noVisibleEntries"):
        assert sg[key] == so[key], f"{tag} {key}: gpu {sg[key]} oracle {so[key]}"
    assert_bit_exact(f"{tag} pose", g.getCameraPose()[:3, :4], o.pose())
    if grey:
        assert_bit_exact(f"{tag} renderImage grey", g.frame_grey(), o.frame_grey())
    assert_bit_exact(f"{tag} raycast", g.raycast_result(), o.raycast_result())
    for l in range(3):
        gp, gn = g.prev_maps(l)
        op, on = o.prev_maps(l)
        assert_bit_exact(f"{tag} prev points L{l}", gp, op)
        assert_bit_exact(f"{tag} prev normals L{l}", gn, on)


def test_bench_shape_batched(oracle_mod):
    """The exact path bench.py times: 640x480, 5 mm, the default schedule,
    frames handed to tf_process_frames in device memory with the two-frame lookahead -- 36
    frames as three calls of 12, the state compared with the oracle run frame by frame after
    every call: counters, pose, the last frame's renderImage, the raycast, all ICP-map levels,
    and the whole scene at the end."""
    from parity_util import DeviceFrames
    g, o = make_pair(oracle_mod)
    n, chunk = 36, 12
    seq = synth.orbit_sequence(n, 640, 480, seed=7)
    dev = DeviceFrames(seq)
    fb = 640 * 480 * 2
    for c0 in range(0, n, chunk):
        okg = g.process_frames(dev.ptr + c0 * fb, chunk)
        oko = np.array([o(seq[k]) for k in range(c0, c0 + chunk)])
        assert np.array_equal(okg, oko), (c0, okg, oko)
        _compare_frame_state(g, o, f"frames {c0}..{c0 + chunk - 1}", grey=bool(oko[-1]))
    compare_scene(g, o, "bench-shape final")
    g.close()
    dev.free()


def test_bench_shape_one_batch(oracle_mod):
    """As test_bench_shape_batched, but 40 frames in ONE tf_process_frames call (two enqueue
    groups: the lookahead crosses the 32-frame group boundary), final state bit-exact."""
    from parity_util import DeviceFrames
    g, o = make_pair(oracle_mod)
    n = 40
    seq = synth.orbit_sequence(n, 640, 480, seed=7)
    dev = DeviceFrames(seq)
    okg = g.process_frames(dev.ptr, n)
    oko = np.array([o(seq[k]) for k in range(n)])
    assert np.array_equal(okg, oko), (okg, oko)
    _compare_frame_state(g, o, "one batch of 40", grey=bool(oko[-1]))
    compare_scene(g, o, "one batch final")
    g.close()
    dev.free()


def test_bench_timed_window(oracle_mod):
    """The bench's own C2 input and schedule over its WHOLE run (bench.py: 640x480, 5 mm, the
    GPU-rendered orbit of seed 7, 32-frame tf_process_frames steps, 5 warm-up + 20 timed steps =
    frames 0..799): the context runs the 25 steps exactly as the bench does, the OpenMP oracle runs
    them frame by frame; every frame's ok flag is equal, and the whole state -- counters, pose,
    range image, renderImage grey, raycast, all ICP-map levels, hash, visible list and voxels -- is
    bit-exact after frame 191 (the first timed step), 319 (the ping-pong's turn at -25 deg, frame
    300), 479, 639 (the turn at +25 deg, frame 500 + 100 = 600 -> 639's window) and 799 (the last
    timed frame)."""
    import bench
    from topfusion_amd import TopFu, default_params
    W, H, F, steps = 640, 480, 32, 25
    dev = bench.orbit_frames(steps * F, W, H, 7)
    fx, fy, cx, cy = synth.intrinsics(W, H)
    args = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy)
    g = TopFu(default_params(**args))
    o = oracle_mod.Oracle(oracle_mod.default_params(**args), omp=True)
    fb = W * H * 2
    n_reset = 0
    for step in range(steps):
        okg = g.process_frames(dev.ptr + step * F * fb, F)
        host = dev.download(step * F, F)
        oko = np.array([o(host[k]) for k in range(F)])
        assert np.array_equal(okg, oko), (step, okg, oko)
        n_reset += int((~oko).sum())
        if step in (5, 9, 14, 19, 24):
            tag = f"bench frames {step * F}..{(step + 1) * F - 1}"
            _compare_frame_state(g, o, tag, grey=bool(oko[-1]))
            compare_scene(g, o, tag)
    # the reference's frame-mixing resets: the oracle's own count over frames 0..799 of
    # this stream under the default (the reference's OpenCV 4) algebra, profiles/r05/pose_algebra_gap_C2.json
    assert n_reset == 79, n_reset
    g.close()
    dev.free()


def test_two_contexts_one_device(oracle_mod):
    """Two TopFu contexts in one process on one device (contexts share nothing; C4
    runs one per GPU, but nothing stops several per GPU): streams seeded 7 and 8, frames
    interleaved context by context, each context bit-exact with its own oracle after every
    frame."""
    g1, o1 = make_pair(oracle_mod, 320, 240)
    g2, o2 = make_pair(oracle_mod, 320, 240)
    s1 = synth.orbit_sequence(8, 320, 240, seed=7)
    s2 = synth.orbit_sequence(8, 320, 240, seed=8)
    for k in range(8):
        for g, o, s, name in ((g1, o1, s1, "ctx seed 7"), (g2, o2, s2, "ctx seed 8")):
            okg, oko = g(s[k]), o(s[k])
            assert okg == oko, f"{name} frame {k}: gpu {okg} oracle {oko}"
            sg, so = g.last_stats, o.counters()
            for key in ("lastFreeBlockId", "noVisibleEntries", "icp_iterations", "frame_counter", "n_resets"):
                assert sg[key] == so[key], f"{name} frame {k} {key}: gpu {sg[key]} oracle {so[key]}"
            assert_bit_exact(f"{name} frame {k} pose", g.getCameraPose()[:3, :4], o.pose())
    compare_scene(g1, o1, "ctx seed 7")
    compare_scene(g2, o2, "ctx seed 8")
    g1.close()
    g2.close()


def test_concurrent_contexts_one_device(oracle_mod):
    """Three contexts on one device driven at the same time from three host threads (C4's
    replicas, several per GPU): batched 320x240 streams seeded 7, 8 and 9 enqueued together, so
    their kernels interleave on the device -- the persistent ICP launches, which each need the
    whole chip, ordered across the contexts (tf_icp_order_*).  Each context bit-exact with its own
    oracle: per-frame ok flags, counters, final pose, raycast and scene."""
    import threading
    from parity_util import DeviceFrames
    from topfusion_amd import TopFu, default_params
    cols, rows, n = 320, 240, 24
    fx, fy, cx, cy = synth.intrinsics(cols, rows)
    args = dict(cols=cols, rows=rows, fx=fx, fy=fy, cx=cx, cy=cy)
    seeds = (7, 8, 9)
    seqs = [synth.orbit_sequence(n, cols, rows, seed=sd) for sd in seeds]
    ctxs = [TopFu(default_params(**args)) for _ in seeds]
    devs = [DeviceFrames(sq) for sq in seqs]
    res, errs = {}, []

    def run(i):
        try:
            res[i] = ctxs[i].process_frames(devs[i].ptr, n)
        except Exception as ex:                     # reported by the main thread
            errs.append(f"context {i}: {ex!r}")

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(seeds))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a context did not finish"
    assert not errs, errs
    for i, sd in enumerate(seeds):
        o = oracle_mod.Oracle(oracle_mod.default_params(**args))
        oko = np.array([o(seqs[i][k]) for k in range(n)])
        tag = f"concurrent ctx seed {sd}"
        assert np.array_equal(res[i], oko), (tag, res[i], oko)
        sg, so = ctxs[i].stats(), o.counters()
        for key in ("frame_counter", "n_resets", "icp_iterations"):
            assert sg[key] == so[key], f"{tag} {key}: gpu {sg[key]} oracle {so[key]}"
        assert_bit_exact(f"{tag} final pose", ctxs[i].getCameraPose()[:3, :4], o.pose())
        assert_bit_exact(f"{tag} final raycast", ctxs[i].raycast_result(), o.raycast_result())
        compare_scene(ctxs[i], o, tag)
    for g, d in zip(ctxs, devs):
        g.close()
        d.free()


def test_c3_capacity_top_block(oracle_mod):
    """The C3 bench capacity (2^21 - 1 voxel blocks = 4 GiB, 2^22 buckets, 2^20 excess) at C3
    geometry (1280x960, 2 mm): allocation hands out blocks from the top of the free list, so the
    first block of every scene is VBA block 2^21 - 2, the one whose voxels sit at the very end of
    the 32-bit byte-offset range the raycasts use (tf_render.hip vox_at).  Three tracked frames;
    raycast, grey image, ICP maps, poses and the whole scene bit-exact, with the top block
    allocated and in the last frame's visible set."""
    cols, rows = 1280, 960
    cap = dict(n_buckets=1 << 22, n_excess=1 << 20, n_blocks=(1 << 21) - 1, vis_capacity=1 << 21,
               max_render_blocks=1 << 20)
    g, o = make_pair(oracle_mod, cols, rows, voxelSize=0.002, **cap)
    seq = synth.orbit_sequence(3, cols, rows, seed=7)
    for k in range(3):
        okg, oko = g(seq[k]), o(seq[k])
        assert okg == oko, f"frame {k}: ok gpu {okg} oracle {oko}"
        sg, so = g.last_stats, o.counters()
        for key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries", "icp_iterations"):
            assert sg[key] == so[key], f"frame {k} {key}: gpu {sg[key]} oracle {so[key]}"
        assert_bit_exact(f"frame {k} pose", g.getCameraPose()[:3, :4], o.pose())
        if k > 0 and oko:
            assert_bit_exact(f"frame {k} renderImage grey", g.frame_grey(), o.frame_grey())
    _compare_frame_state(g, o, "C3 capacity", grey=False)
    h = g.hash()
    top = np.nonzero(h["ptr"] == cap["n_blocks"] - 1)[0]
    assert len(top) == 1, "the top VBA block is allocated"
    assert g.visible_type()[top[0]] > 0, "the top VBA block is in the visible state"
    compare_scene(g, o, "C3 capacity final")
    g.close()


def test_c5_random_walk_10mm(oracle_mod):
    """C5 geometry: 10 mm voxels (noSteps flips 1 <-> 2 at this size), the seed-13
    random walk (<= 1 cm / 0.5 deg per frame); every frame identical to the oracle, including
    the ICP-failure resets the reference's frame-mixing quirk produces away from the identity."""
    cols, rows, n = 320, 240, 14
    g, o = make_pair(oracle_mod, cols, rows, voxelSize=0.01)
    seq = synth.random_walk_sequence(n, cols, rows, seed=13)
    for k in range(n):
        okg, oko = g(seq[k]), o(seq[k])
        assert okg == oko, f"frame {k}: ok gpu {okg} oracle {oko}"
        sg, so = g.last_stats, o.counters()
        for key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries", "icp_iterations", "frame_counter",
                    "n_resets"):
            assert sg[key] == so[key], f"frame {k} {key}: gpu {sg[key]} oracle {so[key]}"
        assert_bit_exact(f"frame {k} pose", g.getCameraPose()[:3, :4], o.pose())
    compare_scene(g, o, "C5 final")
    assert_bit_exact("C5 final raycast", g.raycast_result(), o.raycast_result())


def test_render_image_types(oracle_mod):
    """The engine's five RenderImageType modes (VisualisationEngine.hpp:15-22; pixel stages
    VisualisationEngine_CUDA.cu:254-290) from the current pose after a tracked sequence, in an
    order where the alpha-preserving colour-from-normal mode follows each of the others."""
    g, o = make_pair(oracle_mod, 320, 240)
    seq = synth.orbit_sequence(6, 320, 240, seed=7)
    for k in range(6):
        assert g(seq[k]) == o(seq[k])
    lit = {}
    for t in (3, 0, 3, 1, 3, 4, 3, 2, 1, 4, 0):
        img_g, img_o = g.renderImage(t), o.render_image_type(t)
        assert_bit_exact(f"render type {t}", img_g, img_o)
        lit[t] = int((img_g[..., :3] > 0).any(-1).sum())
    assert all(v > 1000 for v in lit.values()), lit          # every mode renders the scene
