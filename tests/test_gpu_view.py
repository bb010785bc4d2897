"""GPU parity of the free views (tf_view_*, include/tfusion_hip.h; TopFu.view): FindVisibleBlocks' list and every
stage of a view render against view_ref.py's composition of the oracle, bit for bit, over the standard scene and
the cases A-F whose input conditions test_view_ref.py asserts on the CPU; the capacity rule; colour; and the point
of the feature -- a context with view calls between its frames produces the frames of a twin without."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

import view_ref as V
from parity_util import DeviceFrames, assert_bit_exact
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

TYPES = (0, 1, 2, 3, 4)


def _lib():
    from topfusion_amd import _lib
    return _lib


def _ctx(cols=V.W0, rows=V.H0, tables=V.TABLES, **over):
    from topfusion_amd import TopFu, default_params
    fx, fy, cx, cy = (float(v) for v in V.intr_of(cols))
    kw = dict(tables)
    kw.update(over)
    return TopFu(default_params(cols=cols, rows=rows, fx=fx, fy=fy, cx=cx, cy=cy, **kw))


def _put_scene(g, s, vba_rgb=None):
    """The oracle-built scene into the GPU context (tf_upload + tf_set_counters): nothing is fused on the GPU."""
    L = _lib()
    ids = np.zeros(g.params_.vis_capacity, np.int32)
    ids[:len(s["visible_ids"])] = s["visible_ids"]
    g.upload(L.TF_BUF_HASH, s["hash"])
    g.upload(L.TF_BUF_VBA, s["vba"])
    if vba_rgb is not None:
        g.upload(L.TF_BUF_VBA_RGB, vba_rgb)
    g.upload(L.TF_BUF_ALLOC_LIST, s["alloc_list"])
    g.upload(L.TF_BUF_EXCESS_LIST, s["excess_list"])
    g.upload(L.TF_BUF_VISIBLE_IDS, ids)
    g.upload(L.TF_BUF_VISIBLE_TYPE, s["visible_type"])
    g.set_counters(*s["counters"])


@pytest.fixture(scope="module")
def scene_ctx():
    g = _ctx()
    _put_scene(g, V.standard_scene())
    yield g
    g.close()


def _view_state(v):
    return dict(ids=v._download(_lib().TF_VIEW_VISIBLE_IDS, np.int32, (v.vis_capacity,)), range=v.range_image(),
                raycast=v.raycast_result(), image=v.image(), stats=v.stats())


def _same_state(tag, a, b):
    for k in ("ids", "range", "raycast", "image"):
        assert_bit_exact(f"{tag} {k}", a[k], b[k])
    assert a["stats"] == b["stats"], (tag, a["stats"], b["stats"])


@pytest.mark.parametrize("name", sorted(V.CASES))
def test_staged_stages_and_one_call(scene_ctx, oracle_mod, name):
    """find_visible, expected_depths, raycast, shade (all five types), icp_maps one at a time over pitched caller
    buffers, each stage's buffers against view_ref; tf_view_render in one call equals the staged result."""
    from test_gpu_engines import Pitched, _f, _ok
    L, lib = _lib(), _lib().load()
    g = scene_ctx
    cols, rows, c2w, vp = V.CASES[name]
    ref = V.case_reference(name)
    w2c = oracle_mod.rigid_inv(c2w)
    intr = None if (cols, rows) == (V.W0, V.H0) else V.intr_of(cols)      # NULL: the context's
    ip = None if intr is None else _f(intr)
    with g.view(cols, rows, **vp) as v:
        assert v.vis_capacity == g.n_total and v.max_render_blocks == vp.get("max_render_blocks", g.params_.max_render_blocks)
        n = v.find_visible(w2c, intr)
        assert n == len(ref["ids"]) == v.stats()["noVisibleEntries"], (n, len(ref["ids"]))
        assert_bit_exact(f"{name} visible list", v.visible_ids(), ref["ids"])
        v.expected_depths(w2c, intr)
        assert_bit_exact(f"{name} range image", v.range_image(), ref["range"])
        assert v.stats() == ref["stats"], (v.stats(), ref["stats"])
        v.raycast(c2w, intr)
        assert_bit_exact(f"{name} raycast result", v.raycast_result(), ref["raycast"])
        img = Pitched(rows, cols, np.uint8, 4)
        for t in TYPES:
            _ok(lib.tf_view_shade(v._h, ip, _f(c2w), t, ctypes.c_void_p(img.ptr), img.step), "tf_view_shade")
            assert_bit_exact(f"{name} shade type {t} (caller buffer)", img.get(), ref["images"][t])
            assert_bit_exact(f"{name} shade type {t} (view image)", v.image(), ref["images"][t])
        pts, nrm = Pitched(rows, cols, np.float32, 4), Pitched(rows, cols, np.float32, 4)
        _ok(lib.tf_view_icp_maps(v._h, ip, _f(c2w), ctypes.c_void_p(pts.ptr), pts.step, ctypes.c_void_p(nrm.ptr), nrm.step),
            "tf_view_icp_maps")
        assert_bit_exact(f"{name} icp points", pts.get(), ref["points"])
        assert_bit_exact(f"{name} icp normals", nrm.get(), ref["normals"])
        for b in (img, pts, nrm):
            b.free()
        with g.view(cols, rows, **vp) as one:
            got = one.render(c2w, 0, intr)
            assert_bit_exact(f"{name} one-call image", got, ref["images"][0])
            assert_bit_exact(f"{name} one-call list", one.visible_ids(), ref["ids"])
            assert_bit_exact(f"{name} one-call range", one.range_image(), ref["range"])
            assert_bit_exact(f"{name} one-call raycast", one.raycast_result(), ref["raycast"])
            assert one.stats() == ref["stats"]


def test_capacity(scene_ctx, oracle_mod):
    """One entry short: TF_CAPACITY, the number needed, and the view as the preceding smaller render left it."""
    L = _lib()
    g = scene_ctx
    cols, rows, c2w, _ = V.CASES["A"]
    ref = V.case_reference("A")
    need = len(ref["ids"])
    other = V.rt32(*synth.orbit_pose(-80))
    with g.view(cols, rows, vis_capacity=need - 1) as v:
        v.render(other, 0)
        before = _view_state(v)
        assert 0 < before["stats"]["noVisibleEntries"] < need
        with pytest.raises(L.TfError) as e:
            v.render(c2w, 0)
        assert e.value.status == L.TF_CAPACITY
        _same_state("after a refused render", _view_state(v), before)
        with pytest.raises(L.TfError) as e:
            v.find_visible(oracle_mod.rigid_inv(c2w))
        assert e.value.status == L.TF_CAPACITY and v.needed == need
        _same_state("after a refused find_visible", _view_state(v), before)
    with g.view(cols, rows, vis_capacity=need) as v:
        assert_bit_exact("exact capacity image", v.render(c2w, 0), ref["images"][0])
        assert_bit_exact("exact capacity list", v.visible_ids(), ref["ids"])


def test_colour_from_volume(oracle_mod):
    """A voxel_rgb context: RENDER_COLOUR_FROM_VOLUME through a view of another size from a pose off the fused ones."""
    O = oracle_mod
    W, H = V.W0, V.H0
    o = V.oracle_for(O, W, H, voxel_rgb=1)
    intr = tuple(float(x) for x in V.intr_of(W))
    for k in (0, 24):
        R, t = synth.orbit_pose(k)
        w2c = O.rigid_inv(V.rt32(R, t))
        d = O.compute_dists(synth.render_depth(R, t, W, H, noise_mm=1.0, seed=300 + k, intr=intr))
        for _ in range(40):
            o.alloc(w2c, d)
        o.integrate(w2c, d, synth.render_colour(R, t, W, H, intr=intr))
    c = o.counters()
    s = dict(hash=o.hash(), vba=o.vba(), alloc_list=o.alloc_list(), excess_list=o.excess_list(), visible_ids=o.visible_ids(),
             visible_type=o.visible_type(), counters=(c["lastFreeBlockId"], c["lastFreeExcessListId"], c["noVisibleEntries"]))
    rgb = o.vba_rgb()
    assert int(((rgb >> 24) > 0).sum()) > 1000
    g = _ctx(voxel_rgb=1)
    _put_scene(g, s, rgb)
    cols, rows = 100, 76
    c2w = V.rt32(*synth.orbit_pose(-40))
    ov = V.oracle_for(O, cols, rows, voxel_rgb=1)
    want = V.render(O, ov, s["hash"], s["vba"], rgb, s["counters"], c2w, 2)[2]
    assert (want[..., 3] == 255).mean() > 0.2
    with g.view(cols, rows) as v:
        assert_bit_exact("colour from volume", v.render(c2w, 2, V.intr_of(cols)), want)
    g.close()


# ---- non-interference -----------------------------------------------------------------------------------
TRACKER = dict(n_buckets=0x10000, n_excess=0x4000, n_blocks=0x8000, vis_capacity=0x10000)


def _ctx_buffers(g, swapping=False):
    L = _lib()
    out = {}
    for name in ("HASH", "VBA", "VISIBLE_IDS", "VISIBLE_TYPE", "RANGE", "RAYCAST", "DISTS", "GREY", "ALLOC_LIST", "EXCESS_LIST"):
        out[name] = g.download(getattr(L, "TF_BUF_" + name))
    # (the depth pyramid of a context that ran no frame was never written: the engine path of the swapping twins)
    for name in ("CURR_POINTS", "CURR_NORMALS", "PREV_POINTS", "PREV_NORMALS") + (() if swapping else ("DEPTH",)):
        for l in range(3):
            out[f"{name}{l}"] = g.download(getattr(L, "TF_BUF_" + name), l)
    if swapping:
        for name in ("SWAP_STATE", "SWAP_STORED_FLAGS", "SWAP_STORED"):
            out[name] = g.download(getattr(L, "TF_BUF_" + name))
    out["stats"] = g.stats()
    out["pose"] = g.getCameraPose()
    return out


def _twins_equal(tag, a, b, swapping=False):
    sa, sb = _ctx_buffers(a, swapping), _ctx_buffers(b, swapping)
    assert sa["stats"] == sb["stats"], (tag, sa["stats"], sb["stats"])
    for k in sa:
        if k != "stats":
            assert_bit_exact(f"{tag} {k}", sb[k], sa[k])


OFF_TRACK = [V.rt32(*synth.orbit_pose(k)) for k in (-80, 60)] + [V._look_back()]


def _render_all(v, poses=OFF_TRACK):
    n = 0
    for c2w in poses:
        for t in TYPES:
            v.render(c2w, t, V.intr_of(v.W))
        n += v.stats()["noVisibleEntries"]
        v.icp_maps(c2w)
    return n


@pytest.mark.parametrize("batched", [False, True])
def test_views_leave_the_tracker_alone(batched):
    """Two contexts run the same 6 tracked frames; one of them also renders through views of other sizes from
    off-track poses between the frames (two views from frame 3 on, one of them destroyed again).  After every
    frame (every batch of two) the twins are equal in every buffer, the counters, the pose and the frame's image."""
    n = 6
    seq = synth.orbit_sequence(n, V.W0, V.H0, seed=7)
    a, b = _ctx(tables=TRACKER), _ctx(tables=TRACKER)
    dev = DeviceFrames(seq)
    small = b.view(36, 28)
    big, seen = None, 0
    step = 2 if batched else 1
    for k in range(0, n, step):
        if batched:
            oka = a.process_frames(dev.ptr + k * V.W0 * V.H0 * 2, step)
            okb = b.process_frames(dev.ptr + k * V.W0 * V.H0 * 2, step)
        else:
            oka, okb = [a(dev.ptr + k * V.W0 * V.H0 * 2)], [b(dev.ptr + k * V.W0 * V.H0 * 2)]
        assert list(oka) == list(okb) and (k > 0 or oka[0]), (k, oka, okb)
        for v in (small, big):
            if v is not None:
                seen += _render_all(v)
        if k + step == 4:                       # after frame 3: the second view, every type, one view destroyed
            big = b.view(324, 244)
            seen += _render_all(big)
            if small is not None:
                small.close()
                small = None
        _twins_equal(f"frame {k + step - 1}", a, b)
    assert seen > 0 and big is not None and small is None
    dev.free()
    a.close()
    b.close()


def test_views_leave_a_swapping_tracker_alone(oracle_mod):
    """The same on a swapping context with a VBA too small for the room (the engine path with the swapping engine
    at ground-truth poses).  The view's list is view_ref's over the downloaded hash: entries swapped out are absent."""
    from test_gpu_engines import Pitched, _f, _ok
    L, lib = _lib(), _lib().load()
    O = oracle_mod
    W, H = V.W0, V.H0
    kw = dict(use_swapping=1, n_buckets=0x2000, n_excess=0x1000, n_blocks=700, swap_transfer_blocks=256, vis_capacity=0x3000,
              voxelSize=0.01, mu=0.04)
    a, b = _ctx(tables=kw), _ctx(tables=kw)
    intr = V.intr_of(W)
    dists = Pitched(H, W, np.float32)
    centre = np.array([0.15, -0.15, 0.6])
    view = b.view(100, 76)
    ov = V.oracle_for(O, 100, 76, tables=kw)
    absent = 0
    for k, deg in enumerate((0, 40, 80, 120, 80, 40, 0)):
        R = synth._rot_y(np.deg2rad(deg))
        w2c = O.rigid_inv(V.rt32(R, centre))
        dists.put(O.compute_dists(synth.render_depth(R, centre, W, H, noise_mm=1.0, seed=1000 + k, intr=tuple(float(x) for x in intr))))
        for g in (a, b):
            _ok(lib.tf_scene_alloc(g._h, _f(intr), _f(w2c), dists.ptr, dists.step, 0, 0), "tf_scene_alloc")
            _ok(lib.tf_scene_integrate(g._h, _f(intr), _f(w2c), dists.ptr, dists.step), "tf_scene_integrate")
            g.swap()
        c2w = V.rt32(synth._rot_y(np.deg2rad(deg - 60)), centre)
        for t in TYPES:
            view.render(c2w, t, V.intr_of(100))
        h = b.hash()
        want = V.visible_list(ov, h, O.rigid_inv(c2w))
        assert_bit_exact(f"step {k} list over the resident tier", view.visible_ids(), want)
        gone = h[h["ptr"] == -1]
        if len(gone):
            pos = np.stack([gone["x"], gone["y"], gone["z"]], axis=1).astype(np.int16)
            absent += int((ov.block_visibility(O.rigid_inv(c2w), pos)[0] != 0).sum())
        _twins_equal(f"step {k}", a, b, swapping=True)
    assert absent > 0, "no swapped-out block was ever in the view's frustum"
    dists.free()
    a.close()
    b.close()


def test_map_changes_under_a_view():
    """Render, tf_reset: the next render is the empty one.  tf_scene_load of the scene's checkpoint: case A's again.
    tf_map_load_resized into a context with another n_excess (5008: tf_create wants n_buckets + n_excess to be a
    multiple of 16): the same picture from a different list."""
    cols, rows, c2w, _ = V.CASES["A"]
    ref, empty = V.case_reference("A"), V.case_reference("E")
    s = V.standard_scene()
    g = _ctx()
    _put_scene(g, s)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene.tfs")
        g.save_scene(path)
        v = g.view(cols, rows)
        small = g.view(*V.CASES["E"][:2])
        assert_bit_exact("before", v.render(c2w, 0), ref["images"][0])
        g.reset()
        assert not v.render(c2w, 0).any() and v.stats()["noVisibleEntries"] == 0
        assert not small.render(c2w, 0, V.intr_of(small.W)).any()
        assert_bit_exact("after tf_reset: the empty range image", small.range_image(), empty["range"])
        g.load_scene(path)
        assert_bit_exact("after tf_scene_load", v.render(c2w, 0), ref["images"][0])
        assert_bit_exact("after tf_scene_load: list", v.visible_ids(), ref["ids"])
        g.close()
        r = _ctx(n_excess=5008)
        rv = r.view(cols, rows)
        r.load_map_resized(path)
        assert_bit_exact("resized: image", rv.render(c2w, 0), ref["images"][0])
        assert_bit_exact("resized: raycast", rv.raycast_result(), ref["raycast"])
        ids = rv.visible_ids()
        assert len(ids) == len(ref["ids"]) and not np.array_equal(ids, ref["ids"])
        r.close()


def test_two_views_are_independent_and_destroy_releases_them(scene_ctx):
    g = scene_ctx
    (ca, ra, pa, _), (cb, rb, pb, _) = V.CASES["A"], V.CASES["B"]
    wa, wb = V.case_reference("A"), V.case_reference("B")
    va, vb = g.view(ca, ra), g.view(cb, rb)
    for order in ((va, vb), (vb, va), (va, vb)):
        for v in order:
            if v is va:
                assert_bit_exact("view A", v.render(pa, 0), wa["images"][0])
            else:
                assert_bit_exact("view B", v.render(pb, 0, V.intr_of(cb)), wb["images"][0])
        assert_bit_exact("A's raycast after B rendered", va.raycast_result(), wa["raycast"])
        assert_bit_exact("B's list after A rendered", vb.visible_ids(), wb["ids"])
    va.close()
    vb.close()
    h = _ctx()
    live = [h.view(36, 28), h.view(324, 244)]
    live[0].render(pa, 0)
    h.close()                                   # tf_destroy with two live views
    assert all(v._h is None for v in live)
    live[0].close()
    with pytest.raises(RuntimeError):
        live[1].render(pa, 0)


def test_python_layer_equals_the_c_abi(scene_ctx):
    """TopFu.view(...).render against tf_view_render into a pitched caller buffer."""
    from test_gpu_engines import Pitched, _f, _ok
    lib = _lib().load()
    g = scene_ctx
    cols, rows, c2w, _ = V.CASES["C"]
    intr = V.intr_of(cols)
    with g.view(cols, rows) as v:
        py = v.render(c2w, 4, intr)
    vp = _lib().TfViewParams(cols, rows, 0, 0)
    h = ctypes.c_void_p()
    _ok(lib.tf_view_create(g._h, ctypes.byref(vp), ctypes.byref(h)), "tf_view_create")
    img = Pitched(rows, cols, np.uint8, 4)
    _ok(lib.tf_view_render(h, _f(intr), _f(c2w), 4, ctypes.c_void_p(img.ptr), img.step), "tf_view_render")
    assert_bit_exact("python render", py, img.get())
    lib.tf_view_destroy(h)
    img.free()
    bad = _lib().TfViewParams(38, 28, 0, 0)
    assert lib.tf_view_create(g._h, ctypes.byref(bad), ctypes.byref(h)) == _lib().TF_INVALID_ARG


# ---- the C++ layers ---------------------------------------------------------------------------------------
def _demo_intr(cols):
    """The intrinsics the C++ apps give a cols-wide context: Intr(504.261f * s, ...) with s = cols / 640.0 a double."""
    return np.array([np.float32(float(np.float32(v)) * (cols / 640.0)) for v in (504.261, 503.905, 352.457, 272.202)], np.float32)


def _cv_affine(rvec, t):
    """cv::Affine3f(rvec, t) as include/tfusion/types.hpp forms it: Rodrigues in double (libm's sin / cos), then float."""
    libm = ctypes.CDLL("libm.so.6")
    for f in (libm.sin, libm.cos, libm.sqrt):
        f.argtypes, f.restype = [ctypes.c_double], ctypes.c_double
    rx, ry, rz = (float(np.float32(x)) for x in rvec)
    th = libm.sqrt(rx * rx + ry * ry + rz * rz)
    m = np.zeros((3, 4), np.float32)
    c, s = libm.cos(th), libm.sin(th)
    c1 = 1.0 - c
    r = (rx / th, ry / th, rz / th)
    rx_ = ((0.0, -r[2], r[1]), (r[2], 0.0, -r[0]), (-r[1], r[0], 0.0))
    for i in range(3):
        for j in range(3):
            m[i, j] = np.float32(c * (1.0 if i == j else 0.0) + c1 * (r[i] * r[j]) + s * rx_[i][j])
    m[:, 3] = np.asarray(t, np.float32)
    return m


def test_cpp_layers_write_the_python_render(tmp_path):
    """apps/view_check (FindVisibleBlocks + CreateExpectedDepths + RenderImage with a RenderState_VH of another size;
    TopFu::renderView) and demo_headless --view-out over a saved map: their PPM bytes are the Python render's."""
    import subprocess
    from topfusion_amd import TopFu, default_params
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    apps = os.path.join(root, "apps")
    subprocess.run(["make", "-s", "-C", apps], check=True)
    W, H, vc, vr = V.W0, V.H0, 84, 60
    fx, fy, cx, cy = (float(v) for v in _demo_intr(W))
    g = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy))
    seq = synth.orbit_sequence(3, W, H, seed=7)
    assert all(g(seq[k]) for k in range(3))
    scene = str(tmp_path / "scene.tfs")
    g.save_scene(scene)
    pose = (0.0625, -0.03125, 0.125, 0.0, -0.25, 0.0625)          # tx, ty, tz, rx, ry, rz: exact in float
    c2w = _cv_affine(pose[3:], pose[:3])
    ti = _demo_intr(W)
    sx, sy = np.float32(vc) / np.float32(W), np.float32(vr) / np.float32(H)
    vi = np.array([ti[0] * sx, ti[1] * sy, ti[2] * sx, ti[3] * sy], np.float32)
    with g.view(vc, vr) as v:
        img = v.render(c2w, 0, vi)
    g.close()
    assert int((img[..., 0] > 0).sum()) > 500
    want = b"P6\n%d %d\n255\n" % (vc, vr) + np.ascontiguousarray(img[..., :3]).tobytes()
    pose_arg = ",".join(repr(x) for x in pose)
    e, t, d = (str(tmp_path / n) for n in ("engine.ppm", "topfu.ppm", "demo.ppm"))
    r = subprocess.run([os.path.join(apps, "view_check"), scene, str(W), str(H), str(vc), str(vr), pose_arg, e, t],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "engine == topfu: yes" in r.stdout, r.stdout + r.stderr
    assert open(e, "rb").read() == want, "FindVisibleBlocks + RenderImage through a RenderState_VH"
    assert open(t, "rb").read() == want, "TopFu::renderView"
    r = subprocess.run([os.path.join(apps, "demo_headless"), "--load-scene", scene, "--view-out", d, "--view-pose", pose_arg,
                        "--view-size", f"{vc}x{vr}", "0", str(W), str(H)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "free view 84x60 written" in r.stdout, r.stdout + r.stderr
    assert open(d, "rb").read() == want, "demo_headless --view-out"
