"""GPU parity of the free views' whole reading (tf_set_view_reading(TF_VIEW_WHOLE); TopFu.view(whole=True)) against
view_whole_ref.py's composition -- the oracle's view stages over the scene resolved across the VBA and the GlobalCache
-- bit for bit: the cases A-G over the tiered standard scene (their input conditions are asserted on the CPU,
tests/test_view_whole_ref.py), the maxW clamp, scenes without stored data (whole == resident, byte for byte), the
capacity and argument rules, a scene the swapping engine itself produced, the tracker's indifference, and the layers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import view_ref as V
import view_whole_ref as VW
from parity_util import assert_bit_exact
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWAPPING = dict(V.TABLES, use_swapping=1, swap_transfer_blocks=16)


def _lib():
    from topfusion_amd import _lib
    return _lib


def _ctx(**kw):
    from test_gpu_view import _ctx as ctx
    return ctx(**kw)


def _load(g, t):
    from test_gpu_mesh_whole import _load_two_tier
    _load_two_tier(g, t)


def _all_buffers(v, c2w, intr):
    """Every buffer a view holds after the staged calls from c2w: the list, the range image, the raycast result, the
    five image types, renderICP's maps and the stats."""
    from oracle import oracle as O
    w2c = O.rigid_inv(c2w)
    out = dict(n=v.find_visible(w2c, intr), ids=v.visible_ids())
    v.expected_depths(w2c, intr)
    out["range"] = v.range_image()
    out["stats"] = v.stats()
    v.raycast(c2w, intr)
    out["raycast"] = v.raycast_result()
    out["images"] = {t: v.shade(c2w, t, intr) for t in VW.TYPES}
    out["points"], out["normals"] = v.icp_maps(c2w, intr)
    return out


def _assert_stages(tag, got, ref):
    assert got["n"] == len(ref["ids"]), (tag, got["n"], len(ref["ids"]))
    assert got["stats"] == ref["stats"], (tag, got["stats"], ref["stats"])
    for k in ("ids", "range", "raycast", "points", "normals"):
        assert_bit_exact(f"{tag} {k}", got[k], ref[k])
    for t in VW.TYPES:
        assert_bit_exact(f"{tag} image type {t}", got["images"][t], ref["images"][t])


def _assert_one_call(tag, v, c2w, intr, ref):
    """tf_view_render on a fresh view.  (Types 4 and 0 write all four bytes of every pixel, so the reference's image --
    shaded over the earlier types -- is also a first render's.)"""
    for t in (4, 0):
        assert_bit_exact(f"{tag} one-call image type {t}", v.render(c2w, t, intr), ref["images"][t])
    assert_bit_exact(f"{tag} one-call list", v.visible_ids(), ref["ids"])
    assert_bit_exact(f"{tag} one-call range", v.range_image(), ref["range"])
    assert_bit_exact(f"{tag} one-call raycast", v.raycast_result(), ref["raycast"])
    assert v.stats() == ref["stats"]


@pytest.fixture(scope="module")
def tier_ctx():
    """One swapping context per scene (the tiered standard scene; its shifted twin of case G), made on demand."""
    made = {}

    def get(name):
        key = "G" if name == "G" else "A"
        if key not in made:
            made[key] = _ctx(tables=SWAPPING)
            _load(made[key], VW.scene_of(key))
        return made[key]
    yield get
    for g in made.values():
        g.close()


@pytest.mark.parametrize("name", sorted(VW.CASES))
def test_cases_staged_and_one_call(tier_ctx, name):
    """Every stage's buffers of a whole view, staged and as one call; set back to resident the same view gives the
    resident reference of the same buffers, and -- with the standard scene's hash and VBA back in the context --
    view_ref.case_reference."""
    L = _lib()
    g = tier_ctx(name)
    cols, rows, c2w, vp = VW.CASES[name]
    ref, res = VW.case_reference(name), VW.case_resident(name)
    intr = None if (cols, rows) == (V.W0, V.H0) else V.intr_of(cols)
    with g.view(cols, rows, whole=True, **vp) as v:
        assert v.whole
        _assert_stages(f"{name} whole", _all_buffers(v, c2w, intr), ref)
        with g.view(cols, rows, whole=True, **vp) as one:
            _assert_one_call(f"{name} whole", one, c2w, intr, ref)
        v.whole = False
        assert not v.whole
        _assert_stages(f"{name} resident again", _all_buffers(v, c2w, intr), res)
        if name in V.CASES:
            s, t = V.standard_scene(), VW.scene_of(name)
            g.upload(L.TF_BUF_HASH, s["hash"])
            g.upload(L.TF_BUF_VBA, s["vba"])
            try:
                _assert_stages(f"{name} resident, the standard scene", _all_buffers(v, c2w, intr), V.case_reference(name))
            finally:
                g.upload(L.TF_BUF_HASH, t["hash"])
                g.upload(L.TF_BUF_VBA, t["vba"])


def test_maxw_clamp():
    """CombineVoxelInformation's clamp is the context's maxW: case B on a context with maxW = 1."""
    cols, rows, c2w, vp = VW.CASES["B"]
    ref, ref100 = VW.case_reference("B", 1), VW.case_reference("B")
    assert not np.array_equal(ref["images"][4], ref100["images"][4]), "the confidence image does not show the clamp"
    g = _ctx(tables=dict(SWAPPING, maxW=1))
    _load(g, VW.tiered_scene())
    with g.view(cols, rows, whole=True) as v:
        _assert_stages("B at maxW 1", _all_buffers(v, c2w, V.intr_of(cols)), ref)
    g.close()


@pytest.mark.parametrize("swapping", [False, True])
def test_no_stored_data(swapping):
    """The standard scene with nothing stored: the whole reading is the resident one byte for byte in every buffer
    (and both are view_ref's); an empty map sees nothing."""
    from test_gpu_view import _put_scene
    g = _ctx(tables=SWAPPING if swapping else V.TABLES)
    with g.view(36, 28, whole=True) as v:
        assert not v.render(V.CASES["B"][2], 0, V.intr_of(36)).any() and v.stats()["noVisibleEntries"] == 0
    _put_scene(g, V.standard_scene())
    for name in ("A", "D"):
        cols, rows, c2w, vp = V.CASES[name]
        intr = None if (cols, rows) == (V.W0, V.H0) else V.intr_of(cols)
        with g.view(cols, rows, **vp) as r, g.view(cols, rows, whole=True, **vp) as w:
            a, b = _all_buffers(r, c2w, intr), _all_buffers(w, c2w, intr)
            assert w.whole and not r.whole
            _assert_stages(f"{name} whole, nothing stored", b, V.case_reference(name))
            for k in ("ids", "range", "raycast", "points", "normals"):
                assert a[k].tobytes() == b[k].tobytes(), (name, k)
            for t in VW.TYPES:
                assert a["images"][t].tobytes() == b["images"][t].tobytes(), (name, t)
            assert a["stats"] == b["stats"]
    g.close()


def test_capacity(tier_ctx, oracle_mod):
    """A list long enough for the resident reading and too short for the whole one."""
    from test_gpu_view import _same_state, _view_state
    L = _lib()
    g = tier_ctx("A")
    cols, rows, c2w, _ = VW.CASES["A"]
    ref, res = VW.case_reference("A"), VW.case_resident("A")
    n_res, n_whole = len(res["ids"]), len(ref["ids"])
    cap = (n_res + n_whole) // 2
    assert n_res < cap < n_whole
    with g.view(cols, rows, vis_capacity=cap) as v:
        assert_bit_exact("resident render", v.render(c2w, 0), res["images"][0])
        before = _view_state(v)
        assert before["stats"]["noVisibleEntries"] == n_res
        v.whole = True
        with pytest.raises(L.TfError) as e:
            v.render(c2w, 0)
        assert e.value.status == L.TF_CAPACITY
        _same_state("after a refused whole render", _view_state(v), before)
        with pytest.raises(L.TfError) as e:
            v.find_visible(oracle_mod.rigid_inv(c2w))
        assert e.value.status == L.TF_CAPACITY and v.needed == n_whole
        _same_state("after a refused whole find_visible", _view_state(v), before)
    with g.view(cols, rows, vis_capacity=n_whole, whole=True) as v:
        assert_bit_exact("exact capacity image", v.render(c2w, 0), ref["images"][0])
        assert_bit_exact("exact capacity list", v.visible_ids(), ref["ids"])


def test_arguments(tier_ctx):
    L, lib = _lib(), _lib().load()
    g = tier_ctx("A")
    r = ctypes.c_int(-1)
    with g.view(36, 28) as v:
        assert lib.tf_get_view_reading(v._h, ctypes.byref(r)) == L.TF_OK and r.value == L.TF_VIEW_RESIDENT
        for bad in (-1, 2, 7):
            assert lib.tf_set_view_reading(v._h, bad) == L.TF_INVALID_ARG
        assert lib.tf_get_view_reading(v._h, ctypes.byref(r)) == L.TF_OK and r.value == L.TF_VIEW_RESIDENT
        assert lib.tf_set_view_reading(None, L.TF_VIEW_WHOLE) == L.TF_INVALID_ARG
        assert lib.tf_get_view_reading(None, ctypes.byref(r)) == L.TF_INVALID_ARG
        assert lib.tf_get_view_reading(v._h, None) == L.TF_INVALID_ARG
        for want in (L.TF_VIEW_WHOLE, L.TF_VIEW_RESIDENT, L.TF_VIEW_WHOLE):
            assert lib.tf_set_view_reading(v._h, want) == L.TF_OK
            assert lib.tf_get_view_reading(v._h, ctypes.byref(r)) == L.TF_OK and r.value == want
        assert v.whole
        vp = L.TfViewParams()
        L.check(lib.tf_view_get_params(v._h, ctypes.byref(vp)), "tf_view_get_params")
        assert ctypes.sizeof(vp) == 16 and (vp.cols, vp.rows) == (36, 28)


# ---- a scene the swapping engine produced ---------------------------------------------------------------------
ENGINE_VIEWS = ((36, 28, 90), (164, 124, 180))          # cols, rows, yaw in degrees


def _engine_pose(deg):
    from test_gpu_swapping import _rt32, _yaw_pose
    return _rt32(*_yaw_pose(deg))


def test_engine_scene(oracle_mod):
    """test_gpu_mesh_whole's turning camera (VBA 128 blocks, 16 per transfer): whole views from yaw 90 and 180 deg are
    the reference's over the downloaded tiers and hit more than the resident reading; a twin context with no view
    calls -- some of them in mid-sequence -- is identical in all five buffers and in stats()."""
    from test_gpu_engines import Pitched, _f, _ok
    from test_gpu_mesh_whole import ENGINE, H, W, _ctx as mesh_ctx, _tiers, _turning_frames
    lib = _lib().load()
    frames = _turning_frames(oracle_mod)
    g, twin = mesh_ctx(**ENGINE), mesh_ctx(**ENGINE)
    intr = np.array(synth.intrinsics(W, H), np.float32)
    dists = Pitched(H, W, np.float32)
    views = [g.view(c, r, whole=True) for c, r, _ in ENGINE_VIEWS]
    for k, (dd, w2c) in enumerate(frames):
        dists.put(dd)
        for t in (g, twin):
            _ok(lib.tf_scene_alloc(t._h, _f(intr), _f(w2c), dists.ptr, dists.step, 0, 0), "tf_scene_alloc")
            _ok(lib.tf_scene_integrate(t._h, _f(intr), _f(w2c), dists.ptr, dists.step), "tf_scene_integrate")
            t.swap()
        if k in (len(frames) // 3, len(frames) // 2):             # in mid-sequence: the frames after must not see it
            for v, (c, r, deg) in zip(views, ENGINE_VIEWS):
                for ty in VW.TYPES:
                    v.render(_engine_pose(deg), ty, V.intr_of(c))
                v.icp_maps(_engine_pose(deg), V.intr_of(c))
    tiers = _tiers(g)
    h, _, _, flags, _ = tiers
    assert ((h["ptr"] == -1) & (flags == 1)).any()
    for v, (c, r, deg) in zip(views, ENGINE_VIEWS):
        c2w, vi = _engine_pose(deg), V.intr_of(c)
        want = VW.whole_stages(oracle_mod, tiers, c, r, c2w, tables=ENGINE, intr=vi)
        _assert_stages(f"engine {c}x{r}", _all_buffers(v, c2w, vi), want)
        with g.view(c, r, whole=True) as one:
            _assert_one_call(f"engine {c}x{r}", one, c2w, vi, want)
        res = VW.resident_stages(oracle_mod, tiers, c, r, c2w, tables=ENGINE, intr=vi)
        hits = [int((x["raycast"][..., 3] > 0).sum()) for x in (want, res)]
        print(f"engine {c}x{r} yaw {deg}: visible {len(want['ids'])} vs {len(res['ids'])}, hits {hits[0]} vs {hits[1]}")
        assert hits[0] > hits[1] and len(want["ids"]) > len(res["ids"])
    for name, a, b in zip(("hash", "vba", "swap state", "stored flags", "stored blocks"), _tiers(g), _tiers(twin)):
        assert a.tobytes() == b.tobytes(), f"{name}: the viewing context differs from its twin"
    assert g.stats() == twin.stats()
    dists.free()
    g.close()
    twin.close()


def test_whole_views_leave_a_swapping_tracker_alone(oracle_mod):
    """test_gpu_view's swapping twins with whole views rendered between the frames: equal in every buffer after every
    step, and the view's list is the reference's over both tiers."""
    from test_gpu_engines import Pitched, _f, _ok
    from test_gpu_mesh_whole import _tiers
    from test_gpu_view import _twins_equal
    import mesh_whole_ref as WR
    lib = _lib().load()
    O = oracle_mod
    W, H = V.W0, V.H0
    kw = dict(use_swapping=1, n_buckets=0x2000, n_excess=0x1000, n_blocks=700, swap_transfer_blocks=256, vis_capacity=0x3000,
              voxelSize=0.01, mu=0.04)
    a, b = _ctx(tables=kw), _ctx(tables=kw)
    intr = V.intr_of(W)
    dists = Pitched(H, W, np.float32)
    centre = np.array([0.15, -0.15, 0.6])
    view = b.view(100, 76, whole=True)
    ov = V.oracle_for(O, 100, 76, tables=kw)
    more = 0
    for k, deg in enumerate((0, 40, 80, 120, 80, 40, 0)):
        R = synth._rot_y(np.deg2rad(deg))
        w2c = O.rigid_inv(V.rt32(R, centre))
        dists.put(O.compute_dists(synth.render_depth(R, centre, W, H, noise_mm=1.0, seed=1000 + k, intr=tuple(float(x) for x in intr))))
        for g in (a, b):
            _ok(lib.tf_scene_alloc(g._h, _f(intr), _f(w2c), dists.ptr, dists.step, 0, 0), "tf_scene_alloc")
            _ok(lib.tf_scene_integrate(g._h, _f(intr), _f(w2c), dists.ptr, dists.step), "tf_scene_integrate")
            g.swap()
        c2w = V.rt32(synth._rot_y(np.deg2rad(deg - 60)), centre)
        for t in VW.TYPES:
            view.render(c2w, t, V.intr_of(100))
        view.icp_maps(c2w, V.intr_of(100))
        h, _, state, flags, _ = _tiers(b)
        h2 = h.copy()
        h2["ptr"] = np.where(WR.classify(h, state, flags) >= 0, 0, -2)
        want = V.visible_list(ov, h2, O.rigid_inv(c2w))
        assert_bit_exact(f"step {k} list over both tiers", view.visible_ids(), want)
        more += len(want) - len(V.visible_list(ov, h, O.rigid_inv(c2w)))
        _twins_equal(f"step {k}", a, b, swapping=True)
    assert more > 0, "no stored block was ever in the view's frustum"
    dists.free()
    a.close()
    b.close()


# ---- the layers -----------------------------------------------------------------------------------------------
def test_python_layer_equals_the_c_abi(tier_ctx):
    from test_gpu_engines import Pitched, _f, _ok
    L, lib = _lib(), _lib().load()
    g = tier_ctx("A")
    cols, rows, c2w, _ = VW.CASES["C"]
    intr = V.intr_of(cols)
    with g.view(cols, rows, whole=True) as v:
        py = v.render(c2w, 4, intr)
    vp = L.TfViewParams(cols, rows, 0, 0)
    h = ctypes.c_void_p()
    _ok(lib.tf_view_create(g._h, ctypes.byref(vp), ctypes.byref(h)), "tf_view_create")
    _ok(lib.tf_set_view_reading(h, L.TF_VIEW_WHOLE), "tf_set_view_reading")
    img = Pitched(rows, cols, np.uint8, 4)
    _ok(lib.tf_view_render(h, _f(intr), _f(c2w), 4, ctypes.c_void_p(img.ptr), img.step), "tf_view_render")
    assert_bit_exact("python whole render", py, img.get())
    assert_bit_exact("the reference's", py, VW.case_reference("C")["images"][4])
    lib.tf_view_destroy(h)
    img.free()


def test_view_whole_check_app(tmp_path, oracle_mod):
    """apps/view_whole_check fuses a turning camera into a swapping Scene through the C++ engine layer and renders a
    whole view through FindVisibleBlocks + RenderImage on a RenderState with setWhole(true): the PPM is the
    reference's image for the tiers the program dumps."""
    from topfusion_amd.topfu import HASH_DTYPE, VOXEL_DTYPE
    from test_gpu_view import _cv_affine, _demo_intr
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "apps"), "view_whole_check"], check=True)
    ppm, prefix = tmp_path / "whole.ppm", tmp_path / "tiers"
    r = subprocess.run([os.path.join(ROOT, "apps", "view_whole_check"), str(ppm), str(prefix)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda ext, dt: np.fromfile(str(prefix) + ext, dt)
    tiers = (rd(".hash", HASH_DTYPE), rd(".vba", VOXEL_DTYPE), rd(".state", np.uint8), rd(".flags", np.uint8), rd(".store", VOXEL_DTYPE))
    assert ((tiers[0]["ptr"] == -1) & (tiers[3] == 1)).any(), "the program's scene has no stored-only block"
    info = dict(line.split("=", 1) for line in r.stdout.split() if "=" in line)
    W, vc, vr = int(info["cols"]), int(info["view_cols"]), int(info["view_rows"])
    pose = tuple(float(x) for x in info["pose"].split(","))
    c2w = _cv_affine(pose[3:], pose[:3])
    ti = _demo_intr(W)
    sx, sy = np.float32(vc) / np.float32(W), np.float32(vr) / np.float32(int(info["rows"]))
    vi = np.array([ti[0] * sx, ti[1] * sy, ti[2] * sx, ti[3] * sy], np.float32)
    tables = dict(n_buckets=int(info["n_buckets"]), n_excess=int(info["n_excess"]), n_blocks=int(info["n_blocks"]),
                  vis_capacity=len(tiers[0]), voxelSize=float(info["voxel_size"]), mu=float(info["mu"]))
    want = VW.whole_stages(oracle_mod, tiers, vc, vr, c2w, tables=tables, intr=vi, types=(0,))["images"][0]
    res = VW.resident_stages(oracle_mod, tiers, vc, vr, c2w, tables=tables, intr=vi, types=(0,))["images"][0]
    assert int((want[..., 0] > 0).sum()) > int((res[..., 0] > 0).sum())
    assert ppm.read_bytes() == b"P6\n%d %d\n255\n" % (vc, vr) + np.ascontiguousarray(want[..., :3]).tobytes()


def test_demo_headless_view_whole(tmp_path):
    """demo_headless --view-out ... --view-whole over a saved map (TopFu::renderView(..., whole)): on a map without a
    GlobalCache the picture is the resident one, which is the Python render."""
    from topfusion_amd import TopFu, default_params
    from test_gpu_view import _cv_affine, _demo_intr
    apps = os.path.join(ROOT, "apps")
    subprocess.run(["make", "-s", "-C", apps, "demo_headless"], check=True)
    W, H, vc, vr = V.W0, V.H0, 84, 60
    fx, fy, cx, cy = (float(v) for v in _demo_intr(W))
    g = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy))
    seq = synth.orbit_sequence(3, W, H, seed=7)
    assert all(g(seq[k]) for k in range(3))
    scene = str(tmp_path / "scene.tfs")
    g.save_scene(scene)
    pose = (0.0625, -0.03125, 0.125, 0.0, -0.25, 0.0625)
    ti = _demo_intr(W)
    sx, sy = np.float32(vc) / np.float32(W), np.float32(vr) / np.float32(H)
    vi = np.array([ti[0] * sx, ti[1] * sy, ti[2] * sx, ti[3] * sy], np.float32)
    with g.view(vc, vr, whole=True) as v:
        img = v.render(_cv_affine(pose[3:], pose[:3]), 0, vi)
    g.close()
    assert int((img[..., 0] > 0).sum()) > 500
    want = b"P6\n%d %d\n255\n" % (vc, vr) + np.ascontiguousarray(img[..., :3]).tobytes()
    out = str(tmp_path / "demo.ppm")
    r = subprocess.run([os.path.join(apps, "demo_headless"), "--load-scene", scene, "--view-out", out, "--view-pose",
                        ",".join(repr(x) for x in pose), "--view-size", f"{vc}x{vr}", "--view-whole", "0", str(W), str(H)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "free view 84x60 written" in r.stdout, r.stdout + r.stderr
    assert open(out, "rb").read() == want
