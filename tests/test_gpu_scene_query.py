"""GPU parity of the scene queries (tf_scene_query / tf_scene_slice, include/tfusion_hip.h; TopFu.query / TopFu.slice),
bit for bit: against the reference's own outputs at the pin points (tests/golden/stage_pin_<scene>_sdf_read.bin -- the
first direct comparison of a HIP kernel with them), and against the oracle's per-point reads everywhere else.  The inputs
and their conditions are tests/scene_query_cases.py's (asserted on the CPU by tests/test_scene_query_cases.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pin_scenes as P
import scene_query_cases as Q
from parity_util import assert_bit_exact

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
SHAPES = dict(sdf_nearest=(np.float32, 1), entry=(np.int32, 1), sdf=(np.float32, 1), confidence=(np.float32, 1),
              normal=(np.float32, 3), colour=(np.uint8, 4))


def _lib():
    from topfusion_amd import _lib
    return _lib


def _assert_record(tag, got, want, keys=None):
    for k in (keys or want):
        assert_bit_exact(f"{tag} {k}", got[k], want[k])


# ---- raw calls over caller device buffers ---------------------------------------------------------------------------
class Dev:
    """A device buffer filled from a host array; get() downloads it."""
    def __init__(self, host):
        L = _lib()
        self.hip, self.host = L.hip_runtime(), np.ascontiguousarray(host)
        self.p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.p), ctypes.c_size_t(max(self.host.nbytes, 16))) == 0
        if self.host.nbytes:
            assert self.hip.hipMemcpy(self.p, self.host.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(self.host.nbytes), 1) == 0

    def get(self):
        out = np.empty_like(self.host)
        if out.nbytes:
            assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), self.p, ctypes.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        self.hip.hipFree(self.p)


def raw_query(g, pts, n, cap, outs, units=0, reading=0, slice_args=None, handle="ctx"):
    """tf_scene_query (or tf_scene_slice with slice_args = (o, u, v, cols, rows)) with the outputs named in `outs`,
    each a buffer of `cap` records pre-filled with the sentinel byte: (status, {name: the whole buffer afterwards})."""
    L = _lib()
    lib = L.load()
    bufs = {}
    for k in outs:
        dt, comp = SHAPES[k]
        bufs[k] = Dev(np.full(cap * comp * np.dtype(dt).itemsize, SENTINEL, np.uint8).view(dt).reshape(cap, comp))
    qo = L.TfQueryOut()
    for k, b in bufs.items():
        setattr(qo, k, b.p.value)
    h = g._h if handle == "ctx" else None
    dp = Dev(np.ascontiguousarray(pts, np.float32)) if pts is not None else None
    try:
        if slice_args is None:
            st = lib.tf_scene_query(h, dp.p if dp is not None else None, n, units, reading, ctypes.byref(qo))
        else:
            o, u, v, cols, rows = slice_args
            f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(ctypes.c_void_p)
            st = lib.tf_scene_slice(h, f(o), f(u), f(v), cols, rows, units, reading, ctypes.byref(qo))
        got = {k: b.get().reshape((cap,) + ((SHAPES[k][1],) if SHAPES[k][1] > 1 else ())) for k, b in bufs.items()}
    finally:
        for b in list(bufs.values()) + ([dp] if dp is not None else []):
            b.free()
    return st, got


def _untouched(a, start=0):
    return (a[start:].view(np.uint8) == SENTINEL).all()


# ---- the pin scenes ---------------------------------------------------------------------------------------------------
class Pin:
    def __init__(self, name, oracle_mod):
        from test_gpu_stage_pin import Ctx
        from test_oracle_stage_pin import oracle_params
        self.name, self.c = name, Ctx(name)
        self.g = self.c.g
        s = P.scene(name)
        self.o = oracle_mod.Oracle(oracle_mod.default_params(**oracle_params()))
        self.o.upload_hash(s["hash"])
        self.o.upload_vba(s["vba"], s["vba_rgb"])
        self.pts = P.sdf_points(name)
        self.want = Q.golden_expected(name)


@pytest.fixture(scope="module")
def pins(oracle_mod):
    """One context and one oracle per pin scene, made on demand."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Pin(name, oracle_mod)
        return made[name]
    yield get
    for p in made.values():
        p.g.close()


@pytest.fixture(params=P.SCENES)
def pin(request, pins):
    return pins(request.param)


@pytest.fixture
def sphere(pins):
    return pins("sphere")


def test_against_the_reference_goldens(pin):
    """1. The reference's own outputs at the 4096 pin points, voxel units: this fails without the feature."""
    got = pin.g.query(pin.pts, units="voxels", normals=True, colours=True)
    assert set(got) == set(Q.OUTS)
    _assert_record(pin.name, got, pin.want)


def test_sizes_and_outputs(pin):
    """2. Prefixes of n = 0, 1, 63, 64, 65, 255, 256, 257 points: the first n records are the golden's, everything past n
    keeps the sentinel; each output alone gives the bytes it has among all six."""
    L = _lib()
    cap = max(Q.SIZES) + 7
    for n in Q.SIZES:
        st, got = raw_query(pin.g, pin.pts[:max(n, 1)], n, cap, Q.OUTS)
        assert st == L.TF_OK, (n, st)
        for k in Q.OUTS:
            assert_bit_exact(f"{pin.name} n={n} {k}", got[k][:n], pin.want[k][:n])
            assert _untouched(got[k], n), (n, k)
        if n in (1, 65, 257):
            for k in Q.OUTS:
                st, one = raw_query(pin.g, pin.pts[:n], n, cap, (k,))
                assert st == L.TF_OK and one[k].tobytes() == got[k].tobytes(), (n, k)
    st, got = raw_query(pin.g, None, 0, cap, Q.OUTS)               # n == 0 needs no points
    assert st == L.TF_OK and all(_untouched(a) for a in got.values())


def test_metres(pin):
    """3. The same points in metres: the expected voxel coordinates are recomputed as the header states."""
    pm = Q.metre_points(pin.name)
    want = Q.expected(pin.o, Q.metres_to_voxels(pm, P.VOXEL_SIZE))
    got = pin.g.query(pm, units="m", normals=True, colours=True)
    _assert_record(f"{pin.name} metres", got, want)
    assert pin.g.params_.voxelSize == P.VOXEL_SIZE


def test_guard(sphere):
    """4. NaN, +-inf, +-3e9, +-262136 and the floats beyond it in each axis: nothing outside, the oracle's values inside."""
    pts, ok = Q.guard_points(sphere.name)
    want = Q.expected(sphere.o, pts)
    got = sphere.g.query(pts, units="voxels", normals=True, colours=True)
    _assert_record("guard", got, want)
    none = Q.nothing(int((~ok).sum()))
    for k in Q.OUTS:
        assert_bit_exact(f"guard, out of range: {k}", got[k][~ok], none[k])
    # in metres the guard sees the converted coordinates
    pm = (pts * P.VOXEL_SIZE).astype(np.float32)
    vox = Q.metres_to_voxels(pm, P.VOXEL_SIZE)
    _assert_record("guard, metres", sphere.g.query(pm, units="m", normals=True, colours=True), Q.expected(sphere.o, vox))
    # a slice that walks out of range along x: the same rule per pixel
    o, u, v = np.array([262100, 0, 100], np.float32), np.array([1.5, 0, 0], np.float32), np.array([0, 1, 0], np.float32)
    sp = Q.slice_points(o, u, v, 48, 3)
    assert Q.in_range(sp).any() and not Q.in_range(sp).all()
    got = sphere.g.slice(o, u, v, 48, 3, units="voxels", normals=True, colours=True)
    want = Q.expected(sphere.o, sp)
    for k in Q.OUTS:
        assert_bit_exact(f"guard, slice {k}", got[k].reshape(want[k].shape), want[k])


def test_outside_the_grid(oracle_mod):
    """5. Blocks beyond +-128 blocks, a chained pair there, swapped-out and missing blocks, mixed in every wave."""
    from topfusion_amd import TopFu, default_params
    from test_oracle_stage_pin import oracle_params
    L = _lib()
    s = Q.far_scene()
    pts, _ = Q.far_points()
    o = oracle_mod.Oracle(oracle_mod.default_params(**oracle_params()))
    o.upload_hash(s["hash"])
    o.upload_vba(s["vba"], s["vba_rgb"])
    want = Q.expected(o, pts)
    g = TopFu(default_params(**oracle_params()))
    try:
        g.upload(L.TF_BUF_HASH, s["hash"])
        g.upload(L.TF_BUF_VBA, s["vba"])
        g.upload(L.TF_BUF_VBA_RGB, s["vba_rgb"])
        g.set_counters(P.N_BLOCKS - 1 - len(s["blocks"]), s["last_excess"], 0)
        _assert_record("far scene", g.query(pts, units="voxels", normals=True, colours=True), want)
        _assert_record("far scene, whole on a context without swapping", g.query(pts, units="voxels", whole=True, normals=True), want,
                       keys=Q.OUTS[:5])
    finally:
        g.close()
    cls = Q.far_point_classes(pts)
    assert (want["entry"][cls == 1] >= 0).all() and (want["entry"][cls >= 2] == -1).all()


# ---- the whole reading --------------------------------------------------------------------------------------------------
def _swapping_ctx():
    import view_ref as V
    from test_gpu_view import _ctx
    return _ctx(tables=dict(V.TABLES, use_swapping=1, swap_transfer_blocks=16))


def test_whole_reading(oracle_mod):
    """6. The tiered standard scene: resident, stored-only, pending and face points against the oracle over the resolved
    scene; the resident reading of the same context against the oracle over the VBA alone; colour refused."""
    import view_ref as V
    import view_whole_ref as VW
    from test_gpu_mesh_whole import _load_two_tier, _tiers
    L = _lib()
    t = VW.tiered_scene()
    pts, cls = Q.whole_points()
    want = Q.expected(Q.whole_oracle(oracle_mod, t, V.TABLES, V.W0, V.H0), pts, colour=False)
    orr = V.oracle_for(oracle_mod, V.W0, V.H0)
    orr.upload_hash(t["hash"])
    orr.upload_vba(t["vba"], None)
    res = Q.expected(orr, pts, colour=False)
    g = _swapping_ctx()
    try:
        _load_two_tier(g, t)
        before = _tiers(g)
        _assert_record("whole", g.query(pts, units="voxels", whole=True, normals=True), want)
        _assert_record("resident on the tiered scene", g.query(pts, units="voxels", normals=True), res)
        pm = (pts * np.float32(V.TABLES["voxelSize"])).astype(np.float32)
        wm = Q.expected(Q.whole_oracle(oracle_mod, t, V.TABLES, V.W0, V.H0), Q.metres_to_voxels(pm, g.params_.voxelSize), colour=False)
        _assert_record("whole, metres", g.query(pm, units="m", whole=True, normals=True), wm)
        for n in (1, 65):                                       # a partial wave under the whole reading
            st, got = raw_query(g, pts[:n], n, 72, Q.OUTS[:5], reading=L.TF_VIEW_WHOLE)
            assert st == L.TF_OK
            for k in Q.OUTS[:5]:
                assert_bit_exact(f"whole n={n} {k}", got[k][:n], want[k][:n])
                assert _untouched(got[k], n)
        # a slice through the scene under both readings is the query on its points
        o = pts[0] - np.float32(20)
        u, v = np.array([1.25, 0.125, 0], np.float32), np.array([0, 0.75, 0.5], np.float32)
        sp = Q.slice_points(o, u, v, 37, 29)
        for whole in (True, False):
            a = g.slice(o, u, v, 37, 29, units="voxels", whole=whole, normals=True)
            b = g.query(sp, units="voxels", whole=whole, normals=True)
            for k in b:
                assert a[k].tobytes() == b[k].tobytes(), (whole, k)
        st, got = raw_query(g, pts[:8], 8, 8, Q.OUTS, reading=L.TF_VIEW_WHOLE)
        assert st == L.TF_INVALID_ARG and all(_untouched(a) for a in got.values())
        with pytest.raises(L.TfError) as e:
            g.query(pts[:8], units="voxels", whole=True, colours=True)
        assert e.value.status == L.TF_INVALID_ARG
        for name, a, b in zip(("hash", "vba", "swap state", "stored flags", "stored blocks"), before, _tiers(g)):
            assert a.tobytes() == b.tobytes(), f"{name} changed under the queries"
    finally:
        g.close()


@pytest.mark.parametrize("swapping", [False, True])
def test_whole_equals_resident_without_stored_data(swapping):
    """6. The untiered standard scene: whole == resident byte for byte, and nothing of the scene changes."""
    import view_ref as V
    from test_gpu_mesh_whole import _tiers
    from test_gpu_view import _ctx, _put_scene
    pts, _ = Q.whole_points()
    g = _swapping_ctx() if swapping else _ctx()
    try:
        _put_scene(g, V.standard_scene())
        before = _tiers(g) if swapping else (g.hash(), g.vba())
        a = g.query(pts, units="voxels", normals=True)
        b = g.query(pts, units="voxels", whole=True, normals=True)
        assert (a["entry"] >= 0).sum() >= Q.MIN_PER_CLASS
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        after = _tiers(g) if swapping else (g.hash(), g.vba())
        for x, y in zip(before, after):
            assert x.tobytes() == y.tobytes()
    finally:
        g.close()


# ---- slices ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["oblique", "axis"])
def test_slices(sphere, kind):
    """7. 4x4, 37x29 and 164x124 through the sphere: the slice is tf_scene_query on the numpy-generated points byte for
    byte, and the oracle's values."""
    for cols, rows in Q.SLICE_SIZES:
        for units in (("voxels", "m") if (cols, rows) == (37, 29) else ("voxels",)):
            o, u, v = Q.slice_plane(kind, cols, rows, units)
            sp = Q.slice_points(o, u, v, cols, rows)
            a = sphere.g.slice(o, u, v, cols, rows, units=units, normals=True, colours=True)
            b = sphere.g.query(sp, units=units, normals=True, colours=True)
            vox = sp if units == "voxels" else Q.metres_to_voxels(sp, P.VOXEL_SIZE)
            want = Q.expected(sphere.o, vox)
            for k in Q.OUTS:
                assert a[k].shape[:2] == (rows, cols)
                assert a[k].tobytes() == b[k].tobytes(), (kind, cols, rows, units, k)
                assert_bit_exact(f"{kind} {cols}x{rows} {units} {k}", b[k], want[k])
            if (cols, rows) == (164, 124):
                assert (want["confidence"] > 0).sum() > 100 and (want["entry"] == -1).sum() > 100


# ---- the tracker does not notice ------------------------------------------------------------------------------------------
def test_queries_leave_the_tracker_alone():
    """8. Two 36x28 contexts run the same frames per call (so a query meets a deferred frame tail); one also answers
    queries and a slice, both readings, between every two.  Verdicts, pose, hash, VBA, counters and every other buffer
    are equal after each frame."""
    import view_ref as V
    from test_gpu_view import TRACKER, _ctx, _twins_equal
    from topfusion_amd import synth
    n = 5
    seq = synth.orbit_sequence(n, 36, 28, seed=7)
    a, b = _ctx(36, 28, tables=TRACKER), _ctx(36, 28, tables=TRACKER)
    i = np.arange(700, dtype=np.int64)
    box = np.stack([P._h(181 + k, i) % np.uint32(4001) for k in range(3)], -1).astype(np.float64) / 2000 - 1        # [-1, 1] m
    pts = (box + np.array([0, 0, 1.0])).astype(np.float32)
    seen = 0
    try:
        for k in range(n):
            oka, okb = a(seq[k]), b(seq[k])
            assert oka == okb and (k > 0 or oka), (k, oka, okb)
            for whole in (False, True):
                r = b.query(pts, units="m", whole=whole, normals=True)
                seen += int((r["confidence"] > 0).sum())
                b.slice((-0.5, -0.4, 0.9), (0.025, 0, 0), (0, 0.025, 0.005), 41, 33, units="m", whole=whole, normals=True)
            _twins_equal(f"frame {k}", a, b)
        assert seen > 0, "no query point ever met the map"
    finally:
        a.close()
        b.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(sphere):
    """9. Every TF_INVALID_ARG of the header, with the outputs untouched."""
    from test_gpu_view import _ctx
    L = _lib()
    lib = L.load()
    g, pts = sphere.g, sphere.pts[:64]
    plane = (np.zeros(3, np.float32), np.array([1, 0, 0], np.float32), np.array([0, 1, 0], np.float32))

    def refused(tag, **kw):
        args = dict(g=g, pts=pts, n=64, cap=64, outs=Q.OUTS)
        args.update(kw)
        st, got = raw_query(**args)
        assert st == L.TF_INVALID_ARG, (tag, st)
        assert all(_untouched(a) for a in got.values()), tag

    refused("NULL ctx", handle=None)
    refused("NULL ctx, slice", handle=None, slice_args=plane + (8, 8))
    refused("NULL points", pts=None)
    refused("n < 0", n=-1)
    for bad in (-1, 2, 7):
        refused(f"units {bad}", units=bad)
        refused(f"reading {bad}", reading=bad)
        refused(f"slice units {bad}", units=bad, slice_args=plane + (8, 8))
        refused(f"slice reading {bad}", reading=bad, slice_args=plane + (8, 8))
    for cols, rows in ((0, 8), (8, 0), (-3, 8), (8, -3)):
        refused(f"slice {cols}x{rows}", slice_args=plane + (cols, rows))
    refused("slice NULL origin", slice_args=(None,) + plane[1:] + (8, 8))
    refused("colour under the whole reading", reading=L.TF_VIEW_WHOLE)
    # every output NULL, and a NULL tf_query_out
    d = Dev(pts)
    qo = L.TfQueryOut()
    assert lib.tf_scene_query(g._h, d.p, 64, 0, 0, ctypes.byref(qo)) == L.TF_INVALID_ARG
    assert lib.tf_scene_query(g._h, d.p, 64, 0, 0, None) == L.TF_INVALID_ARG
    assert lib.tf_scene_slice(g._h, *(a.ctypes.data_as(ctypes.c_void_p) for a in plane), 8, 8, 0, 0, ctypes.byref(qo)) == L.TF_INVALID_ARG
    d.free()
    # colour on a context without voxel_rgb
    plain = _ctx(36, 28)
    try:
        refused("colour without voxel_rgb", g=plain)
        st, got = raw_query(plain, pts, 64, 64, Q.OUTS[:5])
        assert st == L.TF_OK and not any(_untouched(a) for a in got.values())
        with pytest.raises(L.TfError):
            plain.query(pts, colours=True)
        with pytest.raises(L.TfError):
            plain.query(pts, units="mm")
    finally:
        plain.close()
    # the context still answers
    _assert_record("after the refusals", g.query(sphere.pts[:64], units="voxels", normals=True, colours=True),
                   {k: v[:64] for k, v in sphere.want.items()})


# ---- the demo ---------------------------------------------------------------------------------------------------------------
def test_demo_headless_slice(tmp_path):
    """demo_headless --slice-out over a saved map (TopFu::slice): the PGM is the host mapping of the Python slice."""
    from topfusion_amd import TopFu, default_params, synth
    from test_gpu_view import _demo_intr
    apps = os.path.join(ROOT, "apps")
    subprocess.run(["make", "-s", "-C", apps, "demo_headless"], check=True)
    W, H, sc, sr = 164, 124, 84, 60
    fx, fy, cx, cy = (float(v) for v in _demo_intr(W))
    g = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy))
    seq = synth.orbit_sequence(3, W, H, seed=7)
    assert all(g(seq[k]) for k in range(3))
    scene = str(tmp_path / "scene.tfs")
    g.save_scene(scene)
    plane = (-0.5, -0.375, 1.0, 0.0125, 0.0, 0.001, 0.0, 0.0125, 0.0005)
    r = g.slice(plane[:3], plane[3:6], plane[6:], sc, sr, units="m")
    g.close()
    grey = np.where(r["confidence"] == 0, 0, ((r["sdf"] + np.float32(1)) * np.float32(127.5)).astype(np.uint8)).astype(np.uint8)
    assert (r["confidence"] != 0).sum() > 100 and len(np.unique(grey)) > 10
    out = str(tmp_path / "slice.pgm")
    run = subprocess.run([os.path.join(apps, "demo_headless"), "--load-scene", scene, "--slice-out", out, "--slice-plane",
                          ",".join(repr(x) for x in plane), "--slice-size", f"{sc}x{sr}", "0", str(W), str(H)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and f"slice {sc}x{sr} written" in run.stdout, run.stdout + run.stderr
    assert open(out, "rb").read() == b"P5\n%d %d\n255\n" % (sc, sr) + grey.tobytes()
