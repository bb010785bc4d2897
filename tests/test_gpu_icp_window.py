"""The persistent ICP's det check in the solve's window under the OpenCV algebras: the
check of iteration k runs beside solve k and is settled at the iteration's closing barrier.
Everything the launch records -- affine, the 27 sums, iterations, ok, and for frames the pose --
bit for bit against the oracle, on the persistent schedule and on the per-iteration one.

* A det failure at every position the control flow distinguishes (iteration 0, the middle of a
  level, the last iteration of a level, the first iteration of the next level, the last iteration
  of the launch), through tf_icp_estimate on the caller pyramids of tests/icp_window_cases.py
  (96 x 72, 3 + 3 + 3 iterations).  The oracle classifies the cases
  (tests/test_icp_window_cases.py asserts on the CPU that every position has one); the seeds
  below were found by running it over seeds 0..399 of the family (failures at iterations 0..8:
  100, 1, 5, 79, 33, 12, 72, 9, 5 cases under opencv4, 98, 2, 6, 79, 33, 11, 70, 9, 3 under
  opencv2; the rest run all nine).
* Slot ownership that changes between levels: 352 x 200 (275 / 78 / 21 CTAs: waves 1.. own a
  slot at level 0 only, most workgroups none at the coarse levels, ragged right and bottom
  tiles) and 80 x 60 (every level under 256 CTAs), four tracked frames each.
* The status paths: a lost peer reported at the last iteration of a level, and the frames a
  halted context skips."""
import ctypes

import numpy as np
import pytest

import icp_window_cases as C
from parity_util import DeviceFrames, assert_bit_exact
from test_gpu_engines import Pitched
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

SEEDS = (2, 54, 336, 64, 0, 8, 72, 1, 20, 78, 212, 10)
ALGEBRAS = ("opencv4", "opencv2")
SCHEDULES = ("persistent", "per_iteration")


@pytest.fixture
def cv_oracle(oracle_mod):
    yield oracle_mod
    oracle_mod.set_pose_algebra("opencv4")


_cases = {}


def _case(seed):
    if seed not in _cases:
        _cases[seed] = C.make_case(seed)
    return _cases[seed]


_expected = {}


def _expect(oracle_mod, algebra):
    """The oracle's estimateTransform on every case, once per algebra."""
    if algebra not in _expected:
        oracle_mod.set_pose_algebra(algebra, libm=False)
        _expected[algebra] = {s: C.oracle_estimate(oracle_mod, *_case(s)) for s in SEEDS}
    return _expected[algebra]


def _ctx(algebra, schedule, monkeypatch, W, H, intr=None, **env):
    from topfusion_amd import TopFu, default_params
    monkeypatch.setenv("TFUSION_ICP_PERSISTENT", "0" if schedule == "per_iteration" else "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fx, fy, cx, cy = intr if intr is not None else synth.intrinsics(W, H)
    g = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy))
    g.set_pose_algebra(algebra)
    assert g.icp_persistent() == (schedule == "persistent")
    return g


def _icp_result(g):
    from topfusion_amd import _lib
    aff, sums = np.zeros(12, np.float32), np.zeros(27, np.float32)
    ok, n = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().tf_icp_get_result(g._h, aff.ctypes.data_as(ctypes.c_void_p), sums.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.byref(ok), ctypes.byref(n)), "tf_icp_get_result")
    return aff, sums, ok.value, n.value


class _Pyramids:
    """A case's maps in pitched device buffers, as tf_icp_estimate takes them."""

    def __init__(self, curr, prev):
        from topfusion_amd import _lib
        self.bufs = []
        self.cl, self.pl = (_lib.TfMapLevel * 3)(), (_lib.TfMapLevel * 3)()
        for l in range(3):
            h, w = curr[l][0].shape[:2]
            for arr, lev, field in ((curr[l][0], self.cl, "points"), (curr[l][1], self.cl, "normals"),
                                    (prev[l][0], self.pl, "points"), (prev[l][1], self.pl, "normals")):
                b = Pitched(h, w, np.float32, 4).put(arr)
                self.bufs.append(b)
                setattr(lev[l], field, b.ptr)
                setattr(lev[l], field + "_step", b.step)

    def free(self):
        for b in self.bufs:
            b.free()


def _estimate(g, pyr):
    """-> the call's status, and its (affine, ok, iterations) outputs."""
    from topfusion_amd import _lib
    intr = np.array([float(v) for v in C.intrinsics(0)], np.float32)
    aff = np.zeros(12, np.float32)
    ok, n = ctypes.c_int(), ctypes.c_int()
    st = _lib.load().tf_icp_estimate(g._h, intr.ctypes.data_as(ctypes.c_void_p), pyr.cl, pyr.pl, 3,
                                     aff.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ok), ctypes.byref(n))
    return st, aff, ok.value, n.value


def _set_params(g):
    from topfusion_amd import _lib
    it = (ctypes.c_int * 4)(*C.ITERS)
    _lib.check(_lib.load().tf_icp_set_params(g._h, C.DIST, float(C.ANGLE), it), "tf_icp_set_params")


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("algebra", ALGEBRAS)
def test_det_failure_positions(cv_oracle, monkeypatch, algebra, schedule):
    from topfusion_amd import _lib
    exp = _expect(cv_oracle, algebra)
    intr = [float(v) for v in C.intrinsics(0)]
    g = _ctx(algebra, schedule, monkeypatch, C.W, C.H, intr)
    _set_params(g)
    for seed in SEEDS:
        ook, on, oaff, osums = exp[seed]
        pyr = _Pyramids(*_case(seed))
        st, aff, ok, n = _estimate(g, pyr)
        tag = f"{algebra} {schedule} seed {seed} ({'ok' if ook else C.CLASSES[C.position(on)]})"
        assert st == _lib.TF_OK, tag
        assert (bool(ok), n) == (ook, on), (tag, ok, n, ook, on)
        assert_bit_exact(tag + " affine", aff, oaff)
        raff, rsums, rok, rn = _icp_result(g)
        assert (rok, rn) == (int(ook), on), tag
        assert_bit_exact(tag + " state affine", raff, oaff)
        assert_bit_exact(tag + " sums", rsums, osums)
        pyr.free()
    g.close()


def _frame_maps(o, oracle_mod, frame, W, H):
    """The current maps estimateTransform sees for `frame` (topfu.cpp:166-197)."""
    fx, fy, cx, cy = [np.float32(v) for v in synth.intrinsics(W, H)]
    d0 = oracle_mod.truncate(oracle_mod.bilateral(frame), 2.0)
    dl = [d0, oracle_mod.pyr_down(d0)]
    dl.append(oracle_mod.pyr_down(dl[1]))
    return [oracle_mod.points_normals(dl[l], fx / np.float32(1 << l), fy / np.float32(1 << l), cx / np.float32(1 << l),
                                      cy / np.float32(1 << l)) for l in range(3)]


_frames_expected = {}


def _frames_expect(oracle_mod, algebra, W, H, N):
    """The oracle over N frames: per frame its bool, iteration count and pose, and the affine and
    sums of estimateTransform run by the oracle's reduction and step on the frame's own maps."""
    key = (algebra, W, H, N)
    if key in _frames_expected:
        return _frames_expected[key]
    oracle_mod.set_pose_algebra(algebra, libm=False)
    fx, fy, cx, cy = synth.intrinsics(W, H)
    p = oracle_mod.default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy)
    o = oracle_mod.Oracle(p)
    frames = synth.orbit_sequence(N, W, H, seed=7)
    out = []
    for k in range(N):
        rec = None
        if k > 0:
            prev = [o.prev_maps(l) for l in range(3)]
            curr = _frame_maps(o, oracle_mod, frames[k], W, H)
            intr = lambda l: tuple(np.float32(v) / np.float32(1 << l) for v in (fx, fy, cx, cy))
            rec = C.oracle_estimate(oracle_mod, curr, prev, iters=tuple(p.icp_iter_num), dist=p.icp_dist_thres,
                                    angle=np.float32(p.icp_angle_thres), intr=intr)
        ok = o(frames[k])
        out.append((ok, o.counters()["icp_iterations"], o.pose().copy(), rec))
    _frames_expected[key] = (frames, out)
    return _frames_expected[key]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("algebra", ALGEBRAS)
@pytest.mark.parametrize("W,H", [(352, 200), (80, 60)])
def test_slot_ownership_between_levels(cv_oracle, monkeypatch, W, H, algebra, schedule):
    N = 5
    frames, exp = _frames_expect(cv_oracle, algebra, W, H, N)
    assert [e[0] for e in exp] == [True] * N, "the oracle must track four frames"
    g = _ctx(algebra, schedule, monkeypatch, W, H)
    dev = DeviceFrames(frames)
    for k in range(N):
        ok, iters, pose, rec = exp[k]
        tag = f"{W}x{H} {algebra} {schedule} frame {k}"
        assert g(dev.ptr + k * W * H * 2) == ok, tag
        assert g.stats()["icp_iterations"] == iters, tag
        assert_bit_exact(tag + " pose", g.getCameraPose()[:3, :4], pose)
        if rec is not None:
            rok, rn, raff, rsums = rec
            assert (rok, rn) == (ok, iters), tag            # the restated loop is the frame's own
            aff, sums, gok, gn = _icp_result(g)
            assert (gok, gn) == (int(rok), rn), tag
            assert_bit_exact(tag + " affine", aff, raff)
            assert_bit_exact(tag + " sums", sums, rsums)
    g.close()
    dev.free()


@pytest.mark.parametrize("algebra", ALGEBRAS)
def test_lost_peer_at_the_last_iteration_of_a_level(cv_oracle, monkeypatch, algebra):
    """TFUSION_ICP_FAULT=1:2: the context's first persistent launch reports a lost peer at iteration
    2, the last of level 2 (no det check is taken from that iteration's window).  The call returns
    TF_HIP_ERROR, the state records ok = -1 and three iterations run; the next call is whole."""
    from topfusion_amd import _lib
    exp = _expect(cv_oracle, algebra)
    seed = 10
    ook, on, oaff, osums = exp[seed]
    assert ook and on == sum(C.ITERS)
    g = _ctx(algebra, "persistent", monkeypatch, C.W, C.H, [float(v) for v in C.intrinsics(0)], TFUSION_ICP_FAULT="1:2")
    _set_params(g)
    pyr = _Pyramids(*_case(seed))
    st, _, _, _ = _estimate(g, pyr)
    assert st == _lib.TF_HIP_ERROR
    _, _, rok, rn = _icp_result(g)
    assert (rok, rn) == (-1, 3)
    st, aff, ok, n = _estimate(g, pyr)
    assert st == _lib.TF_OK and (bool(ok), n) == (ook, on)
    assert_bit_exact("affine after the lost peer", aff, oaff)
    assert_bit_exact("sums after the lost peer", _icp_result(g)[1], osums)
    pyr.free()
    g.close()


def test_halted_context_skips_frames(cv_oracle, monkeypatch):
    """TFUSION_FILL_FAULT=3: frame 2 fails past its ICP and halts the batch; the persistent ICP
    launches of frames 3.. take the skipped-frame exit.  The batch reports TF_HIP_ERROR, and after
    tf_reset the same frames track bit-exactly."""
    from topfusion_amd import _lib as L
    W, H, N = 80, 60, 5
    monkeypatch.setenv("TFUSION_ED_LDS_MAX_N", "0")
    frames, exp = _frames_expect(cv_oracle, "opencv4", W, H, N)
    g = _ctx("opencv4", "persistent", monkeypatch, W, H, TFUSION_FILL_FAULT="3")
    dev = DeviceFrames(frames)
    with pytest.raises(L.TfError) as ei:
        g.process_frames(dev.ptr, N)
    assert ei.value.status == L.TF_HIP_ERROR
    g.reset()
    okg = g.process_frames(dev.ptr, N)
    assert list(okg) == [e[0] for e in exp]
    assert_bit_exact("pose after the reset", g.getCameraPose()[:3, :4], exp[-1][2])
    rok, rn, raff, rsums = exp[-1][3]
    aff, sums, gok, gn = _icp_result(g)
    assert (gok, gn) == (int(rok), rn)
    assert_bit_exact("affine after the reset", aff, raff)
    assert_bit_exact("sums after the reset", sums, rsums)
    g.close()
    dev.free()
