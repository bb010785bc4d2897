"""The input conditions of the free-view GPU tests (test_gpu_view.py), on the CPU: the standard scene and the
cases A-F of view_ref.py are what those tests need them to be, so that a GPU pass means something.  Measured on
the oracle (the figures each assertion prints): 1689 live entries, 1433 of them in the excess list, 1522 in the
tracker's list; case A 1417 visible."""
import numpy as np

import view_ref as V
from parity_util import assert_bit_exact
from topfusion_amd import synth


def _hits(ref):
    return int((ref["raycast"][..., 3] > 0).sum())


def test_standard_scene_fills_the_excess_list():
    s = V.standard_scene()
    h, nb = s["hash"], V.TABLES["n_buckets"]
    live = np.flatnonzero(h["ptr"] >= 0)
    n_total = len(h)
    print("live", len(live), "in excess", int((live >= nb).sum()), "tracker list", len(s["visible_ids"]), "n_total", n_total)
    assert n_total == 4256 and n_total % 16 == 0 and n_total % 64 != 0 and n_total % 256 != 0
    assert len(live) >= 1500 and int((live >= nb).sum()) >= 1000
    assert len(s["visible_ids"]) >= 1000


def test_case_a_differs_from_the_trackers_list_both_ways():
    s, ref = V.standard_scene(), V.case_reference("A")
    ids, tracker = ref["ids"], s["visible_ids"]
    n_total, nb = len(s["hash"]), V.TABLES["n_buckets"]
    extra, absent = np.setdiff1d(ids, tracker), np.setdiff1d(tracker, ids)
    print("A visible", len(ids), "not in tracker's", len(extra), "tracker's absent", len(absent), "excess", int((ids >= nb).sum()))
    assert np.all(np.diff(ids) > 0)
    assert len(extra) >= 100 and len(absent) >= 100
    assert int((ids >= nb).sum()) >= 1000
    assert ids.max() >= n_total // 64 * 64 and ids.max() >= n_total // 256 * 256     # the last partial wave / workgroup
    assert _hits(ref) > 0


def test_cases_b_c_sizes_and_hits():
    for name in ("B", "C"):
        cols, rows, _, _ = V.CASES[name]
        ref = V.case_reference(name)
        print(name, "visible", len(ref["ids"]), "hits", _hits(ref), "tiles", ref["stats"]["noTotalBlocks"])
        assert _hits(ref) > 0 and len(ref["ids"]) > 0
    cols, rows = V.CASES["B"][:2]
    assert cols < V.W0 and rows < V.H0 and cols % 8 and rows % 8 and cols % 16 and rows % 16
    cols, rows = V.CASES["C"][:2]
    assert cols > V.W0 and rows > V.H0


def test_case_d_cap_binds_and_changes_the_image():
    c, d = V.case_reference("C"), V.case_reference("D")
    print("C tiles", c["stats"]["noTotalBlocks"], "D tiles", d["stats"]["noTotalBlocks"], "D hits", _hits(d))
    assert c["stats"]["noTotalBlocks"] > 400 and d["stats"]["noTotalBlocks"] == 400
    assert np.array_equal(c["ids"], d["ids"])
    assert _hits(d) > 0 and not np.array_equal(c["images"][0], d["images"][0])


def test_case_e_sees_nothing():
    e = V.case_reference("E")
    assert len(e["ids"]) == 0 and e["stats"]["noVisibleEntries"] == 0
    assert np.all(e["range"][..., 0] == V.FAR_AWAY) and np.all(e["range"][..., 1] == V.VERY_CLOSE)
    for img in e["images"].values():
        assert not img.any()


def test_case_f_smallest_view_hits():
    f = V.case_reference("F")
    print("F visible", len(f["ids"]), "hits", _hits(f))
    assert V.CASES["F"][:2] == (4, 4) and _hits(f) > 0


def test_world_to_camera_is_the_rigid_inverse(oracle_mod):
    for k in (0, -80, 120):
        R, t = synth.orbit_pose(k)
        assert_bit_exact(f"w2c {k}", synth.world_to_camera_rt(R, t), oracle_mod.rigid_inv(V.rt32(R, t)))
    R, t = synth._rot_y(np.pi), np.zeros(3)
    assert_bit_exact("w2c look back", synth.world_to_camera_rt(R, t), oracle_mod.rigid_inv(V.rt32(R, t)))
