"""The input conditions of the whole-reading view tests (tests/view_whole_ref.py), on the CPU oracle: the tiered
standard scene puts every row of the resolution table under the cases' rays, and the composed reference is the
resident one where nothing is stored.  tests/test_gpu_view_whole.py compares the GPU against these references."""
import numpy as np
import pytest

import mesh_whole_ref as WR
import view_ref as V
import view_whole_ref as VW

ACTIVE, STORED, PENDING, STALE, LOST = range(5)


def _hits(ref):
    return int((ref["raycast"][..., 3] > 0).sum())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_case_a_hits_every_class():
    whole, resident = VW.case_reference("A"), VW.case_resident("A")
    cls, _ = VW.hit_classes("A", whole)
    counts = {k: int((cls == k).sum()) for k in (ACTIVE, STORED, PENDING, STALE)}
    print("case A: visible", len(whole["ids"]), "vs", len(resident["ids"]), "hits", _hits(whole), "vs", _hits(resident), "by class", counts)
    assert min(counts.values()) >= 500, counts
    assert len(whole["ids"]) > len(resident["ids"]) and _hits(whole) > _hits(resident)
    for t in VW.TYPES:
        assert not np.array_equal(whole["images"][t], resident["images"][t]), f"image type {t} is the resident reading's"


def test_case_f_hits_both_tiers():
    cls, _ = VW.hit_classes("F", VW.case_reference("F"))
    assert (cls == STORED).sum() >= 1 and (cls == PENDING).sum() >= 1, cls


def test_case_d_cap_binds_under_both_readings():
    cap = VW.CASES["D"][3]["max_render_blocks"]
    for ref, free in ((VW.case_reference("D"), VW.case_reference("C")), (VW.case_resident("D"), VW.case_resident("C"))):
        assert free["stats"]["noTotalBlocks"] > cap, free["stats"]
        assert not np.array_equal(ref["range"], free["range"]), "the cap dropped no tile"


def test_case_e_sees_nothing():
    ref = VW.case_reference("E")
    assert len(ref["ids"]) == 0 and _hits(ref) == 0 and not any(ref["images"][t].any() for t in VW.TYPES)


def test_case_g_straddles_the_grid():
    whole = VW.case_reference("G")
    cls, bx = VW.hit_classes("G", whole)
    outside = int((bx >= 128).sum())
    print("case G: visible", len(whole["ids"]), "hits", _hits(whole), "outside the grid", outside)
    assert outside >= 1000 and int((bx < 128).sum()) >= 1000
    assert min(int(((cls == k) & (bx >= 128)).sum()) for k in (STORED, PENDING)) > 0


@pytest.mark.parametrize("name", sorted(V.CASES))
def test_no_stored_data_is_the_resident_reference(oracle_mod, name):
    s = V.standard_scene()
    n = len(s["hash"])
    cols, rows, c2w, vp = V.CASES[name]
    store = np.zeros(n * 512, s["vba"].dtype)
    got = VW.whole_stages(oracle_mod, (s["hash"], s["vba"], np.zeros(n, np.uint8), np.zeros(n, np.uint8), store), cols, rows, c2w, vp)
    want = V.case_reference(name)
    for k in ("ids", "range", "raycast", "points", "normals"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (name, k)
    for t in VW.TYPES:
        assert np.array_equal(got["images"][t], want["images"][t]), (name, t)
    assert got["stats"] == want["stats"]


def test_resolution_rows_of_the_scene():
    t = VW.tiered_scene()
    row = WR.classify(t["hash"], t["state"], t["flags"])
    cls = t["cls"]
    assert (row[cls == ACTIVE] == 0).all() and (row[cls == STALE] == 0).all() and (row[cls == PENDING] == 1).all()
    assert (row[cls == STORED] == 2).all() and (row[(cls == LOST) | (cls < 0)] == -1).all()
    assert min(int((cls == k).sum()) for k in range(5)) > 50


def test_reading_calls_are_declared_and_bound():
    """The two calls of the reading are in include/tfusion_hip.h with ctypes signatures, and the enum values agree."""
    from topfusion_amd import _lib
    names = _lib.header_functions()
    assert "tf_set_view_reading" in names and "tf_get_view_reading" in names
    src = open(_lib.HEADER_PATH).read()
    for k, name in enumerate(("TF_VIEW_RESIDENT", "TF_VIEW_WHOLE")):
        assert f"{name} = {k}" in src and getattr(_lib, name) == k
    L = _lib.load()
    assert L.tf_set_view_reading.argtypes is not None and L.tf_get_view_reading.argtypes is not None
