"""The resized load restated serially (tests/scene_resize_ref.py): the closed form a parallel implementation computes
equals the one-at-a-time insertion, and the result is a table in which the reference's chain walk finds exactly the
carried records.  No GPU."""
import numpy as np
import pytest

import scene_ckpt_ref as R
import scene_map_ref as MR
import scene_resize_ref as Z


def _cases():
    return {"tiny v1": R.tiny_state(), "tiny v1 colour": R.tiny_state(voxel_rgb=1), "tiny v2": MR.tiny_state(),
            "made v2": Z.made_state(True), "made v1 colour": Z.made_state(False)}


_made = {}


def _case(name):
    if name not in _made:
        _made.update(_cases())
    return _made[name]


NAMES = ("tiny v1", "tiny v1 colour", "tiny v2", "made v2", "made v1 colour")


def _targets(s, name):
    nb = int(s["params"]["n_buckets"])
    need = {b: Z.needs(s, b) for b in (max(nb // 4, 1), nb, nb * 4)}
    out = []
    for b, n in need.items():
        out.append((b, max(n["excess_used"], 1), max(n["blocks"], 1)))                        # exactly what is needed
        out.append((b, n["excess_used"] + 37, 2 * int(s["params"]["n_blocks"])))
    return out


def test_made_state_is_of_every_kind():
    s = Z.made_state(True)
    rec = MR.records_of(s)
    ptr = rec["entry"]["ptr"]
    assert len(rec) > 2 * 256 and len(rec) % 256                                             # several record groups, a ragged last one
    assert (ptr < -1).sum() >= 8 and ((ptr < -1) & (rec["hasStoredData"] == 1)).any()        # dropped, some with a stored block
    assert ((ptr == -1) & (rec["hasStoredData"] == 1)).any() and ((ptr == -1) & (rec["hasStoredData"] == 0)).any()
    assert ((ptr >= 0) & (rec["swapState"] == 1)).any() and ((ptr >= 0) & (rec["swapState"] == 2)).any()
    n_total = len(s["hash"])
    assert set((0, 255, 256, n_total - 1)) <= set(int(i) for i in rec["index"])               # the corners of the count groups
    assert (s["hash"]["offset"] > 0).sum() > 100                                              # chains
    for b in Z.MADE_TARGET_BUCKETS:
        n = Z.needs(s, b)
        assert n["excess_used"] % 16 == 0 and n["excess_used"] > 0 and n["longest_chain"] > 2, (b, n)
    assert Z.needs(s, Z.MADE_SHORT_BUCKETS)["excess_used"] % 16 == 1
    assert MR.states_equal(MR.unpack(MR.pack(s), store=s["store"]), s)                     # a valid file
    v1 = Z.made_state(False)
    assert R.states_equal(R.unpack(R.pack(v1)), v1) and v1["rgb"] is not None


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_is_the_serial_loop(name):
    s = _case(name)
    rec = MR.records_of(s)
    for nb, ne, nblk in _targets(s, name):
        out, report = Z.resize(s, nb, ne, nblk, 64)
        rows = Z.closed_form(s, nb, ne, nblk)
        assert len(rows) == report["records_carried"] == int((rec["entry"]["ptr"] >= -1).sum())
        assert report["records_dropped"] == len(rec) - len(rows)
        for k, h, m, t, ptr, link in rows:
            e = out["hash"][t]
            src = rec[k]["entry"]
            assert (int(e["x"]), int(e["y"]), int(e["z"])) == (int(src["x"]), int(src["y"]), int(src["z"])), (nb, k)
            assert int(e["ptr"]) == ptr and int(e["pad"]) == 0
            assert (t == h) == (m == 0) and (t < nb) == (m == 0)
            assert int(e["offset"]) == (0 if link < 0 else link - nb + 1)
            assert out["visType"][t] == rec[k]["visType"]
        assert len({r[3] for r in rows}) == len(rows)                                         # distinct entries
        assert report["excess_used"] == sum(1 for r in rows if r[2] > 0)
        assert report["blocks"] == sum(1 for r in rows if r[4] >= 0)
        assert report["longest_chain"] == max(r[2] for r in rows) + 1


@pytest.mark.parametrize("name", NAMES)
def test_carried_records_are_found_and_nothing_else(name):
    s = _case(name)
    sw = MR.swapping(s)
    rec = MR.records_of(s)
    vba_src = np.asarray(s["vba"]).view(np.uint32).reshape(-1, 512)
    cap = 5
    for nb, ne, nblk in _targets(s, name):
        out, report = Z.resize(s, nb, ne, nblk, cap)
        h = out["hash"]
        vba = out["vba"].reshape(-1, 512)
        found_at, longest, cache = set(), 0, 0
        for r in rec:
            e = r["entry"]
            if int(e["ptr"]) < -1:
                continue
            found, walked = Z.find_entry(h, nb, (e["x"], e["y"], e["z"]))
            longest = max(longest, walked)
            assert len(found) == 1, (nb, int(r["index"]))
            t = found[0]
            found_at.add(t)
            assert (int(h[t]["ptr"]) >= 0) == (int(e["ptr"]) >= 0)                            # the ptr class
            if int(e["ptr"]) >= 0:
                assert vba[int(h[t]["ptr"])].tobytes() == vba_src[int(e["ptr"])].tobytes()
                if s["rgb"] is not None:
                    assert (out["rgb"].reshape(-1, 512)[int(h[t]["ptr"])].tobytes() ==
                            np.asarray(s["rgb"]).reshape(-1, 512)[int(e["ptr"])].tobytes())
            assert out["visType"][t] == r["visType"]
            if sw:
                assert out["swapState"][t] == r["swapState"] and out["swapFlags"][t] == r["hasStoredData"]
                if r["hasStoredData"]:
                    cache += 1
                    assert (out["store"].reshape(-1, 512)[t].tobytes() ==
                            np.asarray(s["store"]).view(np.uint32).reshape(-1, 512)[int(r["index"])].tobytes())
        # nothing else: every other entry is ResetScene's, with no visType, state or flag
        others = np.setdiff1d(np.arange(nb + ne), sorted(found_at))
        assert len(found_at) == report["records_carried"]
        assert all(e.tobytes() == R.reset_entry().tobytes() for e in h[others])
        assert not out["visType"][others].any()
        if sw:
            assert not out["swapState"][others].any() and not out["swapFlags"][others].any()
            assert report["cache_blocks"] == cache
        # blocks distinct, from the top of an identity list; the counters; the lists
        ptrs = h["ptr"][h["ptr"] >= 0]
        assert sorted(ptrs) == list(range(nblk - report["blocks"], nblk))
        assert out["allocList"].tobytes() == np.arange(nblk, dtype=np.int32).tobytes()
        assert out["excessList"].tobytes() == np.arange(ne, dtype=np.int32).tobytes()
        c = out["counters"]
        assert c["lastFreeBlockId"] == nblk - 1 - report["blocks"]
        assert c["lastFreeExcessListId"] == ne - 1 - report["excess_used"]
        assert c["frame_counter"] == s["counters"]["frame_counter"]
        free = np.setdiff1d(np.arange(nblk), ptrs)
        assert (vba[free] == R.VOXEL_RESET).all()
        assert report["longest_chain"] == longest
        visible = np.flatnonzero(out["visType"] > 0)
        assert c["noVisibleEntries"] == min(len(visible), cap)
        assert out["visibleIds"].tolist() == visible[:cap].tolist()
        assert out["pose"].tobytes() == np.asarray(s["pose"], np.float32).tobytes()
        assert all(a.tobytes() == np.asarray(b, np.float32).tobytes() for a, b in zip(out["maps"], s["maps"]))


@pytest.mark.parametrize("name", NAMES)
def test_capacity_is_raised_exactly_below_the_need(name):
    s = _case(name)
    nb = int(s["params"]["n_buckets"])
    for b in (max(nb // 4, 1), nb, nb * 4):
        n = Z.needs(s, b)
        B, X = n["blocks"], n["excess_used"]
        assert B > 0
        Z.resize(s, b, max(X, 1), B, 64)
        with pytest.raises(Z.Capacity) as e:
            Z.resize(s, b, X + 5, B - 1, 64)
        assert e.value.report == n
        if X > 0:
            with pytest.raises(Z.Capacity) as e:
                Z.resize(s, b, X - 1, B + 5, 64)
            assert e.value.report == n
