"""The map merge restated serially (tests/scene_merge_ref.py): the closed form a parallel implementation computes equals
the one-at-a-time loop, the made pair hits every case, a merge into a reset state gives the file's map by block
position, the reference's chain walk finds every carried position exactly once afterwards, and the refusals raise and
leave their inputs untouched.  The host pass of the library over a record table runs under ASan + UBSan from a
stand-alone program.  No GPU."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest

import alloc_cases as A
import scene_ckpt_ref as R
import scene_merge_ref as G
import scene_resize_ref as Z
import vbh_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = ((0, 0, 0), G.MADE_OFFSET)


def _snapshot(s):
    return copy.deepcopy({k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in s.items() if k != "maps"})


def _reset_state(like, tables):
    """ResetScene's state in `tables`, with `like`'s parameters otherwise."""
    nb, ne, nblk = tables["n_buckets"], tables["n_excess"], tables["n_blocks"]
    p = like["params"].copy()
    p["n_buckets"], p["n_excess"], p["n_blocks"] = nb, ne, nblk
    return dict(params=p, pose_algebra=4, pose=np.asarray(like["pose"], np.float32).copy(),
                hash=np.full(nb + ne, R.reset_entry(), R.HASH_DTYPE), visType=np.zeros(nb + ne, np.uint8),
                vba=np.full(nblk * 512, R.VOXEL_RESET, np.uint32), rgb=None, visibleIds=np.zeros(0, np.int32),
                allocList=np.arange(nblk, dtype=np.int32), excessList=np.arange(ne, dtype=np.int32), maps=like["maps"],
                counters=dict(lastFreeBlockId=nblk - 1, lastFreeExcessListId=ne - 1, noVisibleEntries=0, frame_counter=0))


def test_made_pair_is_of_every_kind():
    """At least this many of each case, with either offset (the GPU test merges with both)."""
    target, file = G.made_pair()
    assert R.states_equal(R.unpack(R.pack(file)), file)                          # a valid version-1 file
    for key in ("n_buckets", "n_excess", "n_blocks", "cols", "rows"):
        assert int(target["params"][key]) != int(file["params"][key]), key
    h, nb = target["hash"], G.MADE["n_buckets"]
    v, e = target["counters"]["lastFreeBlockId"], target["counters"]["lastFreeExcessListId"]
    assert 0 < v < G.MADE["n_blocks"] - 1 and 0 < e < G.MADE["n_excess"] - 1     # partly consumed ...
    assert (np.diff(target["allocList"][:v + 1]) != 1).sum() > v // 2            # ... and shuffled
    assert (np.diff(target["excessList"][:e + 1]) != 1).sum() > e // 2
    lengths = {}
    for b in range(nb):
        if h["ptr"][b] >= -1:
            n, i = 1, b
            while h["offset"][i] >= 1:
                i, n = nb + int(h["offset"][i]) - 1, n + 1
            lengths[n] = lengths.get(n, 0) + 1
    assert all(lengths.get(n, 0) >= 2 for n in (1, 2, 3)) and sum(c for n, c in lengths.items() if n >= 4) >= 2, lengths
    assert (h["ptr"] == -1).sum() >= 30
    for off in OFFSETS:
        k = G.kinds(target, file, off)
        assert k["orphaned_buckets"] == 3 and k["new_into_orphaned_bucket"] >= 1, k
        assert k["combined"] >= 60 and k["revived"] >= 10, k
        assert k["new_free_bucket"] >= 20 and k["new_chain_end"] >= 40, k
        assert k["buckets_several_new_free"] >= 2 and k["buckets_several_new_chain"] >= 5 and k["longest_new_run"] >= 5, k
        assert k["skipped"] >= 30, k
        assert k["w_zero"] >= 5000 and k["w_max"] >= 5000 and k["w_past_max"] >= 5000, k
        assert k["off_grid_new"] >= 10 and k["off_grid"] >= k["off_grid_new"], k


@pytest.mark.parametrize("off", OFFSETS)
def test_closed_form_is_the_serial_loop(off):
    target, file = G.made_pair()
    out, report = G.merge(target, file, off)
    rows = G.closed_form(target, file, off)
    nb = G.MADE["n_buckets"]
    rec = R.records_of(file)
    assert len(rows) == report["records_combined"] + report["records_inserted"] + report["records_revived"]
    assert report["records_skipped"] == len(rec) - len(rows) == int((rec["entry"]["ptr"] < 0).sum())
    assert report["blocks_used"] == sum(r[1] != G.COMBINE for r in rows) == report["records_inserted"] + report["records_revived"]
    assert report["excess_used"] == sum(r[1] == G.INSERT and r[4] >= nb for r in rows)
    src = np.asarray(file["vba"]).view(np.uint32).reshape(-1, 512)
    vba = out["vba"].reshape(-1, 512)
    linked = {}
    for k, mode, hb, m, t, ptr, link in rows:
        e, f = out["hash"][t], rec[k]["entry"]
        pos = tuple(int(f[a]) + o for a, o in zip("xyz", off))
        assert (int(e["x"]), int(e["y"]), int(e["z"])) == pos and int(e["ptr"]) == ptr, (k, mode)
        if mode != G.COMBINE:
            assert vba[ptr].tobytes() == src[int(f["ptr"])].tobytes(), (k, mode)
        if mode == G.INSERT:
            assert int(e["pad"]) == 0 and out["visType"][t] == 0
            if link >= 0:
                linked[link] = t
                assert int(out["hash"][link]["offset"]) == t - nb + 1, k
    # every entry the merge did not name is the target's, but for the links
    named = {r[4] for r in rows if r[1] != G.COMBINE}
    for i in range(len(target["hash"])):
        if i in named:
            continue
        a, b = target["hash"][i].copy(), out["hash"][i]
        if i in linked:
            a["offset"] = linked[i] - nb + 1
        assert a.tobytes() == b.tobytes(), i
    assert len({r[4] for r in rows}) == len(rows)
    ptrs = [r[5] for r in rows if r[1] != G.COMBINE]
    v = target["counters"]["lastFreeBlockId"]
    assert ptrs == target["allocList"][v + 1 - len(ptrs):v + 1][::-1].tolist()


@pytest.mark.parametrize("off", OFFSETS)
def test_every_carried_position_is_found_once(off):
    target, file = G.made_pair()
    out, report = G.merge(target, file, off)
    nb = G.MADE["n_buckets"]
    _, pos, fptr, _ = G.carried(file, off)
    at = set()
    for p in pos:
        found = V.find_held(out["hash"], nb, p, from_free_bucket=False)[0]
        assert len(found) == 1 and int(out["hash"]["ptr"][found[0]]) >= 0, p
        assert A.lookup(out["hash"], nb, p)[:2] == (found[0], 0)
        at.add(found[0])
    assert len(at) == len(pos)
    # what the target could find it still finds, with the same block
    for i in np.flatnonzero(target["hash"]["ptr"] >= 0):
        e = target["hash"][i]
        if V.find_held(target["hash"], nb, (e["x"], e["y"], e["z"]), from_free_bucket=False)[0] == [i]:
            assert V.find_held(out["hash"], nb, (e["x"], e["y"], e["z"]), from_free_bucket=False)[0] == [i] and int(out["hash"]["ptr"][i]) == int(e["ptr"])
    # blocks distinct; the lists, the visible list, the pose and the maps as they were
    used = out["hash"]["ptr"][out["hash"]["ptr"] >= 0]
    assert len(np.unique(used)) == len(used)
    for k in ("allocList", "excessList", "visibleIds", "pose"):
        assert np.asarray(out[k]).tobytes() == np.asarray(target[k]).tobytes(), k
    c, c0 = out["counters"], target["counters"]
    assert c == dict(c0, lastFreeBlockId=c0["lastFreeBlockId"] - report["blocks_used"],
                     lastFreeExcessListId=c0["lastFreeExcessListId"] - report["excess_used"])


@pytest.mark.parametrize("off", OFFSETS)
def test_into_a_reset_state_gives_the_files_map(off):
    target, file = G.made_pair()
    empty = _reset_state(target, G.MADE)
    out, report = G.merge(empty, file, off)
    _, pos, fptr, _ = G.carried(file, off)
    assert report["records_inserted"] == len(pos) and report["records_combined"] == report["records_revived"] == 0
    src = np.asarray(file["vba"]).view(np.uint32).reshape(-1, 512)
    live = np.flatnonzero(out["hash"]["ptr"] >= 0)
    got = {(int(e["x"]), int(e["y"]), int(e["z"])): out["vba"].reshape(-1, 512)[int(e["ptr"])].tobytes() for e in out["hash"][live]}
    want = {tuple(int(v) for v in p): src[f].tobytes() for p, f in zip(pos, fptr)}
    assert got == want
    # ... and is the resized load's placement: the same rule into a reset table
    if off == (0, 0, 0):
        only = dict(file, hash=file["hash"].copy(), visType=np.zeros_like(file["visType"]))
        only["hash"][only["hash"]["ptr"] == -1] = R.reset_entry()
        rz, _ = Z.resize(only, G.MADE["n_buckets"], G.MADE["n_excess"], G.MADE["n_blocks"], 64)
        assert rz["hash"].tobytes() == out["hash"].tobytes() and rz["vba"].tobytes() == out["vba"].tobytes()
    again, second = G.merge(out, file, off)                                      # a second time: every record combines
    assert second["records_combined"] == len(pos) and second["blocks_used"] == second["excess_used"] == 0
    assert again["hash"].tobytes() == out["hash"].tobytes()


def test_refusals_raise_and_leave_the_inputs_untouched():
    target, file = G.made_pair()
    before = _snapshot(target), _snapshot(file)
    need = G.needs(target, file)
    B, X = need["blocks_used"], need["excess_used"]
    assert B > 0 and X > 0
    exact, report = G.merge(G.with_free(target, B, X), file)
    assert report == need and exact["counters"]["lastFreeBlockId"] == exact["counters"]["lastFreeExcessListId"] == -1
    full, _ = G.merge(target, file)
    assert exact["hash"].tobytes() == full["hash"].tobytes() and exact["vba"].tobytes() == full["vba"].tobytes()
    for nb_free, ne_free in ((B - 1, X + 5), (B + 5, X - 1)):
        short = G.with_free(target, nb_free, ne_free)
        snap = _snapshot(short)
        with pytest.raises(G.Capacity) as e:
            G.merge(short, file)
        assert e.value.report == need and _snapshot(short) == snap

    def invalid(t, f, off=(0, 0, 0)):
        snap = _snapshot(t), _snapshot(f)
        with pytest.raises(G.Invalid):
            G.merge(t, f, off)
        assert (_snapshot(t), _snapshot(f)) == snap

    for key, value in (("voxelSize", 0.006), ("mu", 0.03), ("maxW", 50), ("use_swapping", 1), ("voxel_rgb", 1)):
        p = file["params"].copy()
        p[key] = value
        invalid(target, dict(file, params=p))
    p = target["params"].copy()
    p["use_swapping"] = 1
    invalid(dict(target, params=p), file)
    _, pos, _, _ = G.carried(file)
    invalid(target, file, (32767 - int(pos[:, 0].max()) + 1, 0, 0))
    invalid(target, file, (0, 0, -32768 - int(pos[:, 2].min()) - 1))
    G.needs(target, file, (32767 - int(pos[:, 0].max()), 0, -32768 - int(pos[:, 2].min())))     # the last offsets that fit
    dup = dict(file, hash=file["hash"].copy())
    k = np.flatnonzero(dup["hash"]["ptr"] >= 0)
    for f in "xyz":
        dup["hash"][f][k[-1]] = dup["hash"][f][k[0]]
    invalid(target, dup)
    assert (_snapshot(target), _snapshot(file)) == before


def test_records_pass_under_asan_ubsan(tmp_path):
    """tests/scene_merge_records_main.cpp with topfusion_amd/csrc/tf_scene_file.cpp, built for the CPU with
    -fsanitize=address,undefined: tf_merge_records_check over the made file's record table in a buffer of exactly its
    length -- the offsets at and one past the int16 edges, duplicated positions, an empty table."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "scene_merge_records_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe,
                        os.path.join(ROOT, "tests", "scene_merge_records_main.cpp"),
                        os.path.join(ROOT, "topfusion_amd", "csrc", "tf_scene_file.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, file = G.made_pair()
    path = tmp_path / "made.tfscene"
    path.write_bytes(R.pack(file))
    n_carried = len(G.carried(file)[0])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path), str(n_carried)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 31 checks") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_wrapper_signatures():
    """tf_map_merge through every layer that needs no GPU: the ctypes signature and report, TopFu.merge_map, the C++
    wrappers."""
    import ctypes
    from topfusion_amd import TopFu, _lib as L
    lib = L.load()
    assert lib.tf_map_merge.argtypes[3]._type_ is L.TfMergeReport and ctypes.sizeof(L.TfMergeReport) == 48
    assert tuple(L.TfMergeReport().as_dict()) == G.REPORT_KEYS
    assert lib.tf_map_merge(None, b"x", None, None) == L.TF_INVALID_ARG
    assert callable(TopFu.merge_map)
    for header, cls in (("topfu.hpp", "TopFu"), ("engines.hpp", "Scene")):
        src = open(os.path.join(ROOT, "include", "tfusion", header)).read()
        assert "mergeMap(" in src and "tf_map_merge(" in src, (header, cls)
