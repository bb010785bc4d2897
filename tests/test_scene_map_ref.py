"""The map checkpoint file (version 2: a swapping context's, both tiers) restated in numpy (tests/scene_map_ref.py),
and the library's host parser (topfusion_amd/csrc/tf_scene_file.cpp) over it under AddressSanitizer / UBSan from
a stand-alone program.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import scene_ckpt_ref as R
import scene_map_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tiny_state_has_every_kind_of_record():
    s = MR.tiny_state()
    h, st, fl = s["hash"], s["swapState"], s["swapFlags"]
    reset = np.array([e.tobytes() == R.reset_entry().tobytes() for e in h])
    assert ((h["ptr"] == -1) & (fl == 1)).any()                          # stored only
    assert ((h["ptr"] >= 0) & (fl == 1) & (st == 1)).any()               # pending
    assert ((h["ptr"] >= 0) & (fl == 1) & (st == 2)).any()               # merged
    assert (reset & (fl == 1)).any()                                     # no hash entry left, a stored block
    assert (reset & (fl == 0) & (st != 0) & (s["visType"] == 0)).any()   # only a swap state
    assert (reset & (fl == 0) & (st == 0) & (s["visType"] != 0)).any()   # only visType


def test_roundtrip():
    s = MR.tiny_state()
    data = MR.pack(s)
    assert MR.states_equal(MR.unpack(data), s)                           # a zeroed store but for the flagged blocks
    assert MR.states_equal(MR.unpack(data, store=s["store"]), s)
    assert MR.unpack(data, store=s["store"])["store"].tobytes() == s["store"].tobytes()
    assert MR.pack(MR.unpack(data)) == data
    # unflagged stored blocks are not state: another store there is the same file and an equal state
    t = dict(s, store=s["store"].copy())
    t["store"].reshape(-1, 512)[s["swapFlags"] == 0] ^= 0x5a5a
    assert MR.pack(t) == data and MR.states_equal(t, s)
    t["store"].reshape(-1, 512)[9, 17] ^= 1                              # a flagged one is
    assert MR.pack(t) != data and not MR.states_equal(t, s)
    for k in ("swapState", "swapFlags"):
        t = dict(s, **{k: s[k].copy()})
        t[k][20] = 1
        assert not MR.states_equal(t, s), k


def test_size_formula():
    """304 + 24 R + 2048 (b + s) + 4 (V + A + E) + M: a function of the counts alone, never of a capacity."""
    s = MR.tiny_state()
    data = MR.pack(s)
    rec = MR.records_of(s)
    b, c = int((rec["entry"]["ptr"] >= 0).sum()), int((rec["hasStoredData"] == 1).sum())
    assert (len(rec), b, c) == (7, 3, 4)
    maps = 2 * 16 * (16 * 12 + 8 * 6 + 4 * 3)
    assert len(data) == 304 + 24 * 7 + 2048 * (3 + 4) + 4 * (2 + 1 + 5) + maps == MR.file_size(s["params"], s["counters"], 7, 3, 4)
    assert struct.unpack_from("<q", data, 232)[0] == len(data) and struct.unpack_from("<q", data, 288)[0] == 4
    assert struct.unpack_from("<I", data, 8)[0] == 2
    big = MR.tiny_state(n_buckets=1 << 14, n_excess=1 << 10, n_blocks=2048)
    big["counters"]["lastFreeBlockId"] = 0
    assert len(MR.pack(big)) == len(data)


def test_records_and_payload_order():
    s = MR.tiny_state()
    data = MR.pack(s)
    rec = np.frombuffer(data, MR.RECORD_DTYPE, 7, MR.HEADER_BYTES)
    assert list(rec["index"]) == [3, 7, 9, 11, 13, 14, 18]
    want = {3: (1, 1, 1), 7: (2, 0, 0), 9: (0, 0, 1), 11: (0, 2, 1), 13: (0, 0, 1), 14: (0, 1, 0), 18: (0, 2, 0)}
    got = {int(r["index"]): (int(r["visType"]), int(r["swapState"]), int(r["hasStoredData"])) for r in rec}
    for i, v in want.items():
        assert got[i] == v, i
    assert not rec["pad"].any()
    assert rec[rec["index"] == 13]["entry"].tobytes() == R.reset_entry().tobytes()
    # active blocks in record order (entries 3, 11, 18 hold blocks 1, 3, 0), then stored ones (entries 3, 9, 11, 13)
    o = MR.HEADER_BYTES + 24 * 7
    vba, store = s["vba"].reshape(-1, 512), s["store"].reshape(-1, 512)
    for blk in (1, 3, 0):
        assert data[o:o + 2048] == vba[blk].tobytes()
        o += 2048
    for e in (3, 9, 11, 13):
        assert data[o:o + 2048] == store[e].tobytes()
        o += 2048


def test_version_1_passthrough():
    for rgb in (0, 1):
        s = R.tiny_state(voxel_rgb=rgb)
        data = R.pack(s)
        assert MR.pack(s) == data
        assert MR.records_of(s).tobytes() == R.records_of(s).tobytes()
        assert MR.states_equal(MR.unpack(data), s) and R.states_equal(MR.unpack(data), s)
        rec = R.records_of(s)
        n = int((rec["entry"]["ptr"] >= 0).sum())
        assert MR.file_size(s["params"], s["counters"], len(rec), n) == len(data)


def test_map_parser_under_asan_ubsan(tmp_path):
    """tf_scene_file.cpp built for the CPU with -fsanitize=address,undefined and driven by
    tests/scene_map_parser_main.cpp in one process: the intact version-2 file of the tiny swapping state is
    accepted with pack()'s info fields; every truncated length, every header word and the first records' index,
    ptr, swap state, stored flag and pad byte overwritten by 0, -1, the maximum and an off-by-one are rejected
    (by version 1's reader too), with no sanitizer report."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "scene_map_parser_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe,
                        os.path.join(ROOT, "tests", "scene_map_parser_main.cpp"),
                        os.path.join(ROOT, "topfusion_amd", "csrc", "tf_scene_file.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    s = MR.tiny_state()
    data = MR.pack(s)
    path = tmp_path / "tiny.tfmap"
    path.write_bytes(data)
    c = s["counters"]
    args = [7, 3, 4, c["frame_counter"], c["lastFreeBlockId"], c["lastFreeExcessListId"], c["noVisibleEntries"],
            s["pose_algebra"], 4, 16, 12]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > len(data)              # the truncations alone are that many
