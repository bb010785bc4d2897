"""The scene checkpoint file restated in numpy (tests/scene_ckpt_ref.py), and the library's host parser
(topfusion_amd/csrc/tf_scene_file.cpp) under AddressSanitizer / UBSan from a stand-alone program.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import scene_ckpt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rgb", [0, 1])
def test_roundtrip(rgb):
    s = R.tiny_state(voxel_rgb=rgb)
    data = R.pack(s)
    assert R.states_equal(R.unpack(data), s)
    assert R.pack(R.unpack(data)) == data


def test_roundtrip_larger_tables():
    s = R.tiny_state(cols=96, rows=72, n_buckets=4096, n_excess=512, n_blocks=128, voxel_rgb=1, seed=11)
    s["hash"][4095] = (1, 1, 1, 0, 0, 5)
    s["hash"][4096 + 511] = (2, 2, 2, 0, 0, 7)
    unused = np.setdiff1d(np.arange(128), s["hash"]["ptr"][s["hash"]["ptr"] >= 0])
    s["vba"].reshape(-1, 512)[unused] = R.VOXEL_RESET           # what no entry holds is not part of the state
    s["rgb"].reshape(-1, 512)[unused] = 0
    data = R.pack(s)
    assert R.states_equal(R.unpack(data), s)


@pytest.mark.parametrize("rgb", [0, 1])
def test_size_formula(rgb):
    """296 + 24 records + (2048 | 4096) blocks + 4 (visible + live alloc + live excess) + the maps: a function
    of the counts alone, never of a capacity."""
    s = R.tiny_state(voxel_rgb=rgb)
    data = R.pack(s)
    rec = R.records_of(s)
    n_stored = int((rec["entry"]["ptr"] >= 0).sum())
    assert (len(rec), n_stored) == (4, 2)
    maps = 2 * 16 * (16 * 12 + 8 * 6 + 4 * 3)
    assert len(data) == 296 + 24 * 4 + (4096 if rgb else 2048) * 2 + 4 * (2 + 0 + 5) + maps
    assert struct.unpack_from("<q", data, 232)[0] == len(data)
    # the same scene in tables a thousand times the size: the same length
    big = R.tiny_state(voxel_rgb=rgb, n_buckets=1 << 14, n_excess=1 << 10, n_blocks=2048)
    big["counters"]["lastFreeBlockId"] = -1
    assert len(R.pack(big)) == len(data)


def test_records_ascend_and_visible_only_entry():
    s = R.tiny_state()
    data = R.pack(s)
    rec = np.frombuffer(data, R.RECORD_DTYPE, 4, R.HEADER_BYTES)
    assert list(rec["index"]) == [3, 7, 9, 18]
    assert np.all(np.diff(rec["index"].astype(np.int64)) > 0)
    # entry 7 has only visType set: a record with ResetScene's entry, and no payload for it
    assert rec[1]["visType"] == 2 and rec[1]["entry"].tobytes() == R.reset_entry().tobytes()
    assert not (rec["swapState"].any() or rec["hasStoredData"].any() or rec["pad"].any())    # version 1: three pad bytes
    # payloads in record order: entry 3 holds block 1, entry 18 block 0
    o = R.HEADER_BYTES + 24 * 4
    vba = s["vba"].reshape(-1, 512)
    assert data[o:o + 2048] == vba[1].tobytes() and data[o + 2048:o + 4096] == vba[0].tobytes()


def test_parser_under_asan_ubsan(tmp_path):
    """tf_scene_file.cpp built for the CPU with -fsanitize=address,undefined and driven by
    tests/scene_ckpt_parser_main.cpp in one process: the intact file of a tiny scene (16 x 12, 2 blocks) is
    accepted with pack()'s info fields; every truncated length, every header word and the first records'
    index / ptr overwritten by 0, -1, INT_MAX and an off-by-one are rejected, with no sanitizer report."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "scene_ckpt_parser_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe,
                        os.path.join(ROOT, "tests", "scene_ckpt_parser_main.cpp"),
                        os.path.join(ROOT, "topfusion_amd", "csrc", "tf_scene_file.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    s = R.tiny_state()
    path = tmp_path / "tiny.tfscene"
    path.write_bytes(R.pack(s))
    c = s["counters"]
    args = [4, 2, c["frame_counter"], c["lastFreeBlockId"], c["lastFreeExcessListId"], c["noVisibleEntries"],
            s["pose_algebra"], 2, 16, 12]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > len(R.pack(s))        # the truncations alone are that many
