"""Checkpoints at the smallest tables (topfusion_amd/csrc/tf_scene_ckpt.hip): 256 buckets + 48 excess slots, so one full
256-entry count group and a ragged 48-entry one, and a prefix over two groups (one group per thread, most threads idle).
A hand-made state with records at both group edges, a wave edge and the last entry is saved, loaded and loaded
resized, without colour, with colour and on a swapping context, against the numpy restatements (scene_ckpt_ref /
scene_map_ref / scene_resize_ref) byte for byte; once more in a child process whose staging buffer holds one block, so
that every chunk boundary falls between two blocks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_ckpt_ref as R
import scene_map_ref as MR
import scene_resize_ref as Z
import test_gpu_scene_ckpt as C
import test_gpu_scene_map as T
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 16, 12                                          # scene_ckpt_ref.tiny_state's image: three pyramid levels down to 4 x 3
TABLES = dict(n_buckets=256, n_excess=48, n_blocks=64)
RESIZED = dict(n_buckets=64, n_excess=240, n_blocks=64)         # 304 entries again, longer chains
N_TOTAL = TABLES["n_buckets"] + TABLES["n_excess"]
VARIANTS = ("plain", "colour", "swapping")
# entry -> ptr: both edges of group 0 (0, 255), a wave edge (63 | 64), the ragged group's first and last entry (256, 303)
BLOCKS = {0: 5, 64: 0, 130: 9, 256: 63, 303: 17}
NO_BLOCK = (63, 200)                                    # ptr -1
ONLY_VIS = (192, 255)                                   # ResetScene's entry, visType 2
SAME_BUCKET = (0, 63, 130, 303)                         # positions that share a bucket at 64 buckets: a chain of four


def _ctx(variant, **kw):
    from topfusion_amd import TopFu, default_params
    fx, fy, cx, cy = synth.intrinsics(W, H)
    args = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=0.005, voxel_rgb=int(variant == "colour"), **TABLES)
    if variant == "swapping":
        args.update(use_swapping=1, swap_transfer_blocks=16)
    args.update(kw)
    return TopFu(default_params(**args))


def _made(variant):
    rng = np.random.default_rng(11)
    h = np.full(N_TOTAL, R.reset_entry(), R.HASH_DTYPE)
    for k, i in enumerate(sorted(list(BLOCKS) + list(NO_BLOCK))):
        x = k + 1
        if i in SAME_BUCKET:                            # the first x at which (x, 2k, -k) lands in bucket 7 of 64
            x = next(v for v in range(1, 4000) if Z.hash_index(v, 2 * k, -k, 64) == 7)
        h[i] = (x, 2 * k, -k, 0, 0, BLOCKS.get(i, -1))
    h["offset"][130] = 1                                # 130 -> excess slot 0 (entry 256) -> excess slot 47 (entry 303)
    h["offset"][256] = 48
    vis = np.zeros(N_TOTAL, np.uint8)
    vis[[0, 256]] = (1, 3)
    vis[list(ONLY_VIS)] = 2
    pose = np.eye(4, dtype=np.float32)[:3].reshape(12).copy()
    pose[[3, 7, 11]] = (0.125, -0.5, 0.75)
    s = dict(hash=h, visType=vis, vba=rng.integers(0, 1 << 24, TABLES["n_blocks"] * 512, dtype=np.uint32), rgb=None,
             visibleIds=np.array([0, 256], np.int32), allocList=rng.permutation(TABLES["n_blocks"]).astype(np.int32),
             excessList=rng.permutation(TABLES["n_excess"]).astype(np.int32),
             counters=dict(lastFreeBlockId=TABLES["n_blocks"] - len(BLOCKS) - 1, lastFreeExcessListId=40, noVisibleEntries=2),
             pose=pose, maps=[rng.standard_normal((H >> l, W >> l, 4)).astype(np.float32) for l in range(3) for _ in range(2)])
    if variant == "colour":
        s["rgb"] = rng.integers(0, 1 << 32, TABLES["n_blocks"] * 512, dtype=np.uint32)
    if variant == "swapping":
        st, fl = np.zeros(N_TOTAL, np.uint8), np.zeros(N_TOTAL, np.uint8)
        fl[[0, 63, 255, 303]] = 1                       # merged, stored only, a stored block with no hash entry left, pending
        st[[0, 64, 303]] = (2, 2, 1)
        s.update(swapState=st, swapFlags=fl, store=rng.integers(0, 1 << 24, N_TOTAL * 512, dtype=np.uint32))
    return s


def _upload(g, variant):
    (T._upload_map if variant == "swapping" else C._upload_state)(g, _made(variant))


def _assert_same(tag, got, want):
    for k in ("hash", "visType", "vba", "allocList", "excessList", "pose"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (tag, k)
    assert got["counters"] == want["counters"], (tag, got["counters"], want["counters"])
    n = want["counters"]["noVisibleEntries"]
    assert np.asarray(got["visibleIds"])[:n].tobytes() == np.asarray(want["visibleIds"])[:n].tobytes(), (tag, "visibleIds")
    assert all(np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()
               for a, b in zip(got["maps"], want["maps"])), (tag, "maps")
    assert (got["rgb"] is None) == (want["rgb"] is None), (tag, "rgb")
    if want["rgb"] is not None:
        assert got["rgb"].tobytes() == want["rgb"].tobytes(), (tag, "rgb")
    if "swapFlags" in want:
        for k in ("swapState", "swapFlags"):
            assert got[k].tobytes() == want[k].tobytes(), (tag, k)
        ids = np.flatnonzero(want["swapFlags"] == 1)
        assert got["store"].reshape(-1, 512)[ids].tobytes() == want["store"].reshape(-1, 512)[ids].tobytes(), (tag, "store")


def _round_trip(variant, p_save, p_again, p_resized):
    """The made state saved; that file into a fresh context, saved again; and into RESIZED's tables, saved from there.
    Returns the three contexts' states."""
    g = _ctx(variant)
    _upload(g, variant)
    g.save_map(p_save)
    saved = T._state(g)
    g.close()
    g = _ctx(variant)
    g.load_map(p_save)
    g.save_map(p_again)
    loaded = T._state(g)
    g.close()
    g = _ctx(variant, **RESIZED)
    report = g.load_map_resized(p_save)
    g.save_map(p_resized)
    resized = T._state(g)
    vis_capacity = g.params_.vis_capacity
    g.close()
    return saved, loaded, resized, report, vis_capacity


_files = {}


def _done(tmp_path_factory, variant):
    if variant not in _files:
        d = tmp_path_factory.mktemp(variant)
        paths = [d / n for n in ("made.tfmap", "again.tfmap", "resized.tfmap")]
        _files[variant] = (paths, _round_trip(variant, *paths))
    return _files[variant]


@pytest.mark.parametrize("variant", VARIANTS)
def test_save_load_resize(tmp_path_factory, variant):
    paths, (saved, loaded, resized, report, vis_capacity) = _done(tmp_path_factory, variant)
    sw = variant == "swapping"
    rec = MR.records_of(saved)
    at = sorted(list(BLOCKS) + list(NO_BLOCK) + list(ONLY_VIS))
    assert rec["index"].tolist() == at and {0, 63, 64, 255, 256, 303} <= set(at)
    assert int((rec["entry"]["ptr"] >= 0).sum()) == len(BLOCKS)
    if sw:
        assert int(rec["hasStoredData"].sum()) == 4 and saved["hash"]["ptr"][255] == -2 and saved["swapFlags"][255] == 1
    else:
        assert not np.frombuffer(rec.tobytes(), np.uint8).reshape(-1, 24)[:, 21:].any()     # version 1: bytes 21..23 are zero
    # the saved file is the reference writer's
    data = paths[0].read_bytes()
    assert data == MR.pack(saved)
    # the strict load: every table, list and counter of the file, and a save from there gives the file again
    _assert_same("loaded", loaded, MR.unpack(data))
    assert MR.states_equal(loaded, MR.unpack(data))
    assert paths[1].read_bytes() == data
    # the resized load: the serial restatement's state and report
    want, need = Z.resize(saved, RESIZED["n_buckets"], RESIZED["n_excess"], RESIZED["n_blocks"], vis_capacity)
    assert report == need and need["longest_chain"] == len(SAME_BUCKET) and need["records_dropped"] == len(ONLY_VIS)
    assert need["cache_blocks"] == (3 if sw else 0)            # (entry 255's stored block is dropped with its record)
    _assert_same("resized", resized, want)


def _child(out_dir):
    for variant in VARIANTS:
        _round_trip(variant, *(os.path.join(out_dir, f"{variant}{k}.tfmap") for k in range(3)))


def test_chunks_of_one_block(tmp_path_factory, tmp_path):
    """The same three files from a process whose staging buffer holds a single block (the knob is read at tf_create)."""
    env = dict(os.environ, TFUSION_CKPT_CHUNK_BLOCKS="1")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_scene_small as S; "
            f"S._child({str(tmp_path)!r})")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    for variant in VARIANTS:
        paths, _ = _done(tmp_path_factory, variant)
        for k, p in enumerate(paths):
            assert (tmp_path / f"{variant}{k}.tfmap").read_bytes() == p.read_bytes(), (variant, p.name)
