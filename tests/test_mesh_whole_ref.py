"""The whole reading's reference (tests/mesh_whole_ref.py) and its hand-made scene, on the CPU: the scene
holds every class and sub-case of the resolution table where a cube can see them, and the numpy combine is
the oracle's CombineVoxelInformation bit for bit.  These are conditions on the INPUT of the GPU tests
(tests/test_gpu_mesh_whole.py); the seed (mesh_whole_ref.SEED) was picked so that they hold."""
import itertools

import numpy as np
import pytest

import mesh_ref as M
import mesh_whole_ref as WR
from topfusion_amd import synth


@pytest.fixture(scope="module")
def case():
    return WR.two_tier_case()


def test_classes_and_sub_cases(case):
    cls, sub, h = case["cls"], case["sub"], case["hash"]
    state, flags = case["state"], case["flags"]
    for c in range(5):
        assert (cls == c).any(), WR.CLASSES[c]
    for s in (0, 1):
        assert ((cls == 1) & (state == s)).any(), f"stored only, state {s}"
        assert ((cls == 2) & (state == s)).any(), f"pending, state {s}"
    assert ((cls == 1) & (h["ptr"] == -1) & (flags == 1)).sum() == (cls == 1).sum()
    assert ((cls == 2) & (h["ptr"] >= 0) & (flags == 1) & (state != 2)).sum() == (cls == 2).sum()
    assert ((cls == 3) & (h["ptr"] >= 0) & (flags == 1) & (state == 2)).sum() == (cls == 3).sum()
    assert ((cls == 4) & (h["ptr"] == -1) & (flags == 0)).sum() == (cls == 4).sum()
    # inside the pending merges: oldW == 0, the maxW clamp and an empty active block
    pend = np.nonzero(cls == 2)[0]
    sv = case["store"].reshape(-1, 512)[pend]
    av = case["vba"].reshape(-1, 512)[h["ptr"][pend]]
    assert (sv["w"] == 0).any() and ((sv["w"] == 0) & (av["w"] > 0)).any(), "oldW == 0"
    assert (sv["w"].astype(int) + av["w"] > WR.MAXW).any(), "the maxW clamp"
    assert (sub[pend] >= 2).any() and (av["w"].max(1) == 0).any(), "an empty active block"
    # the table's rows are what the classes were built to be
    row = WR.classify(h, state, flags)
    assert np.array_equal(row[cls >= 0], np.array([0, 2, 1, 0, -1])[cls[cls >= 0]])


def _corner_cubes(case):
    """Over the cubes of every resolving entry that touch another block: (classes of the blocks its corners
    come from, whether a corner block is stored-only and outside the block grid), for the valid ones."""
    h, cls = case["hash"], case["cls"]
    h2, v2 = WR.resolve(h, case["vba"], case["state"], case["flags"], case["store"])
    w = v2["w"].reshape(-1, 8, 8, 8)                            # [block, z, y, x]
    where = {(int(h2["x"][i]), int(h2["y"][i]), int(h2["z"][i])): i for i in np.nonzero(h2["ptr"] >= 0)[0]}
    out = []
    for (bx, by, bz), i in where.items():
        for x, y, z in itertools.product(range(8), repeat=3):
            if max(x, y, z) < 7:
                continue
            ents, ok = set(), True
            for dx, dy, dz in itertools.product((0, 1), repeat=3):
                gx, gy, gz = x + dx, y + dy, z + dz
                j = where.get((bx + (gx >> 3), by + (gy >> 3), bz + (gz >> 3)))
                if j is None or w[h2["ptr"][j], gz & 7, gy & 7, gx & 7] == 0:
                    ok = False
                    break
                ents.add(j)
            if ok:
                far = any(cls[j] == 1 and not all(-128 <= int(h[k][j]) < 128 for k in "xyz") for j in ents)
                out.append(({int(cls[j]) for j in ents}, far))
    return out


def test_cubes_across_tiers(case):
    cubes = _corner_cubes(case)
    assert any(len(c) >= 3 for c, _ in cubes), "no valid cube with corners from three classes"
    assert any(far for _, far in cubes), "no valid cube reaches a stored-only block outside the block grid"


def test_whole_and_resident_differ(case):
    whole = case["tris"]
    resident = M.extract(case["hash"], case["vba"], M.VOXEL_SIZE, M.RANDOM["n_buckets"])
    a = {t.tobytes() for t in whole}
    b = {t.tobytes() for t in resident}
    assert a - b, "the whole reading adds nothing"
    assert b - a, "no resident triangle changed (a pending merge meshes from the combined voxels)"
    assert a & b, "nothing in common (active-only and stale-store entries mesh from their active data in both)"
    assert len(whole) > len(resident) > 0


def test_no_stored_data_is_resident():
    """Without stored data the resolved scene meshes as the raw one does."""
    h, vba, want, _ = M.random_case()
    n_total = len(h)
    z = np.zeros(n_total, np.uint8)
    store = np.zeros(n_total * 512, vba.dtype)
    got = WR.extract(h, vba, z, z, store, M.VOXEL_SIZE, M.RANDOM["n_buckets"])
    assert got.tobytes() == want.tobytes()


def test_store_offset_fits_an_int():
    """The whole reading addresses a stored voxel as entry * 512 + lin in an int, so tf_create refuses a swapping
    table of 2^22 entries or more (the parameters are checked before any device is touched)."""
    import ctypes
    from topfusion_amd import _lib
    L = _lib.load()
    ctx = ctypes.c_void_p()
    big = _lib.default_params(n_buckets=1 << 22, n_excess=16, use_swapping=1, swap_transfer_blocks=16)
    assert (big.n_buckets + big.n_excess) * 512 > 2 ** 31 - 1
    assert L.tf_create(ctypes.byref(big), ctypes.byref(ctx)) == _lib.TF_INVALID_ARG
    ref = _lib.default_params(use_swapping=1)                     # the reference's table: far below the limit
    assert (ref.n_buckets + ref.n_excess) * 512 + 511 <= 2 ** 31 - 1


def test_combine_is_the_oracles(case, oracle_mod):
    """The pending merges (all put into state 1) through the oracle's IntegrateGlobalIntoLocal: its VBA blocks
    equal resolve()'s, bit for bit."""
    cfg = M.RANDOM
    fx, fy, cx, cy = synth.intrinsics(96, 72)
    o = oracle_mod.Oracle(oracle_mod.default_params(cols=96, rows=72, fx=fx, fy=fy, cx=cx, cy=cy, use_swapping=1,
                                                    swap_transfer_blocks=cfg["n_buckets"] + cfg["n_excess"], **cfg))
    assert o.params.maxW == WR.MAXW
    h, cls = case["hash"], case["cls"]
    state = case["state"].copy()
    pend = np.nonzero(cls == 2)[0]
    state[pend] = 1
    o.load_scene_state(h, case["vba"], np.arange(cfg["n_blocks"], dtype=np.int32), np.arange(cfg["n_excess"], dtype=np.int32),
                       np.zeros(o.params.vis_capacity, np.int32), np.zeros(len(h), np.uint8), (-1, -1, 0),
                       swap_state=state, swap_stored_flags=case["flags"], swap_stored=case["store"])
    o.swap_in()
    assert (o.swap_state()[pend] == 2).all()
    got = o.vba().reshape(-1, 512)[h["ptr"][pend]]
    h2, v2 = WR.resolve(h, case["vba"], state, case["flags"], case["store"])
    want = v2.reshape(-1, 512)[h2["ptr"][pend]]
    assert np.array_equal(got["sdf"], want["sdf"]) and np.array_equal(got["w"], want["w"])
    # ... and it changed something: the merge is not the identity on this data
    raw = case["vba"].reshape(-1, 512)[h["ptr"][pend]]
    assert not np.array_equal(raw["sdf"], want["sdf"])
