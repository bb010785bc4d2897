"""The reference of the free views' whole reading (TF_VIEW_WHOLE, include/tfusion_hip.h), and the scene and cases its
tests share.

The whole view of a swapping scene (hash, vba, state, flags, store) is the resident view (view_ref.stages) of the
scene RESOLVED over both tiers (mesh_whole_ref.resolve, DESIGN.md §5 "The whole map"), in an oracle whose n_blocks
is the number of resolving entries: every entry that resolves keeps its index, position and chain link and holds a
block of its own, every other entry is unallocated.

The tiered standard scene: view_ref.standard_scene() with every live entry drawn into one of mesh_whole_ref.CLASSES
(p = .3 / .25 / .25 / .1 / .1), so that the surface the standard scene shows is spread over all rows of the table:

    active   state 2, nothing stored
    stored   the block moved to store[i], its VBA block overwritten with random voxels of w > 0 (nobody's now),
             ptr -1, flag 1, state 0 or 1
    pending  flag 1, state 0 or 1; the stored copy holds weight (w + 1) // 2 and the sdf jittered by +-300, the active
             block weight w // 2 -- one in five has an empty active block (32767, 0) and the stored copy whole
    stale    flag 1, state 2 (merged), random voxels left in the store: they must not show
    lost     ptr -1, flag 0: gone

SEED is the first seed at which every condition of tests/test_view_whole_ref.py holds.

Cases A-F are view_ref.CASES; case G is case A with every block shifted by +128 blocks in x and the pose with it
(blocks -11 .. 14 become 117 .. 142): the scene then straddles the block grid's edge at 128, so half of it is found
through the hash walk alone.  The table is re-hashed with synth.build_hash and everything an entry owns moves with it.
"""
import functools

import numpy as np

import mesh_whole_ref as WR
import view_ref as V
from topfusion_amd import synth

SEED = 0
SHIFT_G = 128                                     # blocks, along x
TYPES = (0, 1, 2, 3, 4)

_cA = V.CASES["A"]
_poseG = _cA[2].copy()
_poseG[0, 3] += np.float32(SHIFT_G * 8 * V.TABLES["voxelSize"])
CASES = dict(V.CASES)
CASES["G"] = (_cA[0], _cA[1], _poseG, {})


@functools.lru_cache(maxsize=None)
def tiered_scene(seed=SEED):
    """dict(hash, vba, state, flags, store, cls, counters): the tiered standard scene; read-only."""
    from topfusion_amd.topfu import VOXEL_DTYPE
    s = V.standard_scene()
    h = s["hash"].copy()
    vba = s["vba"].copy()
    n_total = len(h)
    rng = np.random.default_rng(seed)
    store = np.zeros(n_total * 512, VOXEL_DTYPE)
    store["sdf"] = 32767
    state = np.zeros(n_total, np.uint8)
    flags = np.zeros(n_total, np.uint8)
    cls = np.full(n_total, -1, np.int8)
    live = np.flatnonzero(h["ptr"] >= 0)
    draw = rng.choice(5, len(live), p=[0.3, 0.25, 0.25, 0.1, 0.1])
    sv, av = store.reshape(-1, 512), vba.reshape(-1, 512)
    for i, c in zip(live, draw):
        cls[i] = c
        p = h["ptr"][i]
        if c == 0:
            state[i] = 2
        elif c == 1:
            state[i] = rng.integers(0, 2)
            flags[i] = 1
            sv[i] = av[p]
            av[p] = WR._random_voxels(rng, 512, [1, 5])
            h["ptr"][i] = -1
        elif c == 2:
            state[i] = rng.integers(0, 2)
            flags[i] = 1
            sv[i] = av[p]
            if rng.random() < 0.2:
                av[p]["sdf"], av[p]["w"] = 32767, 0
            else:
                w = av[p]["w"].astype(np.int32)
                jit = sv[i]["sdf"].astype(np.int32) + rng.integers(-300, 301, 512)
                sv[i]["sdf"] = np.clip(jit, -32767, 32767).astype(np.int16)
                sv[i]["w"] = ((w + 1) // 2).astype(np.uint8)
                av[p]["w"] = (w // 2).astype(np.uint8)
        elif c == 3:
            state[i] = 2
            flags[i] = 1
            sv[i] = WR._random_voxels(rng, 512, [1, 5])
        else:
            state[i] = rng.integers(0, 2)
            h["ptr"][i] = -1
    out = dict(hash=h, vba=vba, state=state, flags=flags, store=store, cls=cls, counters=s["counters"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def shifted_scene(seed=SEED):
    """The tiered scene moved by SHIFT_G blocks along x (case G): positions re-hashed, the pointers, swap state, flags,
    stored blocks and classes carried over to each block's new entry."""
    from topfusion_amd.topfu import HASH_DTYPE
    t = tiered_scene(seed)
    h0 = t["hash"]
    held = np.flatnonzero(t["cls"] >= 0)                     # every entry that was live in the standard scene
    pos = np.stack([h0["x"][held], h0["y"][held], h0["z"][held]], -1).astype(np.int64)
    pos[:, 0] += SHIFT_G
    nb, ne = V.TABLES["n_buckets"], V.TABLES["n_excess"]
    h, entry, last_excess = synth.build_hash(pos, nb, ne, HASH_DTYPE)
    h["ptr"][entry] = h0["ptr"][held]
    state, flags, cls = np.zeros_like(t["state"]), np.zeros_like(t["flags"]), np.full_like(t["cls"], -1)
    store = np.zeros_like(t["store"])
    store["sdf"] = 32767
    state[entry], flags[entry], cls[entry] = t["state"][held], t["flags"][held], t["cls"][held]
    store.reshape(-1, 512)[entry] = t["store"].reshape(-1, 512)[held]
    out = dict(hash=h, vba=t["vba"], state=state, flags=flags, store=store, cls=cls,
               counters=(t["counters"][0], last_excess, 0))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def scene_of(name):
    return shifted_scene() if name == "G" else tiered_scene()


def whole_stages(O, tiers, cols, rows, c2w, vp=None, maxW=WR.MAXW, tables=V.TABLES, intr=None, types=TYPES):
    """view_ref.stages of the resolved scene: the whole view of the five tier buffers `tiers` (a dict or a tuple
    hash, vba, state, flags, store)."""
    if isinstance(tiers, dict):
        tiers = tuple(tiers[k] for k in ("hash", "vba", "state", "flags", "store"))
    h2, v2 = WR.resolve(*tiers, maxW=maxW)
    ov = V.oracle_for(O, cols, rows, intr=intr, tables=tables, **dict(vp or {}, n_blocks=len(v2) // 512, maxW=maxW))
    return V.stages(O, ov, h2, v2, None, (0, 0), c2w, types=types)


def resident_stages(O, tiers, cols, rows, c2w, vp=None, tables=V.TABLES, intr=None, types=TYPES):
    """view_ref.stages of the scene as it lies in the VBA: the resident view of the same buffers."""
    h, vba = (tiers["hash"], tiers["vba"]) if isinstance(tiers, dict) else tiers[:2]
    ov = V.oracle_for(O, cols, rows, intr=intr, tables=tables, **dict(vp or {}))
    return V.stages(O, ov, h, vba, None, (0, 0), c2w, types=types)


@functools.lru_cache(maxsize=None)
def case_reference(name, maxW=WR.MAXW):
    """The whole reading's stages of a case over its scene, computed once."""
    from oracle import oracle as O
    cols, rows, c2w, vp = CASES[name]
    return whole_stages(O, scene_of(name), cols, rows, c2w, vp, maxW=maxW)


@functools.lru_cache(maxsize=None)
def case_resident(name):
    """The resident reading's stages of a case over the same (tiered) scene, computed once."""
    from oracle import oracle as O
    cols, rows, c2w, vp = CASES[name]
    return resident_stages(O, scene_of(name), cols, rows, c2w, vp)


def hit_classes(name, ref):
    """Per hit pixel of a case's raycast result the class of the block its surface point lies in (-1: none found):
    (classes of the hit pixels, block x of the hit pixels)."""
    t = scene_of(name)
    h = t["hash"]
    held = np.flatnonzero(t["cls"] >= 0)
    at = {(int(h["x"][i]), int(h["y"][i]), int(h["z"][i])): int(t["cls"][i]) for i in held}
    ray = ref["raycast"]
    pts = ray[ray[..., 3] > 0][:, :3]
    blk = np.floor(np.floor(pts + np.float32(0.5)) / 8).astype(np.int64)      # the block of ROUND(pt)
    return np.array([at.get(tuple(b), -1) for b in blk], np.int64), blk[:, 0]
