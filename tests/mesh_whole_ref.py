"""CPU restatement of the mesher's whole reading (DESIGN.md §Mesh extraction, the whole map) in numpy.

The whole mesh of a swapping scene is the resident mesh (mesh_ref / mesh_attr_ref) of the scene RESOLVED
over both tiers:

    resolve(hash, vba, state, flags, store, maxW) -> (hash', vba')

Every entry that resolves keeps its index, position and chain link and gets a fresh virtual block (ptr
0, 1, 2, ... in ascending entry order) filled by the resolution table; every other entry is unallocated
(ptr -2, its chain link kept so the walk still passes through it).  With p = hash[i].ptr, f = flags[i]
(hasStoredData), s = state[i]:

    p >= 0 and (f == 0 or s == 2)   the active block (a store left behind by a finished merge is stale)
    p >= 0, f == 1, s != 2          CombineVoxelInformation(stored, active, maxW) per voxel
    p == -1, f == 1                 the stored block as it is
    p == -1, f == 0, or p < -1      missing

The combine is float32 and written from its definition: oldW == 0 keeps the active voxel whole; else
newF = (oldW * oldF + newW * newF) / (oldW + newW) with every operation rounded on its own, w = min(oldW +
newW, maxW), sdf = (short)(newF * 32767) truncating.  SDF_shortToFloat is the float32 division s / 32767
(tests/test_oracle.py::test_short_to_float_division_exact), so plain numpy states it.
"""
import itertools

import numpy as np

import mesh_ref as M

MAXW = 100                       # default_params' maxW
CLASSES = ("active", "stored", "pending", "stale", "lost")


def combine(stored, active, maxW):
    """CombineVoxelInformation(src = stored, dst = active) on VOXEL_DTYPE arrays of one shape."""
    out = active.copy()
    oldW = stored["w"].astype(np.int32)
    newW = active["w"].astype(np.int32)
    oldF = (stored["sdf"].astype(np.float32) / np.float32(32767.0)).astype(np.float32)
    newF = (active["sdf"].astype(np.float32) / np.float32(32767.0)).astype(np.float32)
    a = (oldW.astype(np.float32) * oldF).astype(np.float32)
    b = (newW.astype(np.float32) * newF).astype(np.float32)
    tot = oldW + newW
    with np.errstate(invalid="ignore", divide="ignore"):
        f = ((a + b).astype(np.float32) / tot.astype(np.float32)).astype(np.float32)
        sdf = np.trunc((f * np.float32(32767.0)).astype(np.float32))
    go = oldW > 0
    out["sdf"] = np.where(go, np.where(go, sdf, 0).astype(np.int32).astype(np.int16), active["sdf"])
    out["w"] = np.where(go, np.minimum(tot, maxW), newW).astype(np.uint8)
    return out


def classify(h, state, flags):
    """Per entry the table's row: 0 active, 1 combined, 2 stored, -1 missing."""
    p, f, s = h["ptr"], np.asarray(flags) != 0, np.asarray(state)
    row = np.full(len(h), -1, np.int8)
    row[(p >= 0) & (~f | (s == 2))] = 0
    row[(p >= 0) & f & (s != 2)] = 1
    row[(p == -1) & f] = 2
    return row


def resolve(h, vba, state, flags, store, maxW=MAXW):
    """(hash', vba'): see the module docstring.  vba' holds one block per resolving entry."""
    row = classify(h, state, flags)
    ids = np.nonzero(row >= 0)[0]
    h2 = h.copy()
    h2["ptr"] = -2
    h2["ptr"][ids] = np.arange(len(ids))
    v = np.asarray(vba).reshape(-1, 512)
    st = np.asarray(store).reshape(-1, 512)
    out = np.zeros((max(len(ids), 1), 512), v.dtype)
    out["sdf"] = 32767
    for k, i in enumerate(ids):
        if row[i] == 0:
            out[k] = v[h["ptr"][i]]
        elif row[i] == 1:
            out[k] = combine(st[i], v[h["ptr"][i]], maxW)
        else:
            out[k] = st[i]
    out["pad"] = 0
    return h2, out.reshape(-1)


def extract(h, vba, state, flags, store, voxel_size, n_buckets, maxW=MAXW, normals=False):
    """The whole reading's triangles (and normals): the resident references on the resolved scene."""
    h2, v2 = resolve(h, vba, state, flags, store, maxW)
    if not normals:
        return M.extract(h2, v2, voxel_size, n_buckets)
    import mesh_attr_ref as A
    tris, nrm, _ = A.extract_attr(h2, v2, None, voxel_size, n_buckets)
    return tris, nrm


# ---- the hand-made two-tier scene -------------------------------------------------------------------------
SEED = 0                         # the first seed at which every condition of tests/test_mesh_whole_ref.py holds
BOUNDARY = [(127, 0, 0), (128, 0, 0), (-129, 1, -1), (-128, 1, -1), (5, 127, 3), (5, 128, 3), (2, -129, 7), (2, -128, 7),
            (-4, 9, 127), (-4, 9, 128), (6, 6, -129), (6, 6, -128), (127, 127, 127), (128, 128, 128), (127, 128, 127),
            (-129, -129, -129), (-128, -128, -128), (-128, -129, -128)]
FAR = [(300 + dx, -200 + dy, 250 + dz) for dx, dy, dz in itertools.product((0, 1), repeat=3)]

_cache = {}


def _random_voxels(rng, n, wset):
    from topfusion_amd.topfu import VOXEL_DTYPE
    v = np.zeros(n, VOXEL_DTYPE)
    sdf = rng.integers(-32768, 32768, n).astype(np.int16)
    pick = rng.random(n)
    sdf[pick < 0.08] = 0
    sdf[(pick >= 0.08) & (pick < 0.14)] = 32767
    sdf[(pick >= 0.14) & (pick < 0.20)] = -32767
    v["sdf"] = sdf
    v["w"] = rng.choice(np.array(wset, np.uint8), n)
    return v


def two_tier_case(seed=SEED):
    """The hand-made scene of both tiers, capacities mesh_ref.RANDOM: mesh_ref.random_case()'s blocks plus the
    grid-boundary and far-cluster positions, every allocated entry drawn into one of CLASSES (and a sub-case).
    Returns a dict: hash, vba, state, flags, store (all read-only), cls (class index per entry, -1 unallocated),
    sub (the sub-case: the swap state given to a stored / pending entry), tris, normals (the reference's)."""
    key = ("two_tier", seed)
    if key in _cache:
        return _cache[key]
    from topfusion_amd import synth
    from topfusion_amd.topfu import HASH_DTYPE, VOXEL_DTYPE
    cfg = M.RANDOM
    h0 = M.random_case()[0]
    live0 = np.nonzero(h0["ptr"] >= 0)[0]
    pos = np.stack([h0["x"][live0], h0["y"][live0], h0["z"][live0]], -1).astype(np.int64)
    pos = np.concatenate([pos, np.array(BOUNDARY + FAR, np.int64)])
    h, entry, _ = synth.build_hash(pos, cfg["n_buckets"], cfg["n_excess"], HASH_DTYPE)
    n_total = cfg["n_buckets"] + cfg["n_excess"]
    assert len(pos) <= cfg["n_blocks"]
    rng = np.random.default_rng(seed)
    perm = rng.permutation(cfg["n_blocks"])[:len(pos)]
    h["ptr"][entry] = perm
    vba = _random_voxels(rng, cfg["n_blocks"] * 512, [0, 1, 1, 1, 5])
    store = np.zeros(n_total * 512, VOXEL_DTYPE)
    store["sdf"] = 32767
    state = np.zeros(n_total, np.uint8)
    flags = np.zeros(n_total, np.uint8)
    cls = np.full(n_total, -1, np.int8)
    sub = np.zeros(n_total, np.int8)
    draw = rng.choice(5, len(pos), p=[0.3, 0.25, 0.25, 0.1, 0.1])
    sv = store.reshape(-1, 512)
    av = vba.reshape(-1, 512)
    for b, i in enumerate(entry):
        c = int(draw[b])
        cls[i] = c
        if c == 0:                                   # active only
            state[i] = 2
        elif c == 1:                                 # stored only: ptr -1, flag 1, state 0 or 1
            sub[i] = state[i] = rng.integers(0, 2)
            flags[i] = 1
            sv[i] = _random_voxels(rng, 512, [0, 1, 1, 1, 5])
            av[h["ptr"][i]] = _random_voxels(rng, 512, [1, 5])    # what the freed block holds now is nobody's
            h["ptr"][i] = -1
        elif c == 2:                                 # pending merge: ptr >= 0, flag 1, state 1 or 0
            sub[i] = state[i] = rng.integers(0, 2)
            flags[i] = 1
            sv[i] = _random_voxels(rng, 512, [0, 1, 5, 100])
            av[h["ptr"][i]] = _random_voxels(rng, 512, [0, 1, 5])
            if rng.random() < 0.2:                   # an empty active block (freshly reallocated)
                av[h["ptr"][i]]["sdf"], av[h["ptr"][i]]["w"] = 32767, 0
                sub[i] += 2
        elif c == 3:                                 # merged, the store stale: ptr >= 0, flag 1, state 2
            state[i] = 2
            flags[i] = 1
            sv[i] = _random_voxels(rng, 512, [1, 5])
        else:                                        # lost: ptr -1, flag 0
            state[i] = rng.integers(0, 2)
            h["ptr"][i] = -1
    tris, normals = extract(h, vba, state, flags, store, M.VOXEL_SIZE, cfg["n_buckets"], normals=True)
    out = dict(hash=h, vba=vba, state=state, flags=flags, store=store, cls=cls, sub=sub, tris=tris, normals=normals,
               pos=pos, entry=entry)
    for a in out.values():
        a.setflags(write=False)
    _cache[key] = out
    return out
