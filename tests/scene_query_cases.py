"""The inputs of the scene query tests (tf_scene_query / tf_scene_slice, include/tfusion_hip.h), in one place:
tests/test_scene_query_cases.py asserts the conditions they are meant to meet on the CPU, and
tests/test_gpu_scene_query.py feeds them to the HIP kernels.

The expected values are the reference's own (tests/golden/stage_pin_<scene>_sdf_read.bin, at pin_scenes.sdf_points)
where the reference was run, and everywhere else the oracle's per-point functions -- Oracle.sdf_read with a fresh
IndexCache, normal_from_sdf, colour_at -- over the same hash and voxels; under the whole reading over the scene
resolved across both tiers (mesh_whole_ref.resolve).  A point outside the range guard is never given to the oracle:
its expected record is the header's "nothing".

Everything is made from integers (pin_scenes._h: lowbias32 hashing, no np.random) and rounded to float32 once."""
import functools

import numpy as np

import pin_scenes as P
from topfusion_amd import synth
from vbh_ref import HASH_DTYPE, VOXEL_DTYPE

OUTS = ("sdf_nearest", "entry", "sdf", "confidence", "normal", "colour")
LIMIT = np.float32(262136.0)                 # +-32767 * 8
SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
MIN_PER_CLASS = 16


# ---- the guard and the expected record ---------------------------------------------------------------------
def in_range(pts):
    """The header's rule on voxel-unit float32 coordinates: all three in [-262136, 262136]; NaN fails."""
    p = np.asarray(pts, np.float32)
    with np.errstate(invalid="ignore"):
        return ((p >= -LIMIT) & (p <= LIMIT)).all(-1)


def nothing(n):
    return dict(sdf_nearest=np.ones(n, np.float32), entry=np.full(n, -1, np.int32), sdf=np.ones(n, np.float32),
                confidence=np.zeros(n, np.float32), normal=np.zeros((n, 3), np.float32), colour=np.zeros((n, 4), np.uint8))


def expected(o, vox_pts, colour=True):
    """What a query returns at the voxel-unit points (n, 3): the oracle `o`'s reads where the guard passes, nothing
    elsewhere.  Each read with a fresh IndexCache."""
    p = np.ascontiguousarray(vox_pts, np.float32).reshape(-1, 3)
    ok = in_range(p)
    out = nothing(len(p))
    if ok.any():
        q = p[ok]
        u, vm, i, cs, cf = o.sdf_read(q, carried=0)
        assert np.array_equal(i.view(np.uint32), cs.view(np.uint32))       # the two interpolated reads agree
        out["sdf_nearest"][ok], out["entry"][ok], out["sdf"][ok], out["confidence"][ok] = u, vm - 1, i, cf
        out["normal"][ok] = o.normal_from_sdf(q)
        if colour:
            out["colour"][ok] = o.colour_at(q)
    if not colour:
        del out["colour"]
    return out


def golden_expected(name):
    """The reference's record at pin_scenes.sdf_points(name), from the committed golden (the fresh-cache column)."""
    g = P.read_pin(P.golden_path(name, "sdf_read"))
    two = lambda k: g[k].reshape(-1, 2)
    return dict(sdf_nearest=two("uninterp")[:, 0].copy(), entry=(two("vm")[:, 0] - 1).astype(np.int32),
                sdf=two("interp")[:, 0].copy(), confidence=two("conf")[:, 0].copy(),
                normal=g["normal"].reshape(-1, 3).copy(), colour=g["colour"].reshape(-1, 4).copy())


# ---- metres ------------------------------------------------------------------------------------------------
def metre_points(name):
    """pin_scenes.sdf_points in metres: each coordinate times voxelSize, in float32."""
    return (P.sdf_points(name) * P.VOXEL_SIZE).astype(np.float32)


def metres_to_voxels(pts_m, voxel_size):
    """The conversion the header states: times the float32 1.0f / voxelSize, one rounding."""
    return (np.asarray(pts_m, np.float32) * (np.float32(1) / np.float32(voxel_size))).astype(np.float32)


# ---- the guard's points --------------------------------------------------------------------------------------
# the first float32 beyond the limit: 262136 lies below 2^18, where the step is 1/64, so that is 262136.015625; the
# value one 1/32 step out, 262136.03125, is kept beside it
_BEYOND = np.nextafter(LIMIT, np.float32(np.inf), dtype=np.float32)
_BEYOND32 = np.float32(262136.03125)
GUARD_VALUES = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, LIMIT, -LIMIT, _BEYOND, -_BEYOND, _BEYOND32, -_BEYOND32], np.float32)


def guard_points(name="sphere"):
    """Every GUARD_VALUES entry in each axis of an otherwise ordinary point of the scene, each followed by three
    ordinary points (so no wave is all of one kind): (points (n, 3) float32 voxel units, in-range mask)."""
    base = P.sdf_points(name, 4 * 3 * len(GUARD_VALUES))
    rows = []
    k = 0
    for ax in range(3):
        for v in GUARD_VALUES:
            p = base[k].copy()
            p[ax] = v
            rows += [p, base[k + 1], base[k + 2], base[k + 3]]
            k += 4
    pts = np.array(rows, np.float32)
    return pts, in_range(pts)


# ---- a scene with blocks outside the block grid --------------------------------------------------------------
GRID_HALF = 128
FAR_C = np.array([200, -300, 1000])
FAR_CLASSES = ("in-grid", "out-of-grid", "swapped-out", "missing")


def _in_grid(b):
    b = np.asarray(b)
    return ((b >= -GRID_HALF) & (b < GRID_HALF)).all(-1)


@functools.lru_cache(maxsize=None)
def far_scene():
    """A made scene in the pin scenes' table sizes: a 4 x 4 x 4 box of blocks inside the grid, one around block
    (200, -300, 1000) outside it, a pair straddling the grid's edge at x = 127 | 128, and a pair of positions near
    FAR_C that share a bucket (pin_scenes._collision_groups' method), so one of them is found at the end of an excess
    chain.  About one block in five is swapped out (ptr -1), the chained pair never.  Voxels: hashed sdf over the
    whole short range, w from {0, 1, 5, 100}; the colour plane hashed."""
    box = np.array([(x, y, z) for z in range(4) for y in range(4) for x in range(4)], np.int64)
    near = box + np.array([-2, -2, 10])
    far = box + FAR_C - 2
    edge = np.array([(127, 0, 12), (128, 0, 12), (126, 0, 12), (129, 0, 12)], np.int64)
    avoid = {tuple(p) for p in np.concatenate([near, far, edge]).tolist()}
    pair = P._collision_groups(tuple(FAR_C - 20), tuple(FAR_C + 20), 2, 1, avoid)[0]
    blocks = np.concatenate([near, far, edge, pair])
    h, entry, last_excess = synth.build_hash(blocks, P.N_BUCKETS, P.N_EXCESS, HASH_DTYPE)
    perm = np.argsort(P._h(122, np.arange(P.N_BLOCKS)), kind="stable")[:len(blocks)]
    h["ptr"][entry] = perm
    out = P._h(125, blocks[:, 0], blocks[:, 1], blocks[:, 2]) % np.uint32(5) == 0
    out[-6:] = False                                                   # the edge blocks and the chained pair stay
    h["ptr"][entry[out]] = -1
    i = np.arange(P.N_BLOCKS * 512, dtype=np.int64)
    vba = np.zeros(P.N_BLOCKS * 512, VOXEL_DTYPE)
    vba["sdf"] = (P._h(123, i) >> np.uint32(16)).astype(np.int64) - 32768
    vba["w"] = np.array([0, 1, 5, 100], np.uint8)[P._h(124, i) % np.uint32(4)]
    s = dict(hash=h, vba=vba, vba_rgb=P._colours(P.N_BLOCKS * 512), blocks=blocks, entry=entry, swapped=out, pair=pair,
             last_excess=last_excess)
    for a in s.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s


def _local64(seed, i):
    """1/64-voxel positions inside a block, as pin_scenes.sdf_points draws them: integers, half-integers, the +face
    (the +1 neighbours lie in the next block), just below the origin, anything."""
    kind = P._h(seed, i) % np.uint32(6)
    loc = np.stack([P._h(seed + 1 + k, i) % np.uint32(8 * 64) for k in range(3)], -1).astype(np.int64)
    loc = np.where((kind == 0)[:, None], loc // 64 * 64, loc)
    loc = np.where((kind == 1)[:, None], loc // 64 * 64 + 32, loc)
    ax = (P._h(seed + 4, i) % np.uint32(3)).astype(np.int64)
    onax = np.arange(3)[None] == ax[:, None]
    loc = np.where((kind == 2)[:, None] & onax, 7 * 64 + (loc % 64), loc)
    loc = np.where((kind == 3)[:, None], 7 * 64 + (loc % 64), loc)
    loc = np.where((kind == 4)[:, None] & onax, -(loc % 64) - 1, loc)
    return loc


def far_points(n=512):
    """(points (n, 3) float32 voxel units, class index per point): point i is of class i % 4 -- in a resident block
    inside the grid, in a resident block outside it (every 8th of those in the chained pair), in a swapped-out block,
    in no block (empty space beside the near box and beside the far one alternately)."""
    s = far_scene()
    b, sw = s["blocks"], s["swapped"]
    ing = _in_grid(b)
    pools = [b[ing & ~sw], b[~ing & ~sw], b[sw]]
    i = np.arange(n, dtype=np.int64)
    cls = (i % 4).astype(np.int64)
    blk = np.zeros((n, 3), np.int64)
    for c, pool in enumerate(pools):
        m = cls == c
        blk[m] = pool[P._h(131 + c, i[m]) % np.uint32(len(pool))]
    m = (cls == 1) & (i % 32 == 1)
    blk[m] = s["pair"][(i[m] // 32) % 2]
    m = cls == 3
    empty = np.where(((i[m] // 4) % 2 == 0)[:, None], np.array([7, 7, 3]), FAR_C + np.array([9, -9, 5]))
    blk[m] = empty + np.stack([P._h(141 + k, i[m]) % np.uint32(3) for k in range(3)], -1).astype(np.int64)
    p64 = blk * 8 * 64 + _local64(151, i)
    return (p64.astype(np.float64) / 64).astype(np.float32), cls


def far_point_classes(pts):
    """The class of ROUND(pt)'s block per point, from the scene itself: 0 resident in the grid, 1 resident outside it,
    2 swapped out, 3 no entry."""
    s = far_scene()
    at = {tuple(p): (2 if w else (0 if g else 1)) for p, w, g in zip(s["blocks"].tolist(), s["swapped"].tolist(), _in_grid(s["blocks"]).tolist())}
    p = np.asarray(pts, np.float32)
    r = np.where(p < 0, p - np.float32(0.5), p + np.float32(0.5)).astype(np.int64)          # ROUND: (int)(x -+ 0.5)
    return np.array([at.get(tuple(v), 3) for v in (r >> 3).tolist()], np.int64)


# ---- the whole reading -----------------------------------------------------------------------------------------
WHOLE_CLASSES = ("resident", "stored-only", "pending", "face")


@functools.lru_cache(maxsize=None)
def whole_points(n=256):
    """(points (n, 3) float32 voxel units, class per point) over view_whole_ref.tiered_scene(): point i is of class
    i % 4 -- inside a resident block (active or with a stale store), a stored-only block, a block with a pending merge,
    and on the face between a resident and a stored-only block (within the last voxel before it, so the +1 corners and
    half of the gradient's reads lie across)."""
    import view_whole_ref as VW
    t = VW.tiered_scene()
    h, c = t["hash"], t["cls"]
    pos = lambda m: np.stack([h["x"][m], h["y"][m], h["z"][m]], -1).astype(np.int64)
    res, sto, pen = pos((c == 0) | (c == 3)), pos(c == 1), pos(c == 2)
    stored = {tuple(p) for p in sto.tolist()}
    faces = [(p, ax) for p in res.tolist() for ax in range(3) if tuple(np.add(p, np.eye(3, dtype=np.int64)[ax])) in stored]
    assert len(faces) >= MIN_PER_CLASS, len(faces)
    i = np.arange(n, dtype=np.int64)
    cls = i % 4
    blk = np.zeros((n, 3), np.int64)
    for k, pool in enumerate((res, sto, pen)):
        m = cls == k
        blk[m] = pool[P._h(161 + k, i[m]) % np.uint32(len(pool))]
    loc = _local64(171, i)
    m = np.flatnonzero(cls == 3)
    pick = P._h(165, m) % np.uint32(len(faces))
    for j, f in zip(m, pick):
        p, ax = faces[int(f)]
        blk[j] = p
        loc[j] = loc[j] % (8 * 64)
        loc[j, ax] = 7 * 64 + 1 + loc[j, ax] % 63                      # strictly inside the last voxel: floor + 1 is across
    p64 = blk * 8 * 64 + loc
    return (p64.astype(np.float64) / 64).astype(np.float32), cls


def whole_oracle(O, tiers, tables, cols, rows):
    """An oracle holding the scene resolved over both tiers (mesh_whole_ref.resolve): every resolving entry keeps its
    index and chain link and owns one block."""
    import mesh_whole_ref as WR
    import view_ref as V
    if isinstance(tiers, dict):
        tiers = tuple(tiers[k] for k in ("hash", "vba", "state", "flags", "store"))
    h2, v2 = WR.resolve(*tiers, maxW=WR.MAXW)
    o = V.oracle_for(O, cols, rows, tables=tables, n_blocks=len(v2) // 512, maxW=WR.MAXW)
    o.upload_hash(h2)
    o.upload_vba(v2, None)
    return o


def whole_point_classes(pts):
    """Per point the tier class of floor(pt)'s block and of the block of floor(pt) + 1 along each axis, from the scene:
    (class of the own block, set of neighbour classes) with view_whole_ref's numbering (-1: no entry)."""
    import view_whole_ref as VW
    t = VW.tiered_scene()
    h, c = t["hash"], t["cls"]
    held = np.flatnonzero(c >= 0)
    at = {(int(h["x"][k]), int(h["y"][k]), int(h["z"][k])): int(c[k]) for k in held}
    f = np.floor(np.asarray(pts, np.float32)).astype(np.int64)
    own = [at.get(tuple(v), -1) for v in (f >> 3).tolist()]
    nxt = [{at.get(tuple(v), -1) for v in (((f[j] + np.eye(3, dtype=np.int64)) >> 3).tolist())} for j in range(len(f))]
    return np.array(own), nxt


# ---- slices ------------------------------------------------------------------------------------------------------
SLICE_SIZES = ((4, 4), (37, 29), (164, 124))
SPHERE_C = np.array([3.375, -2.625, 140.25])          # pin_scenes.SPHERE_C16 / 16, voxels; radius 56.3


def slice_plane(kind, cols, rows, units="voxels"):
    """(origin, u, v) float32 of a plane through the sphere scene spanning about 120 voxels: "oblique" with steps
    that are no round numbers, "axis" the voxel plane z = 140.25 in exact steps.  In metres the three are scaled by
    voxelSize."""
    step = 120.0 / cols
    if kind == "oblique":
        u = np.float32(step) * np.array([0.83, 0.11, 0.31], np.float32)
        v = np.float32(step) * np.array([-0.07, 0.79, -0.43], np.float32)
    else:
        u = np.array([np.float32(step), 0, 0], np.float32)
        v = np.array([0, np.float32(step), 0], np.float32)
    o = (SPHERE_C - (cols / 2) * u.astype(np.float64) - (rows / 2) * v.astype(np.float64)).astype(np.float32)
    if units == "m":
        o, u, v = ((a * P.VOXEL_SIZE).astype(np.float32) for a in (o, u, v))
    return o, u.astype(np.float32), v.astype(np.float32)


def slice_points(o, u, v, cols, rows):
    """The header's pixel rule in numpy float32, row-major: (o + (float)x * u) + (float)y * v, each operation rounded."""
    x = np.arange(cols, dtype=np.float32)[None, :, None]
    y = np.arange(rows, dtype=np.float32)[:, None, None]
    xu = (x * u[None, None, :]).astype(np.float32)
    yv = (y * v[None, None, :]).astype(np.float32)
    return ((o[None, None, :] + xu).astype(np.float32) + yv).astype(np.float32).reshape(-1, 3)
