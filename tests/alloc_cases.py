"""Constructed inputs of tests/test_gpu_alloc_edges.py, and a plain restatement of AllocateSceneFromDepth to choose and
to check them with, in numpy alone.

The restatement (Ref) follows the reference's definition, not the kernels of topfusion_amd/csrc/tf_scene.hip:

  walk()      buildHashAllocAndVisibleTypePP (SceneReconstructionEngine.hpp:206-298) per pixel in raster order, float32,
              every operation rounded on its own in the reference's order, for world -> camera poses with the identity
              rotation and any translation (the matrix products are then exact, so contraction cannot matter).  One
              record per step: (pixel, step, block position, entry, request type 0 / 1 / 2, found class).
  Ref.alloc() setToType3, the walk's stores with the last writer's block coordinates, the serial allocation loop
              (SceneReconstructionEngine_host.cu:350-415) over the free lists and counters as they are, the visible
              list's compaction with its cap (:434-479, checkBlockVisibility for entries still of type 3, the enlarged
              frustum and the swap states under swapping) and the re-allocation of swapped-out entries (:417-432).

Cases are float32 `dists` images at 36x28 (3 x 2 tiles of 16 x 16 pixels: the last tile column 4 wide, the last tile
row 12 high) and 64x48 (whole tiles), on small tables.  dists are finite and block coordinates stay inside +-32000.
tests/test_alloc_cases.py asserts that Ref equals the oracle on every case and that each family reaches the edge it is
for; the GPU test compares the kernels with the oracle on the same calls."""
import functools

import numpy as np

from topfusion_amd import synth
from vbh_ref import (FOUND_BUCKET, FOUND_BUCKET_OUT, FOUND_CHAIN, FOUND_CHAIN_OUT, FOUND_NONE, HASH_DTYPE,  # noqa: F401
                     chain, empty_hash, hash_index, probe as lookup)      # (lookup: one step's probe, :264-296)

F = np.float32
WALK_DTYPE = np.dtype([("pixel", "<i4"), ("step", "<i4"), ("x", "<i2"), ("y", "<i2"), ("z", "<i2"), ("entry", "<i4"),
                       ("rtype", "u1"), ("found", "u1")])
VOXEL, BLOCK = 0.005, 0.04
TILE, AR_SLOTS, BATCH, CHUNK = 16, 256, 8, 4096               # tf_scene.hip: the request tile, its table, steps per batch
GRID_HALF = 128                                                # tf_grid_in: block coordinates in [-128, 128)
SIZES = ((36, 28), (64, 48))
SMALL = dict(n_buckets=256, n_excess=48, n_blocks=0x1000)
MID = dict(n_buckets=4096, n_excess=16, n_blocks=0x1000)
BIG = dict(n_buckets=0x8000, n_excess=0x2000, n_blocks=0x4000)
COLLIDE = dict(n_buckets=256, n_excess=4000 - 4000 % 16, n_blocks=0x2000)
STEP_MUS = {1: 0.0095, 2: 0.0195, 3: 0.0295, 8: 0.0795, 9: 0.0895, 16: 0.1595, 17: 0.1695}


def rt(t=(0, 0, 0)):
    """World -> camera pose with the identity rotation."""
    m = np.zeros((3, 4), F)
    m[:, :3], m[:, 3] = np.eye(3), t
    return m


def params_kw(W, H, **over):
    fx, fy, cx, cy = (float(v) for v in synth.intrinsics(W, H))
    kw = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=VOXEL, mu=0.02, viewFrustum_min=0.2,
              viewFrustum_max=3.0, vis_capacity=0x4000, max_render_blocks=0x4000, use_swapping=0, **BIG)
    kw.update(over)
    assert (kw["n_buckets"] + kw["n_excess"]) % 16 == 0
    return kw


def mu_accepted(mu, voxel=VOXEL):
    """tf_create's bound on steps per pixel (the 6-bit step field of the request key), in float32 as it states it."""
    return not (F(4.0) * F(mu) / (F(8.0) * F(voxel)) + F(2.0) > F(60.0))


@functools.lru_cache(None)
def mu_largest(voxel=VOXEL):
    """(the largest float32 mu tf_create accepts at this voxel size, the next float32 after it)."""
    lo, hi = F(0.5), F(0.7)
    assert mu_accepted(lo, voxel) and not mu_accepted(hi, voxel)
    while np.nextafter(lo, F(1)) != hi:
        mid = F((np.float64(lo) + np.float64(hi)) / 2)
        mid = mid if lo < mid < hi else np.nextafter(lo, F(1))
        if mu_accepted(mid, voxel):
            lo = mid
        else:
            hi = mid
    return float(lo), float(hi)


# ---- the per-pixel walk ------------------------------------------------------------------------------------------
def segments(kw, pose, dists):
    """Per pixel: (taken, first point, step vector, noSteps), SceneReconstructionEngine.hpp:218-262."""
    W, H = kw["cols"], kw["rows"]
    assert np.array_equal(pose[:, :3], np.eye(3, dtype=F)), "the restatement covers identity rotations only"
    tinv = -np.asarray(pose[:, 3], F)                          # Matrix4::inv of [I | t] (asserted in test_alloc_cases)
    d = np.ascontiguousarray(dists, F).reshape(H, W)
    mu, vmin, vmax = F(kw["mu"]), F(kw["viewFrustum_min"]), F(kw["viewFrustum_max"])
    taken = ~((d <= 0) | ((d - mu) < 0) | ((d - mu) < vmin) | ((d + mu) > vmax))
    invfx, invfy, cx, cy = F(1) / F(kw["fx"]), F(1) / F(kw["fy"]), F(kw["cx"]), F(kw["cy"])
    oovs = F(1) / (F(kw["voxelSize"]) * F(8))
    x, y = np.arange(W, dtype=F)[None, :], np.arange(H, dtype=F)[:, None]
    with np.errstate(all="ignore"):
        pc = [d * ((x - cx) * invfx), d * ((y - cy) * invfy), d]
        norm = np.sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2])
        s1, s2 = F(1) - mu / norm, F(1) + mu / norm
        point = [(pc[k] * s1 + tinv[k]) * oovs for k in range(3)]
        pe = [(pc[k] * s2 + tinv[k]) * oovs for k in range(3)]
        dr = [pe[k] - point[k] for k in range(3)]
        norm = np.sqrt(dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2])
        n = np.where(taken, np.ceil(F(2) * norm), 0).astype(np.int32)
        dv = (n - 1).astype(F)
        dr = [dr[k] / dv for k in range(3)]
    assert all(a.dtype == F for a in point + dr)
    return taken, point, dr, n


def step_blocks(kw, pose, dists):
    """(pixel, step, block position (k, 3) int16) of every step the walk takes, in raster order."""
    taken, point, dr, n = segments(kw, pose, dists)
    point = [p.reshape(-1).copy() for p in point]
    dr = [v.reshape(-1) for v in dr]
    n = n.reshape(-1)
    pix, step, blk = [], [], []
    with np.errstate(all="ignore"):
        for i in range(int(n.max(initial=0))):
            act = np.flatnonzero(i < n)
            b = np.stack([np.floor(point[k][act]) for k in range(3)], axis=1)
            assert np.abs(b).max() <= 32000
            pix.append(act); step.append(np.full(len(act), i)); blk.append(b.astype(np.int16))
            for k in range(3):
                point[k][act] = point[k][act] + dr[k][act]
    if not pix:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.int16)
    pix, step, blk = np.concatenate(pix), np.concatenate(step), np.concatenate(blk)
    order = np.lexsort((step, pix))
    return pix[order], step[order], blk[order]


def walk(kw, pose, dists, hash):
    pix, step, blk = step_blocks(kw, pose, dists)
    out = np.zeros(len(pix), WALK_DTYPE)
    out["pixel"], out["step"], out["x"], out["y"], out["z"] = pix, step, blk[:, 0], blk[:, 1], blk[:, 2]
    uniq, inv = np.unique(blk, axis=0, return_inverse=True)
    res = np.array([lookup(hash, kw["n_buckets"], b) for b in uniq], np.int64).reshape(-1, 3)
    out["entry"], out["rtype"], out["found"] = res[inv.reshape(-1)].T
    return out


# ---- block visibility (SceneReconstructionEngine.hpp:300-375), identity rotation ------------------------------------
def _block_visible(kw, pose, pos, enlarged):
    W, H = kw["cols"], kw["rows"]
    fx, fy, cx, cy = (F(kw[k]) for k in ("fx", "fy", "cx", "cy"))
    t = np.asarray(pose[:, 3], F)
    factor = F(8) * F(kw["voxelSize"])
    pt = [pos[:, k].astype(F) * factor for k in range(3)]
    if enlarged:
        lx, ux, ly, uy = F(-(W // 8)), F(W + W // 8), F(-(H // 8)), F(H + H // 8)    # (C's -W / 8 truncates)
    else:
        lx, ux, ly, uy = F(0), F(W), F(0), F(H)
    seen = np.zeros(len(pos), bool)

    def corner():
        with np.errstate(all="ignore"):
            b = [pt[k] + t[k] for k in range(3)]
            front = ~(b[2] < F(1e-10))
            u = fx * b[0] / b[2] + cx
            v = fy * b[1] / b[2] + cy
            seen[:] |= front & (u >= lx) & (u < ux) & (v >= ly) & (v < uy)

    corner()
    for moves in (((2, 1),), ((1, 1),), ((0, 1),), ((2, -1),), ((1, -1),), ((0, -1), (1, 1)), ((0, 1), (1, -1), (2, 1))):
        for k, sign in moves:
            pt[k] = pt[k] + factor if sign > 0 else pt[k] - factor
        corner()
    return seen


# ---- the whole call ------------------------------------------------------------------------------------------------
class Ref:
    """The scene and render state AllocateSceneFromDepth reads and writes, and the call itself."""

    def __init__(self, kw):
        self.kw = kw
        self.nb, self.n_total = kw["n_buckets"], kw["n_buckets"] + kw["n_excess"]
        self.hash = empty_hash(self.n_total)
        self.vis_type = np.zeros(self.n_total, np.uint8)
        self.visible_ids = np.zeros(kw["vis_capacity"], np.int32)
        self.alloc_list = np.arange(kw["n_blocks"], dtype=np.int32)
        self.excess_list = np.arange(kw["n_excess"], dtype=np.int32)
        self.v, self.e, self.n_vis = kw["n_blocks"] - 1, kw["n_excess"] - 1, 0
        self.swap_state = np.zeros(self.n_total, np.uint8)

    def counters(self):
        return self.v, self.e, self.n_vis

    def requests(self, pose, dists):
        """The walk and what it leaves in entriesAllocType / blockCoords: (walk, alloc type per entry, block
        coordinates per entry (last writer), index into the walk of each entry's last writer or -1)."""
        w = walk(self.kw, pose, dists, self.hash)
        alloc_type = np.zeros(self.n_total, np.uint8)
        coords = np.zeros((self.n_total, 3), np.int16)
        last = np.full(self.n_total, -1, np.int64)
        r = np.flatnonzero(w["rtype"] > 0)
        alloc_type[w["entry"][r]] = w["rtype"][r]
        last[w["entry"][r]] = r                                  # (ascending r: numpy keeps the last assignment)
        live = last >= 0
        for k, f in enumerate("xyz"):
            coords[live, k] = w[f][last[live]]
        return w, alloc_type, coords, last

    def alloc(self, pose, dists, only_update=False, reset_visible=False):
        kw, nb = self.kw, self.nb
        if reset_visible:
            self.n_vis = 0
        off_list = self.vis_type == 3
        off_list[self.visible_ids[:self.n_vis]] = False            # type 3 from an earlier call, no longer on the list
        self.vis_type[self.visible_ids[:self.n_vis]] = 3                                   # setToType3
        w, alloc_type, coords, last = self.requests(pose, dists)
        out = w["found"] >= FOUND_BUCKET_OUT
        f = np.flatnonzero(w["rtype"] == 0)
        self.vis_type[w["entry"][f]] = np.where(out[f], 2, 1)
        self.vis_type[w["entry"][w["rtype"] == 1]] = 1
        fail, per_entry = [0, 0], {}
        if not only_update:                                                                # :350-415, serial
            v, e = self.v, self.e
            for t in np.flatnonzero(alloc_type):
                if alloc_type[t] == 1:
                    vba = v; v -= 1
                    if vba >= 0:
                        self.hash[t] = (*coords[t], 0, 0, self.alloc_list[vba])
                    else:
                        self.vis_type[t] = 0
                        v += 1; fail[0] += 1
                    per_entry[int(t)] = vba >= 0
                else:
                    vba = v; v -= 1
                    exl = e; e -= 1
                    if vba >= 0 and exl >= 0:
                        off = int(self.excess_list[exl])
                        self.hash["offset"][t] = off + 1
                        self.hash[nb + off] = (*coords[t], 0, 0, self.alloc_list[vba])
                        self.vis_type[nb + off] = 1
                    else:
                        v += 1; e += 1; fail[1] += 1
                    per_entry[int(t)] = vba >= 0 and exl >= 0
            self.v, self.e = v, e
        swapping = bool(kw["use_swapping"]) and not only_update
        t3 = np.flatnonzero(self.vis_type == 3)                                            # :434-479
        if len(t3):
            pos = np.stack([self.hash[f][t3] for f in "xyz"], axis=1)
            self.vis_type[t3[~_block_visible(kw, pose, pos, swapping)]] = 0
        listed = np.flatnonzero(self.vis_type > 0)
        if swapping:
            self.swap_state[listed[self.swap_state[listed] != 2]] = 1
        cap = kw["vis_capacity"]
        self.visible_ids[:min(len(listed), cap)] = listed[:cap]
        self.n_vis = min(len(listed), cap)
        realloc = [0, 0]
        if swapping:                                                                       # :417-432, ascending
            for t in listed[self.hash["ptr"][listed] == -1]:
                vba = self.v; self.v -= 1
                if vba >= 0:
                    self.hash["ptr"][t] = self.alloc_list[vba]; realloc[0] += 1
                else:
                    self.v += 1; realloc[1] += 1
        return dict(walk=w, alloc_type=alloc_type, coords=coords, last=last, fail=tuple(fail), ok=per_entry,
                    n1=int((alloc_type == 1).sum()), n2=int((alloc_type == 2).sum()), need=len(listed),
                    realloc=tuple(realloc), vis_type=self.vis_type.copy(), listed=listed, counters=self.counters(),
                    off_list_dropped=int((off_list & (self.vis_type == 0)).sum()))


# ---- what the families are asserted to reach -------------------------------------------------------------------------
def tile_of(kw, pixel):
    W = kw["cols"]
    return (pixel // W) // TILE * ((W + TILE - 1) // TILE) + (pixel % W) // TILE


def n_tiles(kw):
    return ((kw["cols"] + TILE - 1) // TILE) * ((kw["rows"] + TILE - 1) // TILE)


def tile_distinct(kw, w, what="requests"):
    """Per tile, the number of distinct entries its pixels request (what the tile's table aggregates) or find."""
    sel = w[w["rtype"] > 0] if what == "requests" else w[w["rtype"] == 0]
    tiles = tile_of(kw, sel["pixel"])
    return np.array([len(np.unique(sel["entry"][tiles == t])) for t in range(n_tiles(kw))])


def tile_entries(kw, w, tile):
    sel = w[(w["rtype"] > 0) & (tile_of(kw, w["pixel"]) == tile)]
    return np.unique(sel["entry"])


# ---- images ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def noisy(W, H, lo=0.5, hi=2.5, seed=11):
    return np.random.default_rng(seed).uniform(lo, hi, (H, W)).astype(F)


def tile_mask(kw, tile):
    W, H = kw["cols"], kw["rows"]
    pix = np.arange(W * H)
    return (tile_of(kw, pix) == tile).reshape(H, W)


def slots_image(kw, tile, target, base=None, at_least=False):
    """Pixels of one tile of the noisy image enabled in raster order until the tile requests `target` distinct
    entries of an empty table (exactly, or at least); every other pixel 0."""
    W, H = kw["cols"], kw["rows"]
    src = noisy(W, H)
    h = empty_hash(kw["n_buckets"] + kw["n_excess"])
    full = np.where(tile_mask(kw, tile), src, 0).astype(F)
    w = walk(kw, rt(), full, h)
    w = w[w["rtype"] > 0]
    pixels = np.unique(w["pixel"])
    ents = {int(p): set(w["entry"][w["pixel"] == p].tolist()) for p in pixels}
    for start in range(len(pixels)):                       # (a raster order from another start when one falls short)
        out = np.zeros((H, W), F) if base is None else base.copy()
        seen = set()
        for p in np.roll(pixels, -start):
            if not at_least and len(seen | ents[int(p)]) > target:
                continue
            seen |= ents[int(p)]
            out[p // W, p % W] = src[p // W, p % W]
            if len(seen) == target and not at_least:
                break
        if len(seen) == target or (at_least and len(seen) >= target):
            return out
    raise AssertionError((len(seen), target))


def steps_image(W, H, mu):
    """Depths that every accepted mu keeps inside the frustum, a quarter of the pixels dropped."""
    lo, hi = 0.2 + mu + 0.01, 3.0 - mu - 0.01
    d = np.random.default_rng(5).uniform(lo, hi, (H, W)).astype(F)
    d[::2, ::2] = 0
    if mu > 0.3:
        d[1::2, :] = 0                                          # (fewer requests than the contexts have blocks)
    return d


GRID_OFFSET = (0.3, 0.25, 1.0)                 # where, in camera coordinates, the boundary plane of each axis lies


def grid_pose(axis, side):
    """A translation that puts block coordinate -129 | -128 (side 0) or 127 | 128 (side 1) of `axis` on the plane
    x = 0.3, y = 0.25 or z = 1 of the camera, which the segments of a wall 1 m ahead cross (inv(pose) adds -t)."""
    t = np.zeros(3)
    edge = (-GRID_HALF if side == 0 else GRID_HALF) * BLOCK
    t[axis] = GRID_OFFSET[axis] - edge
    return rt(t)


def grid_image(W, H):
    d = np.random.default_rng(3).uniform(0.9, 1.1, (H, W)).astype(F)
    return d


def skip_values(kw):
    """(value, taken) for both sides of every rejection test of :213-216, for this context's mu and frustum."""
    mu, vmin, vmax = F(kw["mu"]), F(kw["viewFrustum_min"]), F(kw["viewFrustum_max"])
    up, down = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    out = [(F(0), False), (F(-1), False), (down(mu), False)]
    lo = F(vmin + mu)
    while F(lo - mu) < vmin:
        lo = up(lo)
    while F(down(lo) - mu) >= vmin:
        lo = down(lo)
    out += [(lo, True), (down(lo), False)]                      # d - mu == viewFrustum_min exactly | one step below
    assert F(lo - mu) == vmin, "choose parameters for which d - mu == viewFrustum_min is representable"
    hi = F(vmax - mu)
    while F(hi + mu) > vmax:
        hi = down(hi)
    while F(up(hi) + mu) <= vmax:
        hi = up(hi)
    assert F(hi + mu) == vmax
    out += [(hi, True), (up(hi), False), (F(1.0), True)]
    return out


def skip_image(kw):
    W, H = kw["cols"], kw["rows"]
    vals = skip_values(kw)
    d = np.zeros((H, W), F)
    flat = d.reshape(-1)
    for i in range(W * H):
        flat[i] = vals[i % len(vals)][0]
    return d, np.array([vals[i % len(vals)][1] for i in range(W * H)]).reshape(H, W)


def permutation(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.int32)


@functools.lru_cache(None)
def _filler_pool(nb):
    """Block positions far from every case's (y <= -20000, z = 25000), by bucket."""
    x, y = np.meshgrid(np.arange(0, 30000, 7), np.arange(-20000, -20256, -1))
    x, y = x.reshape(-1), y.reshape(-1)
    pool = {}
    for b, xx, yy in zip(hash_index(x, y, 25000, nb).tolist(), x.tolist(), y.tolist()):
        pool.setdefault(b, []).append((xx, yy, 25000))
    return pool


def chain_table(kw, blocks_by_class):
    """A table holding the given blocks: "bucket" in their buckets, "chain" at the end of chains of filler entries at
    least 8 long, "out" as "bucket" with ptr == -1; the bucket of the "last" block gets a chain that ends at the table's
    last entry without holding the block, which is then requested there.  Returns
    (hash, alloc_list, excess_list, (lastFreeBlockId, lastFreeExcessListId), entries by class)."""
    nb, ne, nblk = kw["n_buckets"], kw["n_excess"], kw["n_blocks"]
    h = empty_hash(nb + ne)
    ptr, used_ex, where = 0, [], {k: [] for k in blocks_by_class}

    def put(idx, b, p):
        h[idx] = (b[0], b[1], b[2], 0, 0, p)

    def new_ptr():                                               # as a fresh scene hands them out: from the top
        nonlocal ptr
        ptr += 1
        return nblk - ptr

    next_free = [0]

    def free_excess(want=None):
        if want is None:
            while next_free[0] in used_ex:
                next_free[0] += 1
            want = next_free[0]
        assert want not in used_ex and want < ne
        used_ex.append(want)
        return want

    pool = _filler_pool(nb)

    taken = {}

    def find_filler(bucket):
        taken[bucket] = taken.get(bucket, 0) + 1
        return pool[bucket][taken[bucket] - 1]

    def append(b, p, depth=0, last=False):
        bucket = hash_index(*b, nb)
        if h["ptr"][bucket] < -1:
            put(bucket, find_filler(bucket), new_ptr())
        links = list(chain(h, nb, b))
        end, n = links[-1], len(links)
        while n < depth:
            off = free_excess()
            put(nb + off, find_filler(bucket), new_ptr())
            h["offset"][end] = off + 1
            end, n = nb + off, n + 1
        off = free_excess(ne - 1 if last else None)
        put(nb + off, b, p)
        h["offset"][end] = off + 1
        return nb + off

    for cls in ("bucket", "alias"):
        for b in blocks_by_class.get(cls, []):
            bucket = hash_index(*b, nb)
            if h["ptr"][bucket] < -1:
                put(bucket, b, new_ptr())
                where[cls].append(bucket)
    for b in blocks_by_class.get("out", []):
        bucket = hash_index(*b, nb)
        if h["ptr"][bucket] < -1:
            put(bucket, b, -1)
            where["out"].append(bucket)
    for b in blocks_by_class.get("chain", []):
        if len(used_ex) + 9 >= ne - 1:
            break
        where["chain"].append(append(b, new_ptr(), depth=8))
    for b in blocks_by_class.get("last", [])[:1]:                # (after every other chain: this one must end there)
        where["last"].append(append(find_filler(hash_index(*b, nb)), new_ptr(), last=True))
    assert ptr <= nblk
    # the free lists as a scene that allocated these leaves them: the identity block stack taken from the top, the
    # excess offsets in use at the end of their list
    alloc_list = np.arange(nblk, dtype=np.int32)
    rest = [o for o in range(ne) if o not in used_ex]
    excess_list = np.array(rest + used_ex[::-1], np.int32)
    return h, alloc_list, excess_list, (nblk - ptr - 1, len(rest) - 1), where


# ---- states and cases ------------------------------------------------------------------------------------------------
def snapshot(r):
    return dict(hash=r.hash.copy(), vis_type=r.vis_type.copy(), visible_ids=r.visible_ids.copy(),
                alloc_list=r.alloc_list.copy(), excess_list=r.excess_list.copy(), counters=r.counters(),
                swap_state=r.swap_state.copy())


def load(r, s):
    r.hash, r.vis_type, r.visible_ids = s["hash"].copy(), s["vis_type"].copy(), s["visible_ids"].copy()
    r.alloc_list, r.excess_list, r.swap_state = s["alloc_list"].copy(), s["excess_list"].copy(), s["swap_state"].copy()
    r.v, r.e, r.n_vis = s["counters"]
    return r


def fresh(kw):
    return snapshot(Ref(kw))


def after(kw, state, calls):
    """The state `calls` leave, and their infos."""
    r = load(Ref(kw), state)
    infos = [r.alloc(*c) for c in calls]
    return snapshot(r), infos


TILTED = np.zeros((3, 4), F)
TILTED[:, :3] = (np.array([[1, 0, 0], [0, np.cos(0.21), -np.sin(0.21)], [0, np.sin(0.21), np.cos(0.21)]])
                 @ synth._rot_y(-0.33))
TILTED[:, 3] = (0.013, -0.021, 0.017)


class Case:
    """One context's parameters, the state loaded into it, and the calls (pose, dists, onlyUpdateVisibleList,
    resetVisibleList) made on it one after the other.  ref: the restatement covers it (identity rotations)."""

    def __init__(self, name, kw, calls, state=None, env=None, ref=True):
        self.name, self.kw, self.calls, self.env, self.ref = name, kw, calls, env or {}, ref
        self.state = fresh(kw) if state is None else state

    def infos(self):
        assert self.ref
        if not hasattr(self, "_infos"):
            self._infos = after(self.kw, self.state, self.calls)[1]
        return self._infos

    def variant(self, suffix, calls, ref=True):
        return Case(self.name + suffix, self.kw, calls, self.state, self.env, ref)


def call(dists, pose=None, only=False, reset=False):
    return (rt() if pose is None else pose, dists, only, reset)


def until_quiet(kw, state, first, img, cap):
    """`first` and then `img` again and again until a call requests nothing (that call included)."""
    calls = list(first)
    for _ in range(cap):
        infos = after(kw, state, calls)[1]
        if calls and infos[-1]["n1"] + infos[-1]["n2"] == 0:
            return calls
        calls.append(call(img))
    raise AssertionError("requests never stop within the cap")


def variants(c):
    """The first case of a family once more with onlyUpdateVisibleList (then a normal call), with resetVisibleList
    (after a normal call and one on an empty image, which leaves the whole list at type 3; from a shifted pose), and
    under a rotated pose (against the oracle alone)."""
    pose, d = c.calls[0][0], c.calls[0][1]
    shifted = pose.copy()
    shifted[:, 3] += F([0.45, -0.07, 0.05])
    return [c.variant("+only", [call(d, pose, only=True), call(d, pose)]),
            c.variant("+reset", [call(d, pose), call(np.zeros_like(d), pose), call(d, shifted, reset=True), call(d, pose)]),
            c.variant("+rotated", [call(d, TILTED), call(d, TILTED)], ref=False)]


SLOT_MU = 0.0295                               # three steps per pixel: up to 768 blocks per tile
SHARED = dict(n_buckets=4096, n_excess=16, n_blocks=0x1000)
TYPE2 = dict(n_buckets=512, n_excess=1536, n_blocks=0x2000)


@functools.lru_cache(None)
def slots():
    out = []
    kw = params_kw(36, 28, mu=SLOT_MU)
    full = noisy(36, 28)
    for target in (255, 256, 257, 600):
        img = slots_image(kw, 0, target, at_least=target == 600)
        out.append(Case(f"slots_{target}", kw, until_quiet(kw, fresh(kw), [call(img), call(img)], full, 6)))
    kw64 = params_kw(64, 48, mu=STEP_MUS[8])              # (eight steps: an inner tile of whole 16 x 16 pixels)
    img = slots_image(kw64, 5, 600, at_least=True)
    out.append(Case("slots_600_64x48", kw64, until_quiet(kw64, fresh(kw64), [], img, 8)))
    kws = params_kw(36, 28, mu=STEP_MUS[8], **SHARED)
    img = slots_image(kws, 1, 255, base=slots_image(kws, 0, 600, at_least=True))
    out.append(Case("slots_shared", kws, [call(img), call(img), call(img)]))
    kw2 = params_kw(36, 28, mu=SLOT_MU, **TYPE2)
    occupied = after(kw2, fresh(kw2), [call(full)] * 3)[0]
    other = noisy(36, 28, seed=12)
    out.append(Case("slots_type2", kw2, [call(other), call(other)], occupied))
    return out + variants(out[3])


def steps_top():
    return mu_largest()[0]


@functools.lru_cache(None)
def steps():
    out = []
    for n, mu in list(STEP_MUS.items()) + [("top", steps_top())]:
        kw = params_kw(36, 28, mu=mu)
        img = steps_image(36, 28, mu)
        out.append(Case(f"steps_{n}", kw, [call(img), call(img)]))
    kw = params_kw(64, 48, mu=steps_top())
    out.append(Case("steps_top_64x48", kw, [call(steps_image(64, 48, steps_top()))]))
    kw = params_kw(36, 28, mu=STEP_MUS[17], **COLLIDE)
    img = steps_image(36, 28, STEP_MUS[17])
    out.append(Case("steps_17_256", kw, [call(img)] * 3))
    return out + variants(out[6])


COLLIDE_CAP = 60


@functools.lru_cache(None)
def collide():
    kw = params_kw(36, 28, **COLLIDE)
    c = Case("collide", kw, until_quiet(kw, fresh(kw), [], noisy(36, 28), COLLIDE_CAP))
    short = Case("collide_3", kw, c.calls[:3])
    return [c] + variants(short)


GRID_MU = STEP_MUS[17]
GRID_CLASSES = ("bucket", "chain", "out", "request")


def grid_state(kw, pose, img, axis, side):
    """A table that holds, on each side of the boundary, some of the walked blocks in their buckets, some deep in
    chains, some swapped out, and leaves the rest to be requested."""
    w = walk(kw, pose, img, empty_hash(kw["n_buckets"] + kw["n_excess"]))
    blocks = np.unique(np.stack([w["x"], w["y"], w["z"]], axis=1), axis=0)
    edge = -GRID_HALF if side == 0 else GRID_HALF
    by = {k: [] for k in GRID_CLASSES}
    for inside in (False, True):
        sel = blocks[(blocks[:, axis] >= edge) == inside]
        for i, b in enumerate(sel):
            by[GRID_CLASSES[i % 4]].append(tuple(int(v) for v in b))
    by["chain"] = by["chain"][::max(1, len(by["chain"]) // 200)]
    if side == 1:
        # the cells a grid index formed from coordinate 128 would fall on (the carry into the next axis; the wrap to
        # -128 on the last one) hold blocks of their own, far from every segment
        at = blocks[blocks[:, axis] == GRID_HALF].astype(np.int64)
        at[:, axis] = -GRID_HALF
        if axis < 2:
            at[:, axis + 1] += 1
        by["alias"] = [tuple(int(v) for v in b) for b in at]
    by["last"] = [by["request"].pop()]
    h, alloc_list, excess_list, (v, e), where = chain_table(kw, by)
    s = fresh(kw)
    s.update(hash=h, alloc_list=alloc_list, excess_list=excess_list, counters=(v, e, 0))
    s["alias"] = where.get("alias", [])
    return s


def grid_side(c, axis, side):
    """Per walked step of the case's first call: on the far side of the boundary (outside the block grid)?"""
    w = c.infos()[0]["walk"]
    edge = -GRID_HALF if side == 0 else GRID_HALF
    return (w["xyz"[axis]] < edge) if side == 0 else (w["xyz"[axis]] >= edge)


@functools.lru_cache(None)
def grid():
    out = []
    for W, H, axes in ((36, 28, (0, 1, 2)), (64, 48, (0,))):
        kw = params_kw(W, H, mu=GRID_MU)
        img = grid_image(W, H)
        for axis in axes:
            for side in (0, 1):
                pose = grid_pose(axis, side)
                c = Case(f"grid_{W}x{H}_{'xyz'[axis]}{'-+'[side]}", kw, [call(img, pose), call(img, pose)],
                         grid_state(kw, pose, img, axis, side))
                c.axis, c.side = axis, side
                out.append(c)
    return out + variants(out[0])


SKIP_ALT = dict(mu=0.25, viewFrustum_min=0.25, viewFrustum_max=2.0)


@functools.lru_cache(None)
def skip():
    out = []
    for name, over in (("skip", {}), ("skip_alt", SKIP_ALT)):
        kw = params_kw(36, 28, **over)
        img, taken = skip_image(kw)
        c = Case(name, kw, [call(img), call(img)])
        c.taken = taken
        out.append(c)
    return out + variants(out[0])


APPLY_TABLES = {"256+48": (36, 28, SMALL), "4096+16": (36, 28, MID), "0x8000+0x2000": (64, 48, BIG)}


def apply_pairs(n1, n2, v_free, e_free):
    """(name, v0, e0) of the sweep; `plenty` is what the base state really has free."""
    n = n1 + n2
    out = [(f"v0={name}", v, e_free) for name, v in (("-1", -1), ("0", 0), ("n-2", n - 2), ("n-1", n - 1), ("n", n))]
    out += [(f"e0={name}", v_free, e) for name, e in (("-1", -1), ("0", 0), ("n2-2", n2 - 2), ("n2-1", n2 - 1),
                                                       ("n2", n2)) if e <= e_free]
    out += [("excess_first", v_free, min(n2 // 2, e_free) - 1), ("blocks_first", n // 2, min(n2, e_free))]
    return [(a, v, e) for a, v, e in out if -1 <= v <= v_free and -1 <= e <= e_free]


@functools.lru_cache(None)
def apply():
    """Frame 1 (on an empty table: buckets only) gives the base state; the sweep runs frame 2, another image, whose
    requests are of both types, from counters set below what is free and over permuted free lists."""
    out = []
    for tname, (W, H, table) in APPLY_TABLES.items():
        kw = params_kw(W, H, mu=SLOT_MU, **table)
        first, second = noisy(W, H).copy(), noisy(W, H, seed=12)
        if table is SMALL:
            first.reshape(-1)[np.arange(W * H) % 16 != 0] = 0   # (about half of the 256 buckets taken)
        base = after(kw, fresh(kw), [call(first)])[0]
        v_free, e_free, _ = base["counters"]
        base["alloc_list"][:v_free + 1] = base["alloc_list"][:v_free + 1][permutation(v_free + 1, 21)]
        base["excess_list"][:e_free + 1] = base["excess_list"][:e_free + 1][permutation(e_free + 1, 22)]
        probe = after(kw, base, [call(second)])[1][0]
        for name, v0, e0 in apply_pairs(probe["n1"], probe["n2"], v_free, e_free):
            s = dict(base, counters=(v0, e0, base["counters"][2]))
            c = Case(f"apply_{tname}_{name}", kw, [call(second), call(second)], s)
            c.table, c.pair, c.n1, c.n2, c.v0, c.e0, c.plenty = tname, name, probe["n1"], probe["n2"], v0, e0, (v_free, e_free)
            out.append(c)
    # the identity lists: the first type-2 success takes the table's last entry, and a later frame requests there
    kw = params_kw(36, 28, mu=SLOT_MU, **SMALL)
    out.append(Case("apply_last_entry", kw, [call(noisy(36, 28)), call(noisy(36, 28, seed=12)), call(noisy(36, 28, seed=13))]))
    return out + variants(out[0])


def chunk_counts(c, k=0):
    """Requests per chunk of CHUNK entries in the case's call k."""
    t = c.infos()[k]["alloc_type"]
    n_chunks = -(-len(t) // CHUNK)
    return np.array([(t[i * CHUNK:(i + 1) * CHUNK] > 0).sum() for i in range(n_chunks)])


VIS_NEED = 4097
VIS_SHIFT, VIS_SHIFT2 = (0.3, 0.0, 0.0), (0.6, 0.0, 0.0)


@functools.lru_cache(None)
def vis_image():
    """Pixels of the noisy 64x48 image in raster order until an empty table lists exactly VIS_NEED entries."""
    kw = params_kw(64, 48, mu=SLOT_MU)
    src = noisy(64, 48)
    w = walk(kw, rt(), src, empty_hash(kw["n_buckets"] + kw["n_excess"]))
    assert (w["rtype"] == 1).all()
    out, seen = np.zeros_like(src), set()
    for p in range(64 * 48):
        ents = set(w["entry"][w["pixel"] == p].tolist())
        if len(seen | ents) > VIS_NEED:
            continue
        seen |= ents
        out[p // 64, p % 64] = src[p // 64, p % 64]
        if len(seen) == VIS_NEED:
            return out
    raise AssertionError(len(seen))


@functools.lru_cache(None)
def vis():
    out = []
    img = vis_image()
    for cap in (VIS_NEED - 2, VIS_NEED - 1, VIS_NEED, VIS_NEED + 1, 1):
        for fused in ("1", "0"):
            kw = params_kw(64, 48, mu=SLOT_MU, vis_capacity=cap)
            c = Case(f"vis_cap{cap}_fused{fused}", kw, [call(img), call(img, rt(VIS_SHIFT)), call(img, rt(VIS_SHIFT2))],
                     env={"TFUSION_VIS_FUSED": fused})
            c.cap = cap
            out.append(c)
    return out + variants(out[2])


SWAP = dict(use_swapping=1, swap_transfer_blocks=0x1000)


def _halfway(kw, state, first):
    """The state with lastFreeBlockId set so that the blocks run out halfway through the re-allocations of the
    first call, after its ordinary requests have taken theirs."""
    info = after(kw, state, [first])[1][0]
    assert info["fail"][0] == 0 and info["realloc"][1] == 0       # (type-2 requests may lack excess entries)
    served = info["n1"] + info["n2"] - info["fail"][1]
    v0 = served + info["realloc"][0] // 2 - 1
    assert v0 <= state["counters"][0]
    return dict(state, counters=(v0,) + tuple(state["counters"][1:]))


@functools.lru_cache(None)
def swapping():
    out = []
    kw = params_kw(36, 28, mu=GRID_MU, **SWAP)
    img = grid_image(36, 28)
    for axis, side in ((2, 0), (0, 1)):
        pose = grid_pose(axis, side)
        shifted = pose.copy()
        shifted[:, 3] += F([0.4, 0.0, 0.0])
        s = _halfway(kw, grid_state(kw, pose, img, axis, side), call(img, pose))
        out.append(Case(f"swapping_grid_{'xyz'[axis]}{'-+'[side]}", kw, [call(img, pose), call(img, pose), call(img, shifted)], s))
    kw = params_kw(36, 28, mu=SLOT_MU, **dict(MID, **SWAP))
    first, second = noisy(36, 28), noisy(36, 28, seed=12)
    base = after(kw, fresh(kw), [call(first)])[0]
    live = np.flatnonzero(base["hash"]["ptr"] >= 0)
    base["hash"]["ptr"][live[::3]] = -1                          # swapped out (their blocks stay out of the free list)
    base["alloc_list"][:base["counters"][0] + 1] = base["alloc_list"][:base["counters"][0] + 1][permutation(base["counters"][0] + 1, 23)]
    out.append(Case("swapping_apply_4096+16", kw, [call(second), call(second), call(first, rt(VIS_SHIFT))],
                    _halfway(kw, base, call(second))))
    return out + [out[0].variant("+only", [call(img, grid_pose(2, 0), only=True), call(img, grid_pose(2, 0))]),
                  out[0].variant("+rotated", [call(img, TILTED), call(img, TILTED)], ref=False)]


FAMILIES = dict(slots=slots, steps=steps, collide=collide, grid=grid, skip=skip, apply=apply, vis=vis, swapping=swapping)


def all_cases():
    return [c for f in FAMILIES.values() for c in f()]


def case_ids():
    return [c.name for c in all_cases()]
