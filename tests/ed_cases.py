"""Constructed inputs of tests/test_gpu_ed_edges.py: visible lists that put CreateExpectedDepths' boxes on the index
edges of its binning and fill (topfusion_amd/csrc/tf_ed.h, ed_fill_block / ed_tile_range in tf_render.hip), built on
the CPU with numpy alone.

A scene is one hash table for one image size: plain block positions in distinct buckets of an empty table (no excess
chain), ptr = 0, 1, 2, ... in ascending entry order, and per pose a few families of entries:

  far       blocks on a plane 2 m ahead that tile the /8 region and one cell past it, plus blocks half and wholly
            outside each of the four image borders (boxes are clamped to the full-resolution W-1 / H-1)
  near      blocks 0.04-0.25 m ahead: boxes over many rows, past the /8 columns, in the LDS rows under the /8 rows,
            and reaching below the LDS rows (segments small enough for one thread, and larger ones that are queued)
  straddle  blocks around the camera plane: 1..7 corners behind it, all 8 behind it, every front corner nearer than
            VERY_CLOSE, zmin raised to VERY_CLOSE, and two listed entries without a block (ptr -1 and -2)
  wide      more than ED_QUEUE boxes wider than ED_WIDE columns over one common /8 row, plus boxes exactly ED_WIDE and
            ED_WIDE + 1 columns wide in that row

and the lists derived from them: far + near cut or repeated to the counts of COUNTS, and the boxes of far + near +
wide with the caps of cap_points().  Every list is used in the three orders of ORDERS.

The geometry is worked out in float64 (project64) only to choose blocks; what a family really contains is asserted
against the oracle's float32 projection in tests/test_ed_cases.py, so an edit here cannot hollow a GPU test out.

Three things the reference's arithmetic rules out, whatever the input:
  * ProjectSingleBlock starts a box's upper left at (W/8, H/8), so uly <= H/8 < nrows for every box: no box lies
    wholly below the LDS rows (none is in a below bin only), and a block wholly outside the right or the bottom border
    is not rejected but becomes a box from the /8 region's edge to W-1 / H-1 -- the widest and tallest boxes there are.
    Only blocks wholly outside the left or the top border end with ulx > lrx / uly > lry;
  * a corner at camera z in [0, 1e-3) is excluded (INPUT CONDITION below), and with the identity pose every corner's z
    is a multiple of the block size, so a block there has 0 or 8 corners behind the plane (4 would sit on z = 0):
    the 1..7 kinds exist under the tilted pose only;
  * ProjectSingleBlock starts zmax at VERY_CLOSE, so its `zmax < VERY_CLOSE` rejection never fires: a block whose
    front corners are all nearer than VERY_CLOSE is kept with zmin = zmax = VERY_CLOSE ("all_close").

INPUT CONDITION (admissible): every corner's camera z is below 0 or at least 1e-3, and every projected /8
coordinate of a front corner is below 2^30 in magnitude -- past 2^31 the float -> int conversion is undefined and a
host and a GPU may differ."""
import functools

import numpy as np

from topfusion_amd import synth
from vbh_ref import HASH_DTYPE, empty_hash, hash_index  # noqa: F401

VOXEL, BLOCK = 0.005, 0.04
SUB, RB = 8, 16                               # minmaximg_subsample, renderingBlockSize
FAR_AWAY, VERY_CLOSE = np.float32(999999.9), np.float32(0.05)
ED_XROWS, ED_WIDE, ED_QUEUE, ED_CHUNK = 8, 4, 256, 256        # tf_internal.h, tf_render.hip, tf_ed.h
BELOW_BY_THREAD = 64                          # a below segment of at most this many pixels is filled by its thread
TABLES = dict(voxelSize=VOXEL, n_buckets=0x20000, n_excess=0x100, n_blocks=0x1000, vis_capacity=0x1000)
N_TOTAL = TABLES["n_buckets"] + TABLES["n_excess"]
BIG_SIZES, SMALL_SIZES = ((64, 48), (36, 28)), ((12, 8), (4, 4))
ORDERS = ("ascending", "reversed", "shuffled")
COUNTS = (0, 1, 255, 256, 257, 511, 512, 513)
LDS_MAX_N = 512                               # the TFUSION_ED_LDS_MAX_N the count edges are made for
WIDE_BOXES = 300
CAP_NAMES = ("total_eq_cap", "total_eq_cap_plus_1", "first_drop_255", "first_drop_256", "first_drop_last", "exact_fit",
             "multi_then_single")

_CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.float64)


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def _rt(R, t):
    m = np.zeros((3, 4), np.float32)
    m[:, :3], m[:, 3] = R, t
    return m


# world -> camera
POSES = {"identity": _rt(np.eye(3), np.zeros(3)),
         "tilted": _rt(_rot_x(0.21) @ synth._rot_y(-0.33), (0.013, -0.021, 0.017))}


def intr_of(W, H):
    return np.array(synth.intrinsics(W, H), np.float32)


def region(W, H):
    """(rc, rr, nrows): the /8 region's columns and rows, and the fill's LDS rows (ed_nrows)."""
    rc, rr = (W - 1) // SUB + 1, (H - 1) // SUB + 1
    return rc, rr, min(rr + ED_XROWS, H)


def params_kw(W, H, intr=None, **over):
    fx, fy, cx, cy = (float(v) for v in (intr_of(W, H) if intr is None else intr))
    kw = dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, **TABLES)
    kw.update(over)
    return kw


def project64(blocks, pose, W, H, intr=None):
    """ProjectSingleBlock in float64 over block positions (n, 3): dict of valid, box (n, 4: ulx, uly, lrx, lry), z
    (n, 2: as stored), zfront (n, 2: the front corners' own min / max, nan without one), nbehind, admissible, need
    (rendering tiles)."""
    fx, fy, cx, cy = (float(v) for v in (intr_of(W, H) if intr is None else intr))
    b = np.asarray(blocks, np.float64).reshape(-1, 3)
    pose = np.asarray(pose, np.float64)
    pw = (b[:, None, :] + _CORNERS[None]) * BLOCK
    q = pw @ pose[:, :3].T + pose[:, 3]
    z = q[..., 2]
    front = z >= 1e-6
    zs = np.where(front, z, 1.0)
    px = (fx * q[..., 0] / zs + cx) / SUB
    py = (fy * q[..., 1] / zs + cy) / SUB
    big = 2.0 ** 30

    def lo(p, init):
        return np.minimum(init, np.where(front, np.floor(p), big).min(axis=1))

    def hi(p):
        return np.maximum(-1, np.where(front, np.ceil(p), -big).max(axis=1))

    ulx, uly, lrx, lry = lo(px, W // SUB), lo(py, H // SUB), hi(px), hi(py)
    admissible = (((z < 0) | (z >= 1e-3)).all(axis=1)
                  & (np.where(front, np.maximum(np.abs(px), np.abs(py)), 0.0).max(axis=1) < big))
    ulx, uly = np.maximum(ulx, 0), np.maximum(uly, 0)
    lrx, lry = np.minimum(lrx, W - 1), np.minimum(lry, H - 1)
    valid = ~((ulx > lrx) | (uly > lry))
    any_front = front.any(axis=1)
    zf_min = np.where(any_front, np.where(front, z, np.inf).min(axis=1), np.nan)
    zf_max = np.where(any_front, np.where(front, z, -np.inf).max(axis=1), np.nan)
    box = np.stack([ulx, uly, lrx, lry], axis=1).astype(np.int64)
    zmin = np.maximum(np.where(any_front, zf_min, float(FAR_AWAY)), float(VERY_CLOSE))
    zmax = np.maximum(np.where(any_front, zf_max, 0.0), float(VERY_CLOSE))
    need = np.where(valid, -(-(box[:, 2] - box[:, 0] + 1) // RB) * -(-(box[:, 3] - box[:, 1] + 1) // RB), 0)
    return dict(valid=valid, box=box, z=np.stack([zmin, zmax], axis=1), zfront=np.stack([zf_min, zf_max], axis=1),
                nbehind=(~front).sum(axis=1), admissible=admissible, need=need)


def block_at(pose, intr, u8, v8, z):
    """The block that holds the world point projecting to /8 coordinates (u8, v8) at camera depth z."""
    fx, fy, cx, cy = (float(v) for v in intr)
    pose = np.asarray(pose, np.float64)
    pc = np.array([(u8 * SUB - cx) / fx * z, (v8 * SUB - cy) / fy * z, z])
    pw = pose[:, :3].T @ (pc - pose[:, 3])
    return tuple(int(v) for v in np.floor(pw / BLOCK + 1e-9))


def _unique(blocks):
    seen, out = set(), []
    for b in blocks:
        if b not in seen and all(-32000 < v < 32000 for v in b):
            seen.add(b)
            out.append(b)
    return out


def _admissible(blocks, pose, W, H, intr):
    if not blocks:
        return []
    ok = project64(np.array(blocks), pose, W, H, intr)["admissible"]
    return [b for b, k in zip(blocks, ok) if k]


def far_blocks(W, H, pose, intr):
    rc, rr, _ = region(W, H)
    t = [(u, v) for v in np.arange(0.3, rr + 1.0, 0.67) for u in np.arange(0.3, rc + 1.0, 0.67)]
    mu, mv = rc / 2 + 0.1, rr / 2 + 0.1
    t += [(-2.5, mv), (0.0, mv), (W - 1.0, mv), (W + 2.5, mv), (mu, -2.5), (mu, 0.0), (mu, H - 1.0), (mu, H + 2.5)]
    return _admissible(_unique([block_at(pose, intr, u, v, 2.0) for u, v in t]), pose, W, H, intr)


def near_blocks(W, H, pose, intr):
    rc, rr, nrows = region(W, H)
    us = [u for u in (0.5, rc / 2, rc - 0.4, rc + 1.5, 2 * rc + 0.5, 4 * rc, W - 1.5) if u < W]
    vs = [v for v in (0.5, rr / 2, rr - 0.4, rr + 1.5, nrows - 0.5, nrows + 1.5, 2 * nrows, 3 * nrows, H - 1.5) if v < H]
    t = [block_at(pose, intr, u, v, z) for z in (0.06, 0.1, 0.17, 0.25) for v in vs for u in us]
    return _admissible(_unique(t), pose, W, H, intr)


def straddle_blocks(W, H, pose, intr, exclude=()):
    """(blocks, the two of them that are listed without a block: ptr -1 and -2, in no family of `exclude`)."""
    p = np.asarray(pose, np.float64)
    centre = np.floor(-(p[:, :3].T @ p[:, 3]) / BLOCK).astype(int)
    r = np.arange(-3, 4)
    cand = (np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3) + centre)
    g = project64(cand, pose, W, H, intr)
    ok = g["admissible"]
    zf = g["zfront"]
    kinds = [ok & (g["nbehind"] == k) for k in range(1, 9)]
    kinds.append(ok & (g["nbehind"] < 8) & (zf[:, 1] < float(VERY_CLOSE)))                       # all_close
    raised = ok & g["valid"] & (zf[:, 0] < float(VERY_CLOSE)) & (zf[:, 1] >= float(VERY_CLOSE))
    kinds.append(raised)
    out = []
    for m in kinds:
        idx = np.flatnonzero(m)
        idx = idx[np.argsort(~g["valid"][idx], kind="stable")]            # boxes that are kept first
        out += [tuple(int(v) for v in cand[i]) for i in idx[:3]]
    out = _unique(out)
    noblock = [tuple(int(v) for v in cand[i]) for i in np.flatnonzero(raised) if tuple(int(v) for v in cand[i]) not in out
               and tuple(int(v) for v in cand[i]) not in exclude][:2]
    return out + noblock, noblock


def wide_blocks(W, H, pose, intr):
    """(blocks, the common /8 row): four boxes each of exactly ED_WIDE and ED_WIDE + 1 columns in the row most of the
    candidates cover, then every candidate wider than that over the row (the scene takes the first WIDE_BOXES that
    find a free bucket)."""
    fx, fy, cx, cy = (float(v) for v in intr)
    p = np.asarray(pose, np.float64)
    rc, rr, _ = region(W, H)
    xmax = ((W - 1) * SUB - cx) / fx * 0.44
    xs = np.arange(-0.4, xmax + 0.05, 0.02)
    ys = np.arange(-0.4, 0.4, 0.02)
    zs = np.arange(0.02, 0.45, 0.02)
    pc = np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), axis=-1).reshape(-1, 3)
    cand = np.unique(np.floor((pc - p[:, 3]) @ p[:, :3] / BLOCK).astype(np.int64), axis=0)
    g = project64(cand, pose, W, H, intr)
    ok = g["admissible"] & g["valid"] & (g["nbehind"] == 0)
    width = g["box"][:, 2] - g["box"][:, 0] + 1
    covers = [(ok & (g["box"][:, 1] <= r) & (g["box"][:, 3] >= r)) for r in range(rr)]
    row = int(np.argmax([(c & (width > ED_WIDE)).sum() for c in covers]))
    c = covers[row]
    pick = list(np.flatnonzero(c & (width == ED_WIDE))[:4]) + list(np.flatnonzero(c & (width == ED_WIDE + 1))[:4])
    pick += list(np.flatnonzero(c & (width > ED_WIDE + 1)))
    return _unique([tuple(int(v) for v in cand[i]) for i in pick]), row


class Scene:
    """One hash table for a size: `hash` (HASH_DTYPE, N_TOTAL), `n_alloc` blocks, `fam[(pose name, family)]` the
    family's entries in ascending order, `wide_row[pose name]`, `blocks_of(ids)`."""

    def __init__(self, W, H, intr=None):
        self.W, self.H = W, H
        self.intr = intr_of(W, H) if intr is None else np.asarray(intr, np.float32)
        fams, noblock, self.wide_row = {}, [], {}
        for pn, pose in POSES.items():
            fams[(pn, "far")] = far_blocks(W, H, pose, self.intr)
            fams[(pn, "near")] = near_blocks(W, H, pose, self.intr)
            fams[(pn, "wide")], self.wide_row[pn] = wide_blocks(W, H, pose, self.intr)
        others = {b for bl in fams.values() for b in bl}
        for pn, pose in POSES.items():
            fams[(pn, "straddle")], nb = straddle_blocks(W, H, pose, self.intr, others)
            noblock += nb
        # one entry per block, one block per bucket (a later block whose bucket is taken is left out)
        taken, entry = {}, {}
        for key in sorted(fams, key=lambda k: (("straddle", "far", "near", "wide").index(k[1]), k)):   # (the few first)
            placed = []
            for b in fams[key]:
                if key[1] == "wide" and len(placed) >= WIDE_BOXES + 8:
                    break
                if b not in entry:
                    h = hash_index(*b, TABLES["n_buckets"])
                    if h in taken:
                        continue
                    taken[h] = b
                    entry[b] = h
                placed.append(b)
            fams[key] = placed
        self.hash = empty_hash(N_TOTAL)
        noblock = [b for b in noblock if b in entry]
        ptr = 0
        for h in sorted(taken):
            b = taken[h]
            self.hash[h]["x"], self.hash[h]["y"], self.hash[h]["z"] = b
            if b in noblock:
                self.hash[h]["ptr"] = -1 - noblock.index(b) % 2
            else:
                self.hash[h]["ptr"] = ptr
                ptr += 1
        self.n_alloc = ptr
        self.fam = {key: np.array(sorted(entry[b] for b in bl if b in entry), np.int32) for key, bl in fams.items()}
        self.hash.setflags(write=False)

    def blocks_of(self, ids):
        h = self.hash[np.asarray(ids, np.int64)]
        return np.stack([h["x"], h["y"], h["z"]], axis=1).astype(np.int64)

    def hash_only(self, ids):
        """The table with the entries `ids` alone (a free view lists whatever its scan finds in the table)."""
        h = self.hash.copy()
        drop = np.ones(len(h), bool)
        drop[np.asarray(ids, np.int64)] = False
        h[drop] = (0, 0, 0, 0, 0, -2)
        return h

    def counters(self, n_visible):
        """(lastFreeBlockId, lastFreeExcessListId, noVisibleEntries) of the uploaded scene."""
        return TABLES["n_blocks"] - 1 - self.n_alloc, TABLES["n_excess"] - 1, int(n_visible)

    def project(self, ids, pose_name):
        return project64(self.blocks_of(ids), POSES[pose_name], self.W, self.H, self.intr)

    # ---- the lists -------------------------------------------------------------------------------------
    def base(self, pose_name, family):
        """The family's list in ascending entry order.  count_<n>: far + near cut or repeated to n entries; cap:
        the entries of far + near + wide whose box is kept."""
        if family.startswith("count_"):
            n = int(family[6:])
            both = np.union1d(self.fam[(pose_name, "far")], self.fam[(pose_name, "near")]).astype(np.int32)
            return np.sort(np.resize(both, n)).astype(np.int32)
        if family == "cap":
            ids = functools.reduce(np.union1d, [self.fam[(pose_name, f)] for f in ("far", "near", "wide")]).astype(np.int32)
            return ids[self.project(ids, pose_name)["valid"]]
        return self.fam[(pose_name, family)]

    def ordered(self, pose_name, family, order):
        ids = self.base(pose_name, family)
        if order == "reversed":
            return ids[::-1].copy()
        if order == "shuffled":
            return np.random.default_rng(20260 + len(ids)).permutation(ids).astype(np.int32)
        assert order == "ascending"
        return ids.copy()


@functools.lru_cache(maxsize=None)
def scene(W, H, view_cols=None):
    """The scene of a context size, or (view_cols given) of a free view W x H with the intrinsics of a view
    `view_cols` wide (tests/view_ref.py's intr_of)."""
    return Scene(W, H, None if view_cols is None else intr_of(view_cols, view_cols * 3 // 4))


FAMILIES = ("far", "near", "straddle", "wide")
COUNT_FAMILIES = tuple(f"count_{n}" for n in COUNTS)


def serial_cap(need, cap):
    """projectAndSplitBlocks_device's drop rule in list order: kept[i] = need[i] > 0 and off[i] + need[i] <= cap,
    where off advances over every box, dropped ones too.  -> (kept, noTotalBlocks)."""
    need = np.asarray(need, np.int64)
    off = np.cumsum(need) - need
    return (need > 0) & (off + need <= cap), int(min(need.sum(), cap))


def first_deciding(box, z, W, H, start):
    """The first entry k >= start whose box lowers a zmin or raises a zmax of the image of the entries before it: with
    entries 0..k kept, leaving k out changes the image."""
    img = fill(box[:start], z[:start], np.ones(start, bool), W, H)
    for k in range(start, len(box)):
        ulx, uly, lrx, lry = box[k]
        r = img[uly:lry + 1, ulx:lrx + 1]
        if (r[..., 0] > np.float32(z[k][0])).any() or (r[..., 1] < np.float32(z[k][1])).any():
            return k
        r[..., 0] = np.minimum(r[..., 0], np.float32(z[k][0]))
        r[..., 1] = np.maximum(r[..., 1], np.float32(z[k][1]))
    raise AssertionError("no entry decides a pixel on its own")


def cap_points(need, box, z, W, H):
    """max_render_blocks values that put the cap on each edge for a list of boxes that need `need` tiles (every entry
    kept without a cap, at least 258 of them): name -> cap, or None where the list has no such place.  exact_fit is
    met (off + need == cap) by an entry past the middle whose box decides pixels on its own, so that dropping it
    shows."""
    need = np.asarray(need, np.int64)
    assert len(need) >= 258 and (need > 0).all()
    off = np.cumsum(need) - need
    total = int(need.sum())
    k = first_deciding(box, z, W, H, len(need) // 2 + 7)
    assert k < len(need) - 1
    multi = [i for i in range(1, len(need) - 1) if need[i] >= 2 and need[i + 1] == 1]
    return {"total_eq_cap": total, "total_eq_cap_plus_1": total - 1,
            "first_drop_255": int(off[255] + need[255] - 1), "first_drop_256": int(off[256] + need[256] - 1),
            "first_drop_last": total - 1, "exact_fit": int(off[k] + need[k]),
            "multi_then_single": int(off[multi[len(multi) // 2]] + 1) if multi else None}


def cap_expect(name, need, cap):
    """What cap_points' `name` promises, as (first dropped entry or None, entries kept)."""
    kept, _ = serial_cap(need, cap)
    dropped = np.flatnonzero(~kept)
    return (int(dropped[0]) if len(dropped) else None), kept


def fill(boxes, z, kept, W, H):
    """fillBlocks_device in numpy: the range image of the kept boxes over memset(FAR_AWAY, VERY_CLOSE)."""
    img = np.empty((H, W, 2), np.float32)
    img[..., 0], img[..., 1] = FAR_AWAY, VERY_CLOSE
    for (ulx, uly, lrx, lry), (zmin, zmax), k in zip(boxes, z, kept):
        if k:
            r = img[uly:lry + 1, ulx:lrx + 1]
            r[..., 0] = np.minimum(r[..., 0], np.float32(zmin))
            r[..., 1] = np.maximum(r[..., 1], np.float32(zmax))
    return img


# ---- the fused frame path: blocks injected into a running sequence ------------------------------------
FRAME_SIZE, FRAME_COUNT = (100, 76), 4          # tests/offdefault_cases.py's orbit sequence, all frames tracked


FRAME_TABLES = dict(n_buckets=0x10000, n_excess=0x2000, n_blocks=0x2000, vis_capacity=0x4000)   # (small: quick transfers)


def frame_params(**kw):
    W, H = FRAME_SIZE
    fx, fy, cx, cy = synth.intrinsics(W, H)
    return dict(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, **FRAME_TABLES, **kw)


def frame_sequence():
    import offdefault_cases as C
    return C.sequence(8, *FRAME_SIZE)[:FRAME_COUNT]


def inject(state, blocks, n_buckets):
    """The scene state with `blocks` added: each in its own empty bucket (others are left out), its ptr taken from the
    top of the free list, its entry appended to the visible list.  state: dict(hash, alloc_list, visible_ids (whole
    buffer), counters (lastFreeBlockId, lastFreeExcessListId, noVisibleEntries), ...) -> (new state, the new entries)."""
    out = dict(state)
    h, ids = state["hash"].copy(), state["visible_ids"].copy()
    last, last_excess, n = state["counters"]
    entries = []
    for b in blocks:
        i = hash_index(*b, n_buckets)
        if h[i]["ptr"] != -2 or h[i]["offset"] != 0:
            continue
        h[i]["x"], h[i]["y"], h[i]["z"] = b
        h[i]["ptr"] = state["alloc_list"][last]
        last -= 1
        ids[n] = i
        n += 1
        entries.append(i)
    out.update(hash=h, visible_ids=ids, counters=(last, last_excess, n))
    return out, np.array(entries, np.int32)


def _frame_state(O, o, blocks):
    c = o.counters()
    ids = np.zeros(o.params.vis_capacity, np.int32)
    ids[:c["noVisibleEntries"]] = o.visible_ids()
    state = dict(hash=o.hash(), vba=o.vba(), alloc_list=o.alloc_list(), excess_list=o.excess_list(), visible_ids=ids,
                 visible_type=o.visible_type(), total1=c["noTotalBlocks"],
                 counters=(c["lastFreeBlockId"], c["lastFreeExcessListId"], c["noVisibleEntries"]))
    return inject(state, blocks, o.params.n_buckets)


STILL = dict(icp_iter_num=(0, 0, 0, 0))          # no ICP iteration: the pose stays where it is, whatever the range image


@functools.lru_cache(maxsize=None)
def _frame_blocks(still):
    """The near and the wide blocks of the pose after frame 1 that checkBlockVisibility sees then and after frame 2
    (frame 2's pose does not depend on them: its ICP runs on frame 1's maps)."""
    from oracle import oracle as O
    W, H = FRAME_SIZE
    o = O.Oracle(O.default_params(**frame_params(**(STILL if still else {}))))
    seq = frame_sequence()
    assert o(seq[0]) and o(seq[1])
    w2c = O.rigid_inv(o.pose())
    intr = intr_of(W, H)
    blocks = _unique(near_blocks(W, H, w2c, intr) + wide_blocks(W, H, w2c, intr)[0])
    seen = o.block_visibility(w2c, np.array(blocks, np.int16))[0]
    blocks = [b for b, v in zip(blocks, seen) if v]
    state, entries = _frame_state(O, o, blocks)
    frame_load(o, state)
    assert o(seq[2])
    left = set(int(v) for v in o.visible_ids())
    h = state["hash"][entries]
    return tuple((int(x), int(y), int(z)) for x, y, z, e in zip(h["x"], h["y"], h["z"], entries) if int(e) in left)


def frame_setup(O, **kw):
    """The oracle (created with `kw`) after frames 0 and 1 of the sequence, and what to write into both sides before
    frame 2.  -> (oracle, state for frame_load / tf_upload, injected entries)."""
    o = O.Oracle(O.default_params(**frame_params(**kw)))
    seq = frame_sequence()
    assert o(seq[0]) and o(seq[1])
    state, entries = _frame_state(O, o, list(_frame_blocks("icp_iter_num" in kw)))
    empty = state["vba"].reshape(-1, 512)[state["hash"]["ptr"][entries]]
    assert (empty["sdf"] == 32767).all() and (empty["w"] == 0).all()       # never-used blocks: the cleared state
    return o, state, entries


def frame_tiles(O, o):
    """(list, kept boxes' need, box, z) of the oracle's visible list projected at its current pose."""
    vis = o.visible_ids()
    valid, box, z = o.project_blocks(O.rigid_inv(o.pose()), vis)
    box = box.astype(np.int64)
    need = np.where(valid != 0, -(-(box[:, 2] - box[:, 0] + 1) // RB) * -(-(box[:, 3] - box[:, 1] + 1) // RB), 0)
    return vis, need, box, z


@functools.lru_cache(maxsize=None)
def frame_cap():
    """(max_render_blocks, k) for a STILL context: the cap that frame 2's list meets exactly at its entry k (off + need
    == cap), the last injected entry whose box alone decides pixels of the /8 region.  The list is in ascending entry order and ends with the excess
    entries, so such a cap is below frame 1's total too and frame 1's range image is capped.  With ICP iterations the
    pose of frame 2, and with it the list, would move with the cap; in a STILL context it cannot, so the uncapped
    run's offsets hold."""
    from oracle import oracle as O
    o, state, entries = frame_setup(O, **STILL)
    frame_load(o, state)
    assert o(frame_sequence()[2])
    vis, need, box, z = frame_tiles(O, o)
    off = np.cumsum(need) - need
    W, H = FRAME_SIZE
    rc, rr, _ = region(W, H)
    for k in np.flatnonzero(np.isin(vis, entries) & (need > 0))[::-1]:
        cap = int(off[k] + need[k])
        kept, _ = serial_cap(need, cap)
        without = kept.copy()
        without[k] = False
        a, b = fill(box, z, kept, W, H), fill(box, z, without, W, H)
        if (a[:rr, :rc] != b[:rr, :rc]).sum() >= 8:          # entry k alone decides /8 pixels the rays read
            assert cap < int(need.sum())
            return cap, int(k)
    raise AssertionError("no injected box decides a pixel of the /8 region on its own")


def frame_threshold(n_before, n_injected):
    """The TFUSION_ED_LDS_MAX_N between the visible count frame 1's CreateExpectedDepths saw and frame 2's."""
    return n_before + n_injected // 2


def frame_load(o, state):
    o.load_scene_state(state["hash"], state["vba"], state["alloc_list"], state["excess_list"], state["visible_ids"],
                       state["visible_type"], state["counters"])
