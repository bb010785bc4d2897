"""Serial restatement of the map merge (DESIGN.md §5 Map merge; the library's side is tf_map_merge in
topfusion_amd/csrc/tf_scene_ckpt.hip), over scene_ckpt_ref state dicts.

merge(target, file, offset) is the state the target reaches when the file's carried records (entry.ptr >= 0, in file
order), moved by `offset` whole blocks, are applied one at a time: the reference's allocation walk (vbh_ref.probe)
looks the position up in the live table; found with a block -- every voxel becomes CombineVoxelInformation(file,
context) (mesh_whole_ref.combine, held to the oracle); found with ptr == -1 -- the entry takes
allocList[lastFreeBlockId--] and the file's block; not found -- inserted by allocateVoxelBlocksList's rule
(vbh_ref.place: the free bucket entry, or excessList[lastFreeExcessListId--] linked to the end of the chain).
closed_form() is what a parallel implementation computes instead of the loop.  made_pair() is a target and a file in
small tables that hit every case."""
import numpy as np

import mesh_whole_ref as MW
import scene_ckpt_ref as R
import vbh_ref as V
from vbh_ref import HASH_DTYPE, VOXEL_DTYPE, VOXEL_RESET, hash_index

REPORT_KEYS = ("records_combined", "records_inserted", "records_revived", "records_skipped", "blocks_used", "excess_used")
COMBINE, REVIVE, INSERT = 1, 2, 3
GRID_HALF = 128                                         # the block grid spans [-128, 128) blocks


class Capacity(Exception):
    """The free lists are too short; .report holds what would have been needed."""

    def __init__(self, report):
        super().__init__(str(report))
        self.report = report


class Invalid(Exception):
    """Outside the merge's scope, or a file the serial rule is not defined on."""


def _bits(v):
    return np.asarray(v, np.float32).tobytes()


def carried(file, offset=(0, 0, 0)):
    """(record numbers, positions + offset (int64 (n, 3)), file ptrs) of the records with ptr >= 0, in file order, and
    the number of records."""
    rec = R.records_of(file)
    e = rec["entry"]
    k = np.flatnonzero(e["ptr"] >= 0)
    pos = np.stack([e["x"][k], e["y"][k], e["z"][k]], 1).astype(np.int64) + np.asarray(offset, np.int64)
    return k, pos, e["ptr"][k].astype(np.int64), len(rec)


def check(target, file, offset=(0, 0, 0)):
    """Raises Invalid for what tf_map_merge refuses with TF_INVALID_ARG (the file itself is taken as valid)."""
    p, q = target["params"], file["params"]
    for s in (target, file):
        if int(s["params"]["use_swapping"]) or int(s["params"]["voxel_rgb"]) or s["rgb"] is not None or "swapState" in s:
            raise Invalid("a swapping or a colour state")
    if _bits(p["voxelSize"]) != _bits(q["voxelSize"]) or _bits(p["mu"]) != _bits(q["mu"]) or int(p["maxW"]) != int(q["maxW"]):
        raise Invalid("voxelSize, mu or maxW differ")
    _, pos, _, _ = carried(file, offset)
    if len(pos) and (pos.min() < -32768 or pos.max() > 32767):
        raise Invalid("the offset takes a position outside int16")
    if len(np.unique(pos, axis=0)) != len(pos):
        raise Invalid("two carried records share a position")


def _loop(target, file, offset, unlimited):
    """The serial loop.  `unlimited`: both free lists never run out (virtual slots behind the tables, no voxels
    moved) -- the report of what the merge needs."""
    nb, ne, nblk = (int(target["params"][k]) for k in ("n_buckets", "n_excess", "n_blocks"))
    maxW = int(target["params"]["maxW"])
    k, pos, fptr, n_rec = carried(file, offset)
    hash_ = np.array(target["hash"], HASH_DTYPE)
    vis = np.array(target["visType"], np.uint8)
    vba = np.array(target["vba"]).view(np.uint32).reshape(-1, 512)
    src = np.asarray(file["vba"]).view(np.uint32).reshape(-1, 512)
    alloc, excess = np.asarray(target["allocList"], np.int64), np.asarray(target["excessList"], np.int64)
    v, e = target["counters"]["lastFreeBlockId"], target["counters"]["lastFreeExcessListId"]
    if unlimited:                                       # virtual slots behind the real ones, taken when those run out
        m = len(pos)
        hash_ = np.concatenate([hash_, V.empty_hash(m)])
        vis = np.concatenate([vis, np.zeros(m, np.uint8)])
        alloc = np.concatenate([nblk + np.arange(m)[::-1], alloc[:v + 1]])
        excess = np.concatenate([ne + np.arange(m)[::-1], excess[:e + 1]])
        v, e = v + m, e + m
    v0, e0 = v, e
    n = dict.fromkeys(REPORT_KEYS, 0)
    n["records_skipped"] = n_rec - len(pos)

    def take_block(f):
        nonlocal v
        ptr = int(alloc[v])
        v -= 1
        if ptr < nblk:
            vba[ptr] = src[f]
        return ptr

    for p, f in zip(pos, fptr):
        idx, rtype, found = V.probe(hash_, nb, p)
        if rtype == 0 and found in (V.FOUND_BUCKET, V.FOUND_CHAIN):
            ptr = int(hash_["ptr"][idx])
            vba[ptr] = MW.combine(src[f].view(VOXEL_DTYPE), vba[ptr].view(VOXEL_DTYPE), maxW).view(np.uint32)
            n["records_combined"] += 1
        elif rtype == 0:
            hash_["ptr"][idx] = take_block(f)
            n["records_revived"] += 1
        else:
            t, e = V.place(hash_, nb, p, take_block(f), excess, e)
            vis[t] = 0
            n["records_inserted"] += 1
    n["blocks_used"], n["excess_used"] = v0 - v, e0 - e
    return hash_, vis, vba, n


def needs(target, file, offset=(0, 0, 0)):
    """The report: a function of the target's table and the file's carried positions."""
    check(target, file, offset)
    return _loop(target, file, offset, True)[3]


def merge(target, file, offset=(0, 0, 0)):
    """(state', report); Invalid, Capacity(report).  The inputs are left as they are."""
    report = needs(target, file, offset)
    c = target["counters"]
    if report["blocks_used"] > c["lastFreeBlockId"] + 1 or report["excess_used"] > c["lastFreeExcessListId"] + 1:
        raise Capacity(report)
    hash_, vis, vba, again = _loop(target, file, offset, False)
    assert again == report
    out = dict(target)
    out.update(hash=hash_, visType=vis, vba=vba.reshape(-1), params=target["params"].copy(),
               pose=np.asarray(target["pose"], np.float32).copy(), visibleIds=np.asarray(target["visibleIds"], np.int32).copy(),
               allocList=np.asarray(target["allocList"], np.int32).copy(), excessList=np.asarray(target["excessList"], np.int32).copy(),
               maps=[np.asarray(m, np.float32).copy() for m in target["maps"]],
               counters=dict(c, lastFreeBlockId=c["lastFreeBlockId"] - report["blocks_used"],
                             lastFreeExcessListId=c["lastFreeExcessListId"] - report["excess_used"]))
    return out, report


def closed_form(target, file, offset=(0, 0, 0)):
    """Per carried record j, in file order: [record number, mode, h, m, t, ptr', link] -- mode COMBINE / REVIVE / INSERT
    from a walk of the table as it was; m the rank among the records not found of bucket h (-1 when found); t the
    entry (the found one, h, or n_buckets + excessList[lastFreeExcessListId - o]); ptr' the block (the found entry's,
    or allocList[lastFreeBlockId - b]); link the entry whose offset names t (-1: none).  o / b: the earlier records
    that need an excess slot / a block."""
    nb = int(target["params"]["n_buckets"])
    hash_ = target["hash"]
    alloc, excess = target["allocList"], target["excessList"]
    v, e = target["counters"]["lastFreeBlockId"], target["counters"]["lastFreeExcessListId"]
    k, pos, _, _ = carried(file, offset)
    seen, last, rows = {}, {}, []
    o = b = 0
    for rk, p in zip(k, pos):
        idx, rtype, found = V.probe(hash_, nb, p)
        if rtype == 0:
            if found in (V.FOUND_BUCKET, V.FOUND_CHAIN):
                rows.append([int(rk), COMBINE, -1, -1, idx, int(hash_["ptr"][idx]), -1])
            else:
                rows.append([int(rk), REVIVE, -1, -1, idx, int(alloc[v - b]), -1])
                b += 1
            continue
        h = hash_index(int(p[0]), int(p[1]), int(p[2]), nb)
        m = seen.get(h, 0)
        seen[h] = m + 1
        if m == 0 and rtype == 1:
            t, link = h, -1
        else:
            t = nb + int(excess[e - o])
            o += 1
            link = idx if m == 0 else rows[last[h]][4]
        last[h] = len(rows)
        rows.append([int(rk), INSERT, h, m, t, int(alloc[v - b]), link])
        b += 1
    return rows


def kinds(target, file, offset=(0, 0, 0)):
    """How often each case of the merge occurs for this pair: a dict of counts."""
    nb, maxW = int(target["params"]["n_buckets"]), int(target["params"]["maxW"])
    rows = closed_form(target, file, offset)
    _, pos, fptr, n_rec = carried(file, offset)
    free_bucket, per_bucket = {}, {}
    for r in rows:
        if r[1] == INSERT:
            per_bucket[r[2]] = per_bucket.get(r[2], 0) + 1
            if r[3] == 0:
                free_bucket[r[2]] = r[4] == r[2]
    src = np.asarray(file["vba"]).view(VOXEL_DTYPE).reshape(-1, 512)
    dst = np.asarray(target["vba"]).view(VOXEL_DTYPE).reshape(-1, 512)
    w0 = wmax = wpast = 0
    for r, f in zip(rows, fptr):
        if r[1] == COMBINE:
            a, d = src[f]["w"].astype(int), dst[r[5]]["w"].astype(int)
            w0 += int((a == 0).sum())
            wmax += int((a == maxW).sum())
            wpast += int(((a > 0) & (a + d > maxW)).sum())
    orphan = sum(1 for h in range(nb) if int(target["hash"]["ptr"][h]) < -1 and int(target["hash"]["offset"][h]) >= 1)
    return dict(combined=sum(r[1] == COMBINE for r in rows), revived=sum(r[1] == REVIVE for r in rows),
                new_free_bucket=sum(r[1] == INSERT and r[4] < nb for r in rows),
                new_chain_end=sum(r[1] == INSERT and r[3] == 0 and r[4] >= nb for r in rows),
                buckets_several_new_free=sum(1 for h, c in per_bucket.items() if c >= 2 and free_bucket[h]),
                buckets_several_new_chain=sum(1 for h, c in per_bucket.items() if c >= 2 and not free_bucket[h]),
                longest_new_run=max(per_bucket.values(), default=0),
                new_into_orphaned_bucket=sum(r[1] == INSERT and r[4] < nb and int(target["hash"]["offset"][r[2]]) >= 1 for r in rows),
                orphaned_buckets=orphan, skipped=n_rec - len(pos), w_zero=w0, w_max=wmax, w_past_max=wpast,
                off_grid=int(((pos < -GRID_HALF) | (pos >= GRID_HALF)).any(axis=1).sum()),
                off_grid_new=sum(r[1] == INSERT and bool(((p < -GRID_HALF) | (p >= GRID_HALF)).any()) for r, p in zip(rows, pos)))


def with_free(target, n_blocks_free, n_excess_free):
    """The target with only the top n_blocks_free / n_excess_free values of its free lists left (the merge takes from
    the top, so what it places where does not change)."""
    c = target["counters"]
    v, e = c["lastFreeBlockId"], c["lastFreeExcessListId"]
    assert 0 <= n_blocks_free <= v + 1 and 0 <= n_excess_free <= e + 1
    out = dict(target)
    alloc, excess = np.array(target["allocList"], np.int32), np.array(target["excessList"], np.int32)
    alloc[:n_blocks_free] = alloc[v + 1 - n_blocks_free:v + 1].copy()
    excess[:n_excess_free] = excess[e + 1 - n_excess_free:e + 1].copy()
    out.update(allocList=alloc, excessList=excess,
               counters=dict(c, lastFreeBlockId=n_blocks_free - 1, lastFreeExcessListId=n_excess_free - 1))
    return out


# ---- a made pair for the tests -------------------------------------------------------------------------------------------
MADE = dict(n_buckets=256, n_excess=768, n_blocks=640)              # the target's tables
MADE_FILE = dict(n_buckets=128, n_excess=512, n_blocks=512)         # the file's: other capacities, another image size
MADE_OFFSET = (95, 0, -100)                                         # positions lie in [-40, 40]: part of them leaves the grid
MAXW = 100


def _voxels(rng, n_blocks):
    """Weights 0, maxW and in between in equal parts; every sdf; a top byte of its own."""
    n = n_blocks * 512
    kind = rng.integers(0, 4, n)
    w = np.where(kind == 0, 0, np.where(kind == 1, MAXW, rng.integers(1, MAXW, n))).astype(np.uint32)
    return rng.integers(0, 1 << 16, n, dtype=np.uint32) | w << 16 | rng.integers(0, 256, n, dtype=np.uint32) << 24


def _state(rng, pos, holds, tables, cols, rows, extra_vis=()):
    """Positions laid out by the reference's allocation (synth.build_hash) in `tables`, shuffled blocks for those that
    hold one (the others ptr -1), shuffled free lists."""
    from topfusion_amd import synth
    nb, ne, nblk = tables["n_buckets"], tables["n_excess"], tables["n_blocks"]
    h, entry, last_excess = synth.build_hash(np.asarray(pos, np.int64), nb, ne, HASH_DTYPE)
    held = np.flatnonzero(holds)
    blocks = rng.permutation(nblk)
    h["ptr"][entry] = -1
    h["ptr"][entry[held]] = blocks[:len(held)]
    free = blocks[len(held):]
    vba = _voxels(rng, nblk)
    vba.reshape(-1, 512)[free] = VOXEL_RESET
    alloc = np.arange(nblk, dtype=np.int32)
    alloc[:len(free)] = free
    excess = np.arange(ne, dtype=np.int32)
    excess[:last_excess + 1] = rng.permutation(last_excess + 1)
    vis = np.zeros(nb + ne, np.uint8)
    vis[entry[::3]] = 1
    vis[entry[1::7]] = 3
    for i in extra_vis:
        if h["ptr"][i] == -2:
            vis[i] = 2
    ids = np.flatnonzero(vis == 1).astype(np.int32)
    p = R.tiny_state(cols=cols, rows=rows, n_buckets=nb, n_excess=ne, n_blocks=nblk)["params"]
    p["vis_capacity"], p["max_render_blocks"], p["maxW"] = 4096, 4096, MAXW
    pose = np.eye(4, dtype=np.float32)[:3].reshape(12).copy()
    pose[[3, 7, 11]] = (0.125, -0.5, 0.75)
    maps = [rng.standard_normal((rows >> l, cols >> l, 4)).astype(np.float32) for l in range(3) for _ in range(2)]
    s = dict(params=p, pose_algebra=4, pose=pose, hash=h, visType=vis, vba=vba, rgb=None, visibleIds=ids, allocList=alloc,
             excessList=excess, maps=maps,
             counters=dict(lastFreeBlockId=len(free) - 1, lastFreeExcessListId=int(last_excess), noVisibleEntries=len(ids),
                           frame_counter=9))
    return s, entry


_pair = {}


def made_pair(seed=23):
    """(target, file): see the module text.  The target: 330 positions in MADE's tables (chains of one to four and more
    entries), a seventh of them with ptr == -1, three buckets whose entry was freed while its chain stayed, shuffled
    and partly consumed free lists.  The file, in MADE_FILE's tables at 64 x 48: positions the target holds with a
    block and with ptr == -1, each both as they are and moved back by MADE_OFFSET (so that either offset finds some),
    new positions -- random ones, and runs of five into one free bucket, one orphaned bucket and one chain -- records
    with ptr == -1 and records that only kept a visType."""
    if seed in _pair:
        return _pair[seed]
    rng = np.random.default_rng(seed)
    off = np.asarray(MADE_OFFSET, np.int64)
    nb = MADE["n_buckets"]
    cand = rng.integers(-40, 41, (6000, 3))
    cand = cand[np.sort(np.unique(cand, axis=0, return_index=True)[1])]
    tpos, rest = cand[:330], cand[330:]
    holds = rng.integers(0, 7, len(tpos)) > 0
    target, entry = _state(rng, tpos, holds, MADE, 96, 72)
    h = target["hash"]
    # three buckets with a chain lose their bucket entry (ptr -2, the offset stays): the chain is no longer reachable
    chained = [int(i) for i in np.flatnonzero((h["offset"][:nb] >= 1) & (h["ptr"][:nb] >= 0))][:3]
    orphaned = set()
    for b in chained:
        orphaned.update(V.chain(h, nb, (h["x"][b], h["y"][b], h["z"][b])))
        h["ptr"][b] = -2
        target["visType"][b] = 0
    target["visibleIds"] = np.flatnonzero(target["visType"] == 1).astype(np.int32)
    target["counters"]["noVisibleEntries"] = len(target["visibleIds"])
    target["counters"]["frame_counter"] = 0            # (no upload sets it; the file keeps its own, which a merge ignores)
    reach = np.array([int(e) not in orphaned for e in entry])
    with_block = tpos[reach & holds]
    without = tpos[reach & ~holds]
    hb = lambda p: hash_index(int(p[0]), int(p[1]), int(p[2]), nb)
    occupied = set(hb(p) for p in tpos)

    def run(pool, want, count, taken):
        out = []
        for p in pool:
            if hb(p) == want and tuple(p) not in taken:
                out.append(p)
                taken.add(tuple(p))
                if len(out) == count:
                    break
        assert len(out) == count
        return out

    taken = set(map(tuple, tpos)) | set(map(tuple, tpos - off)) | set(map(tuple, tpos + off))
    free_b = next(b for b in range(nb) if b not in occupied)
    long_b = max((b for b in occupied if b not in chained), key=lambda b: sum(hb(p) == b for p in tpos))
    big = rng.integers(-40, 41, (60000, 3))
    parts = [with_block[:70], with_block[70:140] - off, without[:15], without[15:30] - off]
    for shift in (0, off):                              # the runs, for either offset
        parts += [np.array(run(big, b, 5, taken)) - shift for b in (free_b, chained[0], long_b)]
    fresh = [p for p in rest if tuple(p) not in taken][:120]
    parts.append(np.array(fresh))
    fpos = np.concatenate(parts)
    assert len(np.unique(fpos, axis=0)) == len(fpos)
    extra = np.unique(rng.integers(-40, 41, (40, 3)), axis=0) + 500    # records without a block (ptr -1), far from the rest
    fall = np.concatenate([fpos, extra])
    order = rng.permutation(len(fall))
    fall, fholds = fall[order], (np.arange(len(fall)) < len(fpos))[order]
    n_total_f = MADE_FILE["n_buckets"] + MADE_FILE["n_excess"]
    file, _ = _state(rng, fall, fholds, MADE_FILE, 64, 48, extra_vis=(0, 255, 256, n_total_f - 1, 300, 401))
    _pair[seed] = (target, file)
    return _pair[seed]
