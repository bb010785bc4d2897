"""Serial restatement of the resized load (DESIGN.md §5 Resized load; the library's side is tf_map_load_resized in
topfusion_amd/csrc/tf_scene_ckpt.hip), over scene_ckpt_ref / scene_map_ref state dicts.

resize(state, n_buckets, n_excess, n_blocks, vis_capacity) is the state a freshly reset context of those capacities
reaches when the carried records of `state`'s file (entry.ptr >= -1, in file order) are inserted one at a time by the
reference's allocation rule (vbh_ref.place: the bucket entry when the bucket is empty, else the end of the bucket's
chain linked to excessList[lastFreeExcessListId--]); a block from allocList[lastFreeBlockId--] where the record has
one.  find_entry is vbh_ref.find_held: the whole chain, every entry that holds the position.  Records with ptr < -1 have no position and are dropped.  closed_form() is what a parallel
implementation computes instead of the loop."""
import numpy as np

import scene_map_ref as MR
from vbh_ref import HASH_DTYPE, VOXEL_RESET, empty_hash, find_held as find_entry, hash_index, place  # noqa: F401

REPORT_KEYS = ("records_carried", "records_dropped", "blocks", "cache_blocks", "excess_used", "longest_chain")


class Capacity(Exception):
    """The carried content does not fit; .report holds what would have been needed."""

    def __init__(self, report):
        super().__init__(str(report))
        self.report = report


def _record_fields(state):
    rec = MR.records_of(state)
    sw = MR.swapping(state)
    flag = rec["hasStoredData"] if sw else np.zeros(len(rec), np.uint8)
    return rec, sw, flag


def needs(state, n_buckets):
    """The report of a resize into n_buckets buckets: a function of the records and the hash size alone."""
    rec, _, flag = _record_fields(state)
    count = {}
    carried = dropped = blocks = cache = 0
    for r, f in zip(rec, flag):
        e = r["entry"]
        if int(e["ptr"]) < -1:
            dropped += 1
            continue
        carried += 1
        blocks += int(e["ptr"]) >= 0
        cache += int(f) == 1
        h = hash_index(int(e["x"]), int(e["y"]), int(e["z"]), n_buckets)
        count[h] = count.get(h, 0) + 1
    return dict(records_carried=carried, records_dropped=dropped, blocks=blocks, cache_blocks=cache,
                excess_used=carried - len(count), longest_chain=max(count.values(), default=0))


def resize(state, n_buckets, n_excess, n_blocks, vis_capacity):
    """(state', report), or Capacity.  A plain loop over the records."""
    rec, sw, flag = _record_fields(state)
    report = needs(state, n_buckets)
    if report["blocks"] > n_blocks or report["excess_used"] > n_excess:
        raise Capacity(report)
    rgb_src = state["rgb"]
    n_total = n_buckets + n_excess
    hash_ = empty_hash(n_total)
    vis, st, fl = (np.zeros(n_total, np.uint8) for _ in range(3))
    alloc, excess = np.arange(n_blocks, dtype=np.int32), np.arange(n_excess, dtype=np.int32)
    last_block, last_excess = n_blocks - 1, n_excess - 1
    vba = np.full((n_blocks, 512), VOXEL_RESET, np.uint32)
    rgb = None if rgb_src is None else np.zeros((n_blocks, 512), np.uint32)
    store = np.zeros((n_total, 512), np.uint32) if sw else None
    vba_src = np.asarray(state["vba"]).view(np.uint32).reshape(-1, 512)
    for r, f in zip(rec, flag):
        e = r["entry"]
        ptr = int(e["ptr"])
        if ptr < -1:
            continue
        new_ptr = -1
        if ptr >= 0:
            new_ptr = int(alloc[last_block])
            last_block -= 1
            vba[new_ptr] = vba_src[ptr]
            if rgb is not None:
                rgb[new_ptr] = np.asarray(rgb_src).view(np.uint32).reshape(-1, 512)[ptr]
        t, last_excess = place(hash_, n_buckets, (e["x"], e["y"], e["z"]), new_ptr, excess, last_excess)
        vis[t] = r["visType"]
        if sw:
            st[t], fl[t] = r["swapState"], f
            if f:
                store[t] = np.asarray(state["store"]).view(np.uint32).reshape(-1, 512)[int(r["index"])]
    ids = np.flatnonzero(vis > 0)[:vis_capacity].astype(np.int32)
    p = state["params"].copy()
    p["n_buckets"], p["n_excess"], p["n_blocks"], p["vis_capacity"] = n_buckets, n_excess, n_blocks, vis_capacity
    c = dict(state["counters"], lastFreeBlockId=last_block, lastFreeExcessListId=last_excess, noVisibleEntries=len(ids))
    out = dict(params=p, pose_algebra=state["pose_algebra"], counters=c, pose=np.asarray(state["pose"], np.float32).copy(),
               hash=hash_, visType=vis, vba=vba.reshape(-1), rgb=None if rgb is None else rgb.reshape(-1), visibleIds=ids,
               allocList=alloc, excessList=excess, maps=[np.asarray(m, np.float32).copy() for m in state["maps"]])
    if sw:
        out.update(swapState=st, swapFlags=fl, store=store.reshape(-1))
    return out, report


def closed_form(state, n_buckets, n_excess, n_blocks):
    """Per carried record j, in file order: (record number in the file, h, m, t, ptr', the t its entry links to or -1).
    m(j) = earlier carried records of the same h; o(j) = records before j with m > 0; b(j) = records before j with
    ptr >= 0; t = h if m == 0 else n_buckets + n_excess - 1 - o; ptr' = n_blocks - 1 - b, or -1."""
    rec = MR.records_of(state)
    seen, last, rows = {}, {}, []
    o = b = 0
    for k, r in enumerate(rec):
        e = r["entry"]
        ptr = int(e["ptr"])
        if ptr < -1:
            continue
        h = hash_index(int(e["x"]), int(e["y"]), int(e["z"]), n_buckets)
        m = seen.get(h, 0)
        seen[h] = m + 1
        t = h if m == 0 else n_buckets + n_excess - 1 - o
        if m > 0:
            rows[last[h]][5] = t
            o += 1
        new_ptr = -1
        if ptr >= 0:
            new_ptr = n_blocks - 1 - b
            b += 1
        last[h] = len(rows)
        rows.append([k, h, m, t, new_ptr, -1])
    return rows


# ---- a made map for the tests: random positions in a small table, every kind of record -------------------------------
MADE = dict(n_buckets=256, n_excess=768, n_blocks=640)
MADE_TARGET_BUCKETS = (64, 256, 1024)              # file / 4, the file's, file x 4
# tf_create wants (n_buckets + n_excess) % 16 == 0.  The excess slots X a target needs are made a multiple of 16 where a
# context of exactly X is wanted, and 1 more than one at 4096 buckets, where one of X - 1 is (the refusal)
MADE_EXCESS_MOD16 = {64: 0, 256: 0, 1024: 0, 4096: 1}
MADE_SHORT_BUCKETS = 4096


def made_state(swapping, cols=96, rows=72, seed=41):
    """About 700 block positions laid out in MADE's tables by the reference's allocation (synth.build_hash), with
    shuffled VBA ptrs; a fifth of the entries without a block (ptr -1); with `swapping` stored-only, pending and merged
    entries; dropped records -- slots without a hash entry that kept a visType, a swap state or a flagged stored block --
    among them every free corner of the 256-entry groups; free lists and counters as the tables imply.  Without
    `swapping` a colour scene (version 1).  Positions are then added until the excess slots the target hash sizes need
    are as MADE_EXCESS_MOD16 says."""
    from topfusion_amd import synth
    import scene_ckpt_ref as R
    rng = np.random.default_rng(seed)
    cand = rng.integers(-40, 41, (4000, 3))
    cand = cand[np.sort(np.unique(cand, axis=0, return_index=True)[1])]
    pos = [tuple(int(v) for v in p) for p in cand[:700]]
    sizes = sorted(MADE_EXCESS_MOD16, reverse=True)
    hs = {nb: {} for nb in sizes}
    for p in pos:
        for nb in sizes:
            h = hash_index(*p, nb)
            hs[nb][h] = hs[nb].get(h, 0) + 1

    def excess_needed(nb):
        return sum(hs[nb].values()) - len(hs[nb])

    # a position that collides at 1024 buckets collides at 256 and 64 too: settle the largest table first, then add
    # only positions that take a bucket of their own in the tables already settled
    for k, nb in enumerate(sizes):
        for p in cand[700:]:
            if excess_needed(nb) % 16 == MADE_EXCESS_MOD16[nb]:
                break
            p = tuple(int(v) for v in p)
            if p in pos or hash_index(*p, nb) not in hs[nb] or any(hash_index(*p, b) in hs[b] for b in sizes[:k]):
                continue
            pos.append(p)
            for b in sizes:
                h = hash_index(*p, b)
                hs[b][h] = hs[b].get(h, 0) + 1
        assert excess_needed(nb) % 16 == MADE_EXCESS_MOD16[nb]
    pos = np.array(pos, np.int64)
    pos = pos[rng.permutation(len(pos))]
    nb, ne, nblk = MADE["n_buckets"], MADE["n_excess"], MADE["n_blocks"]
    n_total = nb + ne
    h, entry, last_excess = synth.build_hash(pos, nb, ne, HASH_DTYPE)
    kind = rng.integers(0, 5, len(pos))                  # 0: no block; the rest hold one
    held = np.flatnonzero(kind > 0)
    assert len(held) <= nblk - 8
    blocks = rng.permutation(nblk)
    h["ptr"][entry] = -1
    h["ptr"][entry[held]] = blocks[:len(held)]
    free = blocks[len(held):]
    vis = np.zeros(n_total, np.uint8)
    vis[entry[::3]] = 1
    vis[entry[1::7]] = 3
    vis[entry[2::11]] = 2
    unused = np.flatnonzero(h["ptr"] == -2)
    corners = [i for i in (0, 255, 256, n_total - 1) if h["ptr"][i] == -2]
    dropped = sorted(set(corners) | set(int(i) for i in unused[::29]))
    vis[dropped[::2]] = 2
    p = R.tiny_state(cols=cols, rows=rows, n_buckets=nb, n_excess=ne, n_blocks=nblk, voxel_rgb=0 if swapping else 1)["params"]
    p["vis_capacity"], p["max_render_blocks"] = 4096, 4096
    vba = rng.integers(0, 1 << 24, nblk * 512, dtype=np.uint32)
    vba.reshape(-1, 512)[free] = VOXEL_RESET
    alloc = np.arange(nblk, dtype=np.int32)
    alloc[:len(free)] = free
    ids = np.flatnonzero(vis == 1).astype(np.int32)
    pose = np.eye(4, dtype=np.float32)[:3].reshape(12).copy()
    pose[[3, 7, 11]] = (0.125, -0.5, 0.75)
    maps = [rng.standard_normal((rows >> l, cols >> l, 4)).astype(np.float32) for l in range(3) for _ in range(2)]
    s = dict(params=p, pose_algebra=4, pose=pose, hash=h, visType=vis, vba=vba, rgb=None, visibleIds=ids, allocList=alloc,
             excessList=np.arange(ne, dtype=np.int32), maps=maps,
             counters=dict(lastFreeBlockId=len(free) - 1, lastFreeExcessListId=int(last_excess), noVisibleEntries=len(ids),
                           frame_counter=9))
    if not swapping:
        s["rgb"] = rng.integers(0, 1 << 32, nblk * 512, dtype=np.uint32)
        s["rgb"].reshape(-1, 512)[free] = 0
        return s
    p["use_swapping"], p["swap_transfer_blocks"] = 1, 16
    st, fl = np.zeros(n_total, np.uint8), np.zeros(n_total, np.uint8)
    lost = entry[kind == 0]
    fl[lost[::2]] = 1                                    # stored only; the other half lost
    st[lost[1::4]] = 1
    fl[entry[kind == 1]], st[entry[kind == 1]] = 1, 1    # pending
    fl[entry[kind == 2]], st[entry[kind == 2]] = 1, 2    # merged
    st[entry[kind == 3]] = 2                             # active, never stored
    fl[dropped[1::2]] = 1                                # no hash entry left, a stored block
    st[dropped[1::4]] = 1
    for i in dropped:                                    # every dropped slot has a record
        if not (vis[i] or st[i] or fl[i]):
            st[i] = 1
    s.update(swapState=st, swapFlags=fl, store=rng.integers(0, 1 << 24, n_total * 512, dtype=np.uint32))
    return s
