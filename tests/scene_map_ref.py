"""Numpy restatement of the map checkpoint file (DESIGN.md §5 Map checkpoints; the library's side is
topfusion_amd/csrc/tf_scene_file.h), on top of scene_ckpt_ref: version 2 is the file of a swapping context.

A swapping state is scene_ckpt_ref's state dict (params["use_swapping"] == 1, rgb None) plus
    swapState     uint8[n_total]          HashSwapState::state per entry (0, 1, 2)
    swapFlags     uint8[n_total]          hasStoredData per entry (0, 1)
    store         uint32[n_total * 512]   the GlobalCache's block per entry; state only where the flag is 1

and allocList is state only in [0, lastFreeBlockId]: SaveToGlobalMemory pushes freed blocks back, so what a sequence
leaves above the top is stale (allocation and reallocation read at or below it, and every reset of a swapping context
is a full one, which rewrites the list); a load leaves the identity there.

pack / unpack / file_size / states_equal of a state without use_swapping are scene_ckpt_ref's (version 1)."""
import struct
import zlib

import numpy as np

import scene_ckpt_ref as R
from scene_ckpt_ref import BLOCK_BYTES, HASH_DTYPE, LEVELS, MAGIC, PARAMS_DTYPE, PARAMS_OFFSET, POSE_OFFSET, VOXEL_RESET, reset_entry  # noqa: F401

VERSION = 2
HEADER_BYTES = 304
CACHE_BLOCKS_OFFSET, CRC_OFFSET, RECORDS_CRC_OFFSET = 288, 296, 300
RECORD_DTYPE = np.dtype([("index", "<u4"), ("entry", HASH_DTYPE), ("visType", "u1"), ("swapState", "u1"), ("hasStoredData", "u1"),
                         ("pad", "u1")])
assert RECORD_DTYPE.itemsize == 24


def swapping(state):
    return int(state["params"]["use_swapping"]) != 0


def file_size(params, counters, n_records, n_blocks_stored, n_cache_blocks=0):
    """304 + 24 R + 2048 (b + s) + 4 (V + A + E) + M for a swapping context; version 1's otherwise."""
    if not params["use_swapping"]:
        assert n_cache_blocks == 0
        return R.file_size(params, counters, n_records, n_blocks_stored)
    assert not params["voxel_rgb"]
    cols, rows = int(params["cols"]), int(params["rows"])
    maps = sum(2 * 16 * (cols >> l) * (rows >> l) for l in range(LEVELS))
    return (HEADER_BYTES + 24 * n_records + BLOCK_BYTES * (n_blocks_stored + n_cache_blocks) +
            4 * (counters["noVisibleEntries"] + counters["lastFreeBlockId"] + 1 + counters["lastFreeExcessListId"] + 1) + maps)


def records_of(state):
    """Ascending by entry index: entries whose HashEntry is not ResetScene's or whose visType, swapState or
    hasStoredData is non-zero."""
    if not swapping(state):
        return R.records_of(state)
    h = np.ascontiguousarray(state["hash"])
    differs = (h.view(np.uint8).reshape(-1, 16) != np.frombuffer(reset_entry().tobytes(), np.uint8)).any(axis=1)
    vis, st, fl = (np.asarray(state[k], np.uint8) for k in ("visType", "swapState", "swapFlags"))
    idx = np.flatnonzero(differs | (vis != 0) | (st != 0) | (fl != 0))
    rec = np.zeros(len(idx), RECORD_DTYPE)
    rec["index"] = idx
    rec["entry"] = h[idx]
    rec["visType"], rec["swapState"], rec["hasStoredData"] = vis[idx], st[idx], fl[idx]
    return rec


def pack(state):
    if not swapping(state):
        return R.pack(state)
    p, c = state["params"], state["counters"]
    assert int(p["use_swapping"]) == 1 and not p["voxel_rgb"]
    rec = records_of(state)
    ptrs = rec["entry"]["ptr"][rec["entry"]["ptr"] >= 0].astype(np.int64)
    cached = rec["index"][rec["hasStoredData"] == 1].astype(np.int64)
    size = file_size(p, c, len(rec), len(ptrs), len(cached))
    hdr = bytearray(HEADER_BYTES)
    hdr[0:8] = MAGIC
    struct.pack_into("<II", hdr, 8, VERSION, PARAMS_DTYPE.itemsize)
    hdr[PARAMS_OFFSET:PARAMS_OFFSET + 180] = np.asarray(p, PARAMS_DTYPE).tobytes()
    struct.pack_into("<5i", hdr, 196, state["pose_algebra"], c["frame_counter"], c["lastFreeBlockId"], c["lastFreeExcessListId"],
                     c["noVisibleEntries"])
    struct.pack_into("<3q", hdr, 216, len(rec), len(ptrs), size)
    hdr[POSE_OFFSET:POSE_OFFSET + 48] = np.asarray(state["pose"], "<f4").reshape(12).tobytes()
    struct.pack_into("<q", hdr, CACHE_BLOCKS_OFFSET, len(cached))
    struct.pack_into("<II", hdr, CRC_OFFSET, zlib.crc32(bytes(hdr[:CRC_OFFSET])), zlib.crc32(rec.tobytes()))
    out = [bytes(hdr), rec.tobytes()]
    out.append(np.asarray(state["vba"], "<u4").reshape(-1, 512)[ptrs].tobytes())
    out.append(np.asarray(state["store"], "<u4").reshape(-1, 512)[cached].tobytes())
    out.append(np.asarray(state["visibleIds"], "<i4")[:c["noVisibleEntries"]].tobytes())
    out.append(np.asarray(state["allocList"], "<i4")[:c["lastFreeBlockId"] + 1].tobytes())
    out.append(np.asarray(state["excessList"], "<i4")[:c["lastFreeExcessListId"] + 1].tobytes())
    for m in state["maps"]:
        out.append(np.ascontiguousarray(m, "<f4").tobytes())
    data = b"".join(out)
    assert len(data) == size
    return data


def unpack(data, store=None):
    """The state of the file.  Version 2: `store` is what the loading context's store held before (blocks the
    file does not flag stay as they are); None stands for a zeroed one."""
    assert data[:8] == MAGIC
    version, params_bytes = struct.unpack_from("<II", data, 8)
    if version == R.VERSION:
        return R.unpack(data)
    assert version == VERSION and params_bytes == PARAMS_DTYPE.itemsize
    assert struct.unpack_from("<I", data, CRC_OFFSET)[0] == zlib.crc32(data[:CRC_OFFSET])
    p = np.frombuffer(data, PARAMS_DTYPE, 1, PARAMS_OFFSET)[0].copy()
    assert int(p["use_swapping"]) == 1 and int(p["voxel_rgb"]) == 0
    alg, fc, lfb, lfe, nvis = struct.unpack_from("<5i", data, 196)
    n_records, n_stored, file_bytes = struct.unpack_from("<3q", data, 216)
    n_cache = struct.unpack_from("<q", data, CACHE_BLOCKS_OFFSET)[0]
    counters = dict(lastFreeBlockId=lfb, lastFreeExcessListId=lfe, noVisibleEntries=nvis, frame_counter=fc)
    assert file_bytes == len(data) == file_size(p, counters, n_records, n_stored, n_cache)
    n_total, n_blocks, n_excess = int(p["n_buckets"]) + int(p["n_excess"]), int(p["n_blocks"]), int(p["n_excess"])
    o = HEADER_BYTES
    assert struct.unpack_from("<I", data, RECORDS_CRC_OFFSET)[0] == zlib.crc32(data[o:o + 24 * n_records])
    rec = np.frombuffer(data, RECORD_DTYPE, n_records, o)
    o += 24 * n_records
    assert not rec["pad"].any() and (rec["swapState"] <= 2).all() and (rec["hasStoredData"] <= 1).all()
    hash_ = np.full(n_total, reset_entry(), HASH_DTYPE)
    vis, st, fl = (np.zeros(n_total, np.uint8) for _ in range(3))
    hash_[rec["index"]] = rec["entry"]
    vis[rec["index"]], st[rec["index"]], fl[rec["index"]] = rec["visType"], rec["swapState"], rec["hasStoredData"]
    ptrs = rec["entry"]["ptr"][rec["entry"]["ptr"] >= 0].astype(np.int64)
    cached = rec["index"][rec["hasStoredData"] == 1].astype(np.int64)
    assert len(ptrs) == n_stored and len(cached) == n_cache
    vba = np.full((n_blocks, 512), VOXEL_RESET, np.uint32)
    vba[ptrs] = np.frombuffer(data, "<u4", n_stored * 512, o).reshape(n_stored, 512)
    o += BLOCK_BYTES * n_stored
    sto = np.zeros((n_total, 512), np.uint32) if store is None else np.array(store, np.uint32).reshape(n_total, 512)
    sto[cached] = np.frombuffer(data, "<u4", n_cache * 512, o).reshape(n_cache, 512)
    o += BLOCK_BYTES * n_cache
    visible = np.frombuffer(data, "<i4", nvis, o).copy()
    o += 4 * nvis
    alloc = np.arange(n_blocks, dtype=np.int32)
    alloc[:lfb + 1] = np.frombuffer(data, "<i4", lfb + 1, o)
    o += 4 * (lfb + 1)
    excess = np.arange(n_excess, dtype=np.int32)
    excess[:lfe + 1] = np.frombuffer(data, "<i4", lfe + 1, o)
    o += 4 * (lfe + 1)
    maps = []
    for l in range(LEVELS):
        h, w = int(p["rows"]) >> l, int(p["cols"]) >> l
        for _ in range(2):
            maps.append(np.frombuffer(data, "<f4", h * w * 4, o).reshape(h, w, 4).copy())
            o += 16 * h * w
    assert o == len(data)
    return dict(params=p, pose_algebra=alg, counters=counters, pose=np.frombuffer(data, "<f4", 12, POSE_OFFSET).copy(),
                hash=hash_, visType=vis, vba=vba.reshape(-1), rgb=None, visibleIds=visible, allocList=alloc, excessList=excess,
                maps=maps, swapState=st, swapFlags=fl, store=sto.reshape(-1))


def states_equal(a, b):
    """Bit for bit; of a swapping state the store only where the flag is 1 and allocList only in [0, lastFreeBlockId]."""
    if swapping(a) != swapping(b):
        return False
    if not swapping(a):
        return R.states_equal(a, b)
    if a["counters"] != b["counters"]:
        return False
    live = a["counters"]["lastFreeBlockId"] + 1
    ident = np.arange(len(a["allocList"]), dtype=np.int32)

    def live_only(s):
        return dict(s, allocList=np.concatenate([np.asarray(s["allocList"], np.int32)[:live], ident[live:]]))
    if len(a["allocList"]) != len(b["allocList"]) or not R.states_equal(live_only(a), live_only(b)):
        return False
    for k in ("swapState", "swapFlags"):
        if np.asarray(a[k], np.uint8).tobytes() != np.asarray(b[k], np.uint8).tobytes():
            return False
    ids = np.flatnonzero(np.asarray(a["swapFlags"]) == 1)
    sa, sb = (np.asarray(s[("store")]).view(np.uint32).reshape(-1, 512)[ids] for s in (a, b))
    return sa.tobytes() == sb.tobytes()


def tiny_state(seed=3, **kw):
    """scene_ckpt_ref.tiny_state as a swapping context's (n_blocks = 4), with one entry of every kind of cache
    record: stored only (ptr -1, flag 1), pending (ptr >= 0, flag 1, state 1), merged (state 2, its store
    stale), a flagged entry whose hash entry is ResetScene's, and an entry with only a swap state."""
    kw.setdefault("n_blocks", 4)
    s = R.tiny_state(seed=seed, voxel_rgb=0, **kw)
    rng = np.random.default_rng(seed + 100)
    s["params"]["use_swapping"] = 1
    s["params"]["swap_transfer_blocks"] = 2
    nb = int(s["params"]["n_buckets"])
    n_total = nb + int(s["params"]["n_excess"])
    h = s["hash"]
    st, fl = np.zeros(n_total, np.uint8), np.zeros(n_total, np.uint8)
    fl[9] = 1                                            # R.tiny_state's entry 9 has ptr -1: stored only
    fl[3], st[3] = 1, 1                                  # entry 3 holds block 1: pending
    h[11] = (2, 2, 2, 0, 0, 3)
    fl[11], st[11] = 1, 2                                # merged
    fl[13] = 1                                           # no hash entry left, a stored block
    st[14] = 1                                           # only a swap state
    st[nb + 2] = 2                                       # the excess entry: active, never stored
    s["swapState"], s["swapFlags"] = st, fl
    s["store"] = rng.integers(0, 1 << 24, n_total * 512, dtype=np.uint32)
    # blocks 0, 1, 3 are held; block 2 is free (at Voxel_s(): what no entry holds is not part of the state), and so
    # is every block past 3 of a larger VBA
    free = np.setdiff1d(np.arange(int(s["params"]["n_blocks"])), [0, 1, 3])
    s["vba"].reshape(-1, 512)[free] = VOXEL_RESET
    s["counters"]["lastFreeBlockId"] = 0
    s["allocList"][0] = 2
    return s
