"""Numpy restatement of the checkpoint file, both versions (DESIGN.md §5 Scene checkpoints, Map checkpoints; the
library's side is topfusion_amd/csrc/tf_scene_file.h).  layout() is the file; pack(state) -> bytes and
unpack(bytes) -> state, from plain arrays, write and slice by it.

A state is a dict:
    params        0-d record of PARAMS_DTYPE (tf_params)
    pose_algebra  int
    counters      dict: lastFreeBlockId, lastFreeExcessListId, noVisibleEntries, frame_counter
    pose          float32[12]
    hash          HASH_DTYPE[n_buckets + n_excess]
    visType       uint8[n_buckets + n_excess]
    vba           uint32[n_blocks * 512]   (a voxel's sdf | w << 16 | pad << 24)
    rgb           uint32[n_blocks * 512] with voxel_rgb, else None
    visibleIds    int32[noVisibleEntries]
    allocList     int32[n_blocks]; the file holds [0, lastFreeBlockId], the rest is the identity
    excessList    int32[n_excess]; likewise with lastFreeExcessListId
    maps          six float32 (h, w, 4) arrays: previous points, normals of level 0, 1, 2
and, where params["use_swapping"] is set (version 2), what tests/scene_map_ref.py describes: swapState, swapFlags, store.
"""
import struct
import zlib

import numpy as np

from vbh_ref import HASH_DTYPE, VOXEL_RESET, reset_entry  # noqa: F401

PARAMS_DTYPE = np.dtype([
    ("cols", "<i4"), ("rows", "<i4"), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
    ("bilateral_sigma_depth", "<f4"), ("bilateral_sigma_spatial", "<f4"), ("bilateral_kernel_size", "<i4"),
    ("icp_truncate_depth_dist", "<f4"), ("icp_dist_thres", "<f4"), ("icp_angle_thres", "<f4"), ("icp_iter_num", "<i4", (4,)),
    ("mu", "<f4"), ("maxW", "<i4"), ("voxelSize", "<f4"), ("viewFrustum_min", "<f4"), ("viewFrustum_max", "<f4"),
    ("n_buckets", "<i4"), ("n_excess", "<i4"), ("n_blocks", "<i4"), ("vis_capacity", "<i4"), ("max_render_blocks", "<i4"),
    ("use_swapping", "<i4"), ("swap_transfer_blocks", "<i4"), ("voxel_rgb", "<i4"), ("rgb_intr", "<f4", (4,)),
    ("depth_to_rgb", "<f4", (12,))])
# version 1's record is this one with swapState and hasStoredData zero
RECORD_DTYPE = np.dtype([("index", "<u4"), ("entry", HASH_DTYPE), ("visType", "u1"), ("swapState", "u1"), ("hasStoredData", "u1"),
                         ("pad", "u1")])
assert PARAMS_DTYPE.itemsize == 180 and RECORD_DTYPE.itemsize == 24 and HASH_DTYPE.itemsize == 16

MAGIC = b"TFSCENE\0"
# the header: magic, version and params_bytes (<II at 8), params (16), pose_algebra, frame_counter, lastFreeBlockId,
# lastFreeExcessListId, noVisibleEntries (<5i at 196), n_records, n_blocks_stored, file_bytes (<3q at 216), pose (240),
# in version 2 n_cache_blocks (<q at 288), and as its last eight bytes the CRC32 of what precedes them and the records'
HEADER_BYTES_OF = {1: 296, 2: 304}
VERSION, HEADER_BYTES = 1, HEADER_BYTES_OF[1]
PARAMS_OFFSET, POSE_OFFSET, CACHE_BLOCKS_OFFSET = 16, 240, 288
BLOCK_BYTES = 2048
LEVELS = 3


def params_record(p):
    """A ctypes tf_params (topfusion_amd.TfParams) or 180 bytes as a PARAMS_DTYPE record."""
    return np.frombuffer(bytes(p), PARAMS_DTYPE)[0].copy()


def swapping(state):
    return int(state["params"]["use_swapping"]) != 0


def layout(params, counters, n_records, n_blocks_stored, n_cache_blocks=0):
    """(version, the sections in file order as (name, offset, bytes), total bytes): a pure function of the counts.
    Version 2 is the file of a swapping context, as in tf_map_layout."""
    version = 2 if params["use_swapping"] else 1
    assert n_cache_blocks == 0 if version == 1 else not params["voxel_rgb"]
    cols, rows = int(params["cols"]), int(params["rows"])
    sizes = [("header", HEADER_BYTES_OF[version]), ("records", 24 * n_records),
             ("active_blocks", BLOCK_BYTES * (2 if params["voxel_rgb"] else 1) * n_blocks_stored)]
    if version == 2:
        sizes.append(("stored_blocks", BLOCK_BYTES * n_cache_blocks))
    sizes += [("visibleIds", 4 * counters["noVisibleEntries"]), ("allocList", 4 * (counters["lastFreeBlockId"] + 1)),
              ("excessList", 4 * (counters["lastFreeExcessListId"] + 1))]
    sizes += [(f"map{k}", 16 * (cols >> k // 2) * (rows >> k // 2)) for k in range(2 * LEVELS)]
    offsets = np.cumsum([0] + [n for _, n in sizes]).tolist()
    return version, [(name, o, n) for (name, n), o in zip(sizes, offsets)], offsets[-1]


def file_size(params, counters, n_records, n_blocks_stored, n_cache_blocks=0):
    return layout(params, counters, n_records, n_blocks_stored, n_cache_blocks)[2]


def records_of(state):
    """The entry records, ascending by entry index: entries whose HashEntry is not ResetScene's or whose visType --
    of a swapping state also swapState or hasStoredData -- is non-zero."""
    h = np.ascontiguousarray(state["hash"])
    vis = np.asarray(state["visType"], np.uint8)
    keep = (h.view(np.uint8).reshape(-1, 16) != np.frombuffer(reset_entry().tobytes(), np.uint8)).any(axis=1) | (vis != 0)
    if swapping(state):
        st, fl = np.asarray(state["swapState"], np.uint8), np.asarray(state["swapFlags"], np.uint8)
        keep |= (st != 0) | (fl != 0)
    idx = np.flatnonzero(keep)
    rec = np.zeros(len(idx), RECORD_DTYPE)
    rec["index"], rec["entry"], rec["visType"] = idx, h[idx], vis[idx]
    if swapping(state):
        rec["swapState"], rec["hasStoredData"] = st[idx], fl[idx]
    return rec


def _payload(rec):
    """(the VBA blocks, the store's entries) whose voxels follow the records, in record order."""
    return rec["entry"]["ptr"][rec["entry"]["ptr"] >= 0].astype(np.int64), rec["index"][rec["hasStoredData"] == 1].astype(np.int64)


def header(state, version, n_records, n_blocks_stored, n_cache_blocks, file_bytes, records_crc):
    c = state["counters"]
    hdr = bytearray(HEADER_BYTES_OF[version])
    hdr[0:8] = MAGIC
    struct.pack_into("<II", hdr, 8, version, PARAMS_DTYPE.itemsize)
    hdr[PARAMS_OFFSET:PARAMS_OFFSET + 180] = np.asarray(state["params"], PARAMS_DTYPE).tobytes()
    struct.pack_into("<5i", hdr, 196, state["pose_algebra"], c["frame_counter"], c["lastFreeBlockId"],
                     c["lastFreeExcessListId"], c["noVisibleEntries"])
    struct.pack_into("<3q", hdr, 216, n_records, n_blocks_stored, file_bytes)
    hdr[POSE_OFFSET:POSE_OFFSET + 48] = np.asarray(state["pose"], "<f4").reshape(12).tobytes()
    if version == 2:
        struct.pack_into("<q", hdr, CACHE_BLOCKS_OFFSET, n_cache_blocks)
    struct.pack_into("<II", hdr, len(hdr) - 8, zlib.crc32(bytes(hdr[:-8])), records_crc)
    return bytes(hdr)


def pack(state):
    p, c = state["params"], state["counters"]
    rec = records_of(state)
    ptrs, cached = _payload(rec)
    version, sections, total = layout(p, c, len(rec), len(ptrs), len(cached))
    blocks = np.asarray(state["vba"], "<u4").reshape(-1, 512)[ptrs]
    if p["voxel_rgb"]:
        blocks = np.concatenate([blocks, np.asarray(state["rgb"], "<u4").reshape(-1, 512)[ptrs]], axis=1)
    part = dict(header=header(state, version, len(rec), len(ptrs), len(cached), total, zlib.crc32(rec.tobytes())),
                records=rec, active_blocks=blocks,
                visibleIds=np.asarray(state["visibleIds"], "<i4")[:c["noVisibleEntries"]],
                allocList=np.asarray(state["allocList"], "<i4")[:c["lastFreeBlockId"] + 1],
                excessList=np.asarray(state["excessList"], "<i4")[:c["lastFreeExcessListId"] + 1])
    if version == 2:
        part["stored_blocks"] = np.asarray(state["store"], "<u4").reshape(-1, 512)[cached]
    part.update((f"map{k}", np.ascontiguousarray(m, "<f4")) for k, m in enumerate(state["maps"]))
    out = [part[name] if name == "header" else part[name].tobytes() for name, _, _ in sections]
    assert [len(b) for b in out] == [n for _, _, n in sections]
    return b"".join(out)


def unpack(data, store=None):
    """The state of the file.  Version 2: `store` is what the loading context's store held before (blocks the
    file does not flag stay as they are); None stands for a zeroed one."""
    assert data[:8] == MAGIC
    version, params_bytes = struct.unpack_from("<II", data, 8)
    assert version in HEADER_BYTES_OF and params_bytes == PARAMS_DTYPE.itemsize
    crc_at = HEADER_BYTES_OF[version] - 8
    crc, records_crc = struct.unpack_from("<II", data, crc_at)
    assert crc == zlib.crc32(data[:crc_at])
    p = np.frombuffer(data, PARAMS_DTYPE, 1, PARAMS_OFFSET)[0].copy()
    alg, fc, lfb, lfe, nvis = struct.unpack_from("<5i", data, 196)
    n_records, n_stored, file_bytes = struct.unpack_from("<3q", data, 216)
    n_cache = struct.unpack_from("<q", data, CACHE_BLOCKS_OFFSET)[0] if version == 2 else 0
    counters = dict(lastFreeBlockId=lfb, lastFreeExcessListId=lfe, noVisibleEntries=nvis, frame_counter=fc)
    assert version == 1 or int(p["use_swapping"]) == 1
    lay_version, sections, total = layout(p, counters, n_records, n_stored, n_cache)
    assert lay_version == version and file_bytes == len(data) == total
    at = {name: (o, n) for name, o, n in sections}

    def take(name, dtype):
        o, n = at[name]
        return np.frombuffer(data, dtype, n // np.dtype(dtype).itemsize, o)

    rec = take("records", RECORD_DTYPE)
    assert records_crc == zlib.crc32(rec.tobytes())
    assert not rec["pad"].any() and (rec["swapState"] <= 2).all() and (rec["hasStoredData"] <= 1).all()
    assert version == 2 or not (rec["swapState"].any() or rec["hasStoredData"].any())
    n_total, n_blocks, n_excess = int(p["n_buckets"]) + int(p["n_excess"]), int(p["n_blocks"]), int(p["n_excess"])
    hash_ = np.full(n_total, reset_entry(), HASH_DTYPE)
    vis, st, fl = (np.zeros(n_total, np.uint8) for _ in range(3))
    hash_[rec["index"]] = rec["entry"]
    vis[rec["index"]], st[rec["index"]], fl[rec["index"]] = rec["visType"], rec["swapState"], rec["hasStoredData"]
    ptrs, cached = _payload(rec)
    assert len(ptrs) == n_stored and len(cached) == n_cache
    blocks = take("active_blocks", "<u4").reshape(n_stored, 1024 if p["voxel_rgb"] else 512)
    vba = np.full((n_blocks, 512), VOXEL_RESET, np.uint32)
    vba[ptrs] = blocks[:, :512]
    rgb = None
    if p["voxel_rgb"]:
        rgb = np.zeros((n_blocks, 512), np.uint32)
        rgb[ptrs] = blocks[:, 512:]
    alloc, excess = np.arange(n_blocks, dtype=np.int32), np.arange(n_excess, dtype=np.int32)
    alloc[:lfb + 1] = take("allocList", "<i4")
    excess[:lfe + 1] = take("excessList", "<i4")
    maps = [take(f"map{k}", "<f4").reshape(int(p["rows"]) >> k // 2, int(p["cols"]) >> k // 2, 4).copy() for k in range(2 * LEVELS)]
    out = dict(params=p, pose_algebra=alg, counters=counters, pose=np.frombuffer(data, "<f4", 12, POSE_OFFSET).copy(),
               hash=hash_, visType=vis, vba=vba.reshape(-1), rgb=None if rgb is None else rgb.reshape(-1),
               visibleIds=take("visibleIds", "<i4").copy(), allocList=alloc, excessList=excess, maps=maps)
    if version == 2:
        sto = np.zeros((n_total, 512), np.uint32) if store is None else np.array(store, np.uint32).reshape(n_total, 512)
        sto[cached] = take("stored_blocks", "<u4").reshape(n_cache, 512)
        out.update(swapState=st, swapFlags=fl, store=sto.reshape(-1))
    return out


def states_equal(a, b):
    """Bit for bit."""
    def same(x, y):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        return x.shape == y.shape and x.tobytes() == y.tobytes()
    if a["counters"] != b["counters"] or a["pose_algebra"] != b["pose_algebra"]:
        return False
    if np.asarray(a["params"], PARAMS_DTYPE).tobytes() != np.asarray(b["params"], PARAMS_DTYPE).tobytes():
        return False
    if (a["rgb"] is None) != (b["rgb"] is None) or (a["rgb"] is not None and not same(a["rgb"], b["rgb"])):
        return False
    n = a["counters"]["noVisibleEntries"]
    if not same(np.asarray(a["visibleIds"])[:n], np.asarray(b["visibleIds"])[:n]):
        return False
    if len(a["maps"]) != len(b["maps"]) or not all(same(np.asarray(x, np.float32), np.asarray(y, np.float32)) for x, y in zip(a["maps"], b["maps"])):
        return False
    return all(same(a[k], b[k]) for k in ("pose", "hash", "visType", "vba", "allocList", "excessList"))


def tiny_state(cols=16, rows=12, n_buckets=16, n_excess=16, n_blocks=2, voxel_rgb=0, seed=3):
    """A small valid state from a seeded generator: every block in use, one excess chain, one entry
    with only visType set, non-identity live list parts."""
    rng = np.random.default_rng(seed)
    p = np.zeros((), PARAMS_DTYPE)
    p["cols"], p["rows"] = cols, rows
    p["fx"] = p["fy"] = 20.0
    p["cx"], p["cy"] = cols / 2, rows / 2
    p["mu"], p["maxW"], p["voxelSize"] = 0.02, 100, 0.005
    p["n_buckets"], p["n_excess"], p["n_blocks"] = n_buckets, n_excess, n_blocks
    p["vis_capacity"], p["max_render_blocks"] = 64, 64
    p["voxel_rgb"] = voxel_rgb
    p["bilateral_kernel_size"] = 7
    n_total = n_buckets + n_excess
    hash_ = np.full(n_total, reset_entry(), HASH_DTYPE)
    vis = np.zeros(n_total, np.uint8)
    # block 1 in bucket 3 with a chain into excess slot 2 (entry n_buckets + 2), which holds block 0
    hash_[3] = (1, -2, 3, 0, 3, 1)
    hash_[n_buckets + 2] = (4, 5, -6, 0, 0, 0)
    vis[3] = 1
    vis[7] = 2                                           # only visType
    hash_[9] = (7, 7, 7, 0, 0, -1)                       # an entry without a block (ptr < 0)
    vba = rng.integers(0, 1 << 24, n_blocks * 512, dtype=np.uint32)
    rgb = rng.integers(0, 1 << 32, n_blocks * 512, dtype=np.uint32) if voxel_rgb else None
    alloc = np.arange(n_blocks, dtype=np.int32)
    excess = np.arange(n_excess, dtype=np.int32)
    excess[:5] = [4, 0, 1, 3, 6]
    counters = dict(lastFreeBlockId=-1, lastFreeExcessListId=4, noVisibleEntries=2, frame_counter=5)
    maps = []
    for l in range(LEVELS):
        for _ in range(2):
            maps.append(rng.standard_normal((rows >> l, cols >> l, 4)).astype(np.float32))
    pose = np.eye(4, dtype=np.float32)[:3].reshape(12).copy()
    pose[3] = 0.25
    return dict(params=p, pose_algebra=4, counters=counters, pose=pose, hash=hash_, visType=vis, vba=vba, rgb=rgb,
                visibleIds=np.array([3, n_buckets + 2], np.int32), allocList=alloc, excessList=excess, maps=maps)
