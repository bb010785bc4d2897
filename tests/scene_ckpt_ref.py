"""Numpy restatement of the scene checkpoint file (DESIGN.md §5 Scene checkpoints; the library's side is
topfusion_amd/csrc/tf_scene_file.h).  pack(state) -> bytes and unpack(bytes) -> state, from plain arrays.

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
"""
import struct
import zlib

import numpy as np

HASH_DTYPE = np.dtype([("x", "<i2"), ("y", "<i2"), ("z", "<i2"), ("pad", "<i2"), ("offset", "<i4"), ("ptr", "<i4")])
PARAMS_DTYPE = np.dtype([
    ("cols", "<i4"), ("rows", "<i4"), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
    ("bilateral_sigma_depth", "<f4"), ("bilateral_sigma_spatial", "<f4"), ("bilateral_kernel_size", "<i4"),
    ("icp_truncate_depth_dist", "<f4"), ("icp_dist_thres", "<f4"), ("icp_angle_thres", "<f4"), ("icp_iter_num", "<i4", (4,)),
    ("mu", "<f4"), ("maxW", "<i4"), ("voxelSize", "<f4"), ("viewFrustum_min", "<f4"), ("viewFrustum_max", "<f4"),
    ("n_buckets", "<i4"), ("n_excess", "<i4"), ("n_blocks", "<i4"), ("vis_capacity", "<i4"), ("max_render_blocks", "<i4"),
    ("use_swapping", "<i4"), ("swap_transfer_blocks", "<i4"), ("voxel_rgb", "<i4"), ("rgb_intr", "<f4", (4,)),
    ("depth_to_rgb", "<f4", (12,))])
RECORD_DTYPE = np.dtype([("index", "<u4"), ("entry", HASH_DTYPE), ("visType", "u1"), ("pad", "u1", (3,))])
assert PARAMS_DTYPE.itemsize == 180 and RECORD_DTYPE.itemsize == 24 and HASH_DTYPE.itemsize == 16

MAGIC = b"TFSCENE\0"
VERSION = 1
HEADER_BYTES = 296
BLOCK_BYTES = 2048
VOXEL_RESET = 0x00007FFF            # Voxel_s(): sdf 32767, w 0
LEVELS = 3
# header offsets: name -> (offset, struct format)
HEADER_FIELDS = {"version": (8, "<I"), "params_bytes": (12, "<I"), "pose_algebra": (196, "<i"), "frame_counter": (200, "<i"),
                 "lastFreeBlockId": (204, "<i"), "lastFreeExcessListId": (208, "<i"), "noVisibleEntries": (212, "<i"),
                 "n_records": (216, "<q"), "n_blocks_stored": (224, "<q"), "file_bytes": (232, "<q"), "crc": (288, "<I"), "records_crc": (292, "<I")}
PARAMS_OFFSET, POSE_OFFSET, CRC_OFFSET, RECORDS_CRC_OFFSET = 16, 240, 288, 292


def params_record(p):
    """A ctypes tf_params (topfusion_amd.TfParams) or 180 bytes as a PARAMS_DTYPE record."""
    return np.frombuffer(bytes(p), PARAMS_DTYPE)[0].copy()


def reset_entry():
    e = np.zeros((), HASH_DTYPE)
    e["ptr"] = -2
    return e


def file_size(params, counters, n_records, n_blocks_stored):
    """The size formula: a pure function of the counts."""
    cols, rows = int(params["cols"]), int(params["rows"])
    maps = sum(2 * 16 * (cols >> l) * (rows >> l) for l in range(LEVELS))
    return (HEADER_BYTES + 24 * n_records + BLOCK_BYTES * (2 if params["voxel_rgb"] else 1) * n_blocks_stored +
            4 * counters["noVisibleEntries"] + 4 * (counters["lastFreeBlockId"] + 1) +
            4 * (counters["lastFreeExcessListId"] + 1) + maps)


def records_of(state):
    """The entry records, ascending by entry index: entries whose HashEntry is not ResetScene's or whose
    visType is non-zero."""
    h = np.ascontiguousarray(state["hash"])
    differs = (h.view(np.uint8).reshape(-1, 16) != np.frombuffer(reset_entry().tobytes(), np.uint8)).any(axis=1)
    idx = np.flatnonzero(differs | (np.asarray(state["visType"]) != 0))
    rec = np.zeros(len(idx), RECORD_DTYPE)
    rec["index"] = idx
    rec["entry"] = h[idx]
    rec["visType"] = np.asarray(state["visType"])[idx]
    return rec


def header(state, n_records, n_blocks_stored, records_crc):
    c = state["counters"]
    hdr = bytearray(HEADER_BYTES)
    hdr[0:8] = MAGIC
    struct.pack_into("<II", hdr, 8, VERSION, PARAMS_DTYPE.itemsize)
    hdr[PARAMS_OFFSET:PARAMS_OFFSET + 180] = np.asarray(state["params"], PARAMS_DTYPE).tobytes()
    struct.pack_into("<5i", hdr, 196, state["pose_algebra"], c["frame_counter"], c["lastFreeBlockId"],
                     c["lastFreeExcessListId"], c["noVisibleEntries"])
    struct.pack_into("<3q", hdr, 216, n_records, n_blocks_stored, file_size(state["params"], c, n_records, n_blocks_stored))
    hdr[POSE_OFFSET:POSE_OFFSET + 48] = np.asarray(state["pose"], "<f4").reshape(12).tobytes()
    struct.pack_into("<II", hdr, CRC_OFFSET, zlib.crc32(bytes(hdr[:CRC_OFFSET])), records_crc)
    return bytes(hdr)


def pack(state):
    p, c = state["params"], state["counters"]
    rec = records_of(state)
    ptrs = rec["entry"]["ptr"][rec["entry"]["ptr"] >= 0].astype(np.int64)
    out = [header(state, len(rec), len(ptrs), zlib.crc32(rec.tobytes())), rec.tobytes()]
    vba = np.asarray(state["vba"], "<u4").reshape(-1, 512)
    if p["voxel_rgb"]:
        rgb = np.asarray(state["rgb"], "<u4").reshape(-1, 512)
        out.append(np.concatenate([vba[ptrs], rgb[ptrs]], axis=1).tobytes())
    else:
        out.append(vba[ptrs].tobytes())
    out.append(np.asarray(state["visibleIds"], "<i4")[:c["noVisibleEntries"]].tobytes())
    out.append(np.asarray(state["allocList"], "<i4")[:c["lastFreeBlockId"] + 1].tobytes())
    out.append(np.asarray(state["excessList"], "<i4")[:c["lastFreeExcessListId"] + 1].tobytes())
    for m in state["maps"]:
        out.append(np.ascontiguousarray(m, "<f4").tobytes())
    data = b"".join(out)
    assert len(data) == file_size(p, c, len(rec), len(ptrs))
    return data


def unpack(data):
    assert data[:8] == MAGIC
    version, params_bytes = struct.unpack_from("<II", data, 8)
    assert version == VERSION and params_bytes == PARAMS_DTYPE.itemsize
    assert struct.unpack_from("<I", data, CRC_OFFSET)[0] == zlib.crc32(data[:CRC_OFFSET])
    p = np.frombuffer(data, PARAMS_DTYPE, 1, PARAMS_OFFSET)[0].copy()
    alg, fc, lfb, lfe, nvis = struct.unpack_from("<5i", data, 196)
    n_records, n_stored, file_bytes = struct.unpack_from("<3q", data, 216)
    assert file_bytes == len(data)
    counters = dict(lastFreeBlockId=lfb, lastFreeExcessListId=lfe, noVisibleEntries=nvis, frame_counter=fc)
    assert file_bytes == file_size(p, counters, n_records, n_stored)
    n_total, n_blocks, n_excess = int(p["n_buckets"]) + int(p["n_excess"]), int(p["n_blocks"]), int(p["n_excess"])
    o = HEADER_BYTES
    assert struct.unpack_from("<I", data, RECORDS_CRC_OFFSET)[0] == zlib.crc32(data[o:o + 24 * n_records])
    rec = np.frombuffer(data, RECORD_DTYPE, n_records, o)
    o += 24 * n_records
    hash_ = np.full(n_total, reset_entry(), HASH_DTYPE)
    vis = np.zeros(n_total, np.uint8)
    hash_[rec["index"]] = rec["entry"]
    vis[rec["index"]] = rec["visType"]
    ptrs = rec["entry"]["ptr"][rec["entry"]["ptr"] >= 0].astype(np.int64)
    assert len(ptrs) == n_stored
    per = 1024 if p["voxel_rgb"] else 512
    blocks = np.frombuffer(data, "<u4", n_stored * per, o).reshape(n_stored, per)
    o += 4 * n_stored * per
    vba = np.full((n_blocks, 512), VOXEL_RESET, np.uint32)
    vba[ptrs] = blocks[:, :512]
    rgb = None
    if p["voxel_rgb"]:
        rgb = np.zeros((n_blocks, 512), np.uint32)
        rgb[ptrs] = blocks[:, 512:]
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
                hash=hash_, visType=vis, vba=vba.reshape(-1), rgb=None if rgb is None else rgb.reshape(-1),
                visibleIds=visible, allocList=alloc, excessList=excess, maps=maps)


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
