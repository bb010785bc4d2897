"""What is specific to a swapping state of the checkpoint file restated in tests/scene_ckpt_ref.py (DESIGN.md §5 Map
checkpoints): version 2 is the file of a swapping context.

A swapping state is scene_ckpt_ref's state dict (params["use_swapping"] == 1, rgb None) plus
    swapState     uint8[n_total]          HashSwapState::state per entry (0, 1, 2)
    swapFlags     uint8[n_total]          hasStoredData per entry (0, 1)
    store         uint32[n_total * 512]   the GlobalCache's block per entry; state only where the flag is 1

and allocList is state only in [0, lastFreeBlockId]: SaveToGlobalMemory pushes freed blocks back, so what a sequence
leaves above the top is stale (allocation and reallocation read at or below it, and every reset of a swapping context
is a full one, which rewrites the list); a load leaves the identity there.

pack / unpack / file_size / records_of are scene_ckpt_ref's, which follow params["use_swapping"]."""
import numpy as np

import scene_ckpt_ref as R
from scene_ckpt_ref import CACHE_BLOCKS_OFFSET, RECORD_DTYPE, VOXEL_RESET, file_size, pack, records_of, swapping, unpack  # noqa: F401

VERSION = 2
HEADER_BYTES = R.HEADER_BYTES_OF[VERSION]
CRC_OFFSET, RECORDS_CRC_OFFSET = HEADER_BYTES - 8, HEADER_BYTES - 4
assert (HEADER_BYTES, CACHE_BLOCKS_OFFSET, CRC_OFFSET, RECORDS_CRC_OFFSET) == (304, 288, 296, 300)


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
