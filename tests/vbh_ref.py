"""The reference's voxel block hash in numpy, once: the entry and voxel layouts, hashIndex, the bucket-then-excess
chain, and the rules the reference walks it by.  Every tests/*_ref.py and *_cases.py takes these from here and says
which rule it uses; tests/test_vbh_ref.py holds them to the oracle.  numpy only: neither topfusion_amd nor oracle.

A table is HASH_DTYPE[n_buckets + n_excess]: bucket i of hashIndex, then the excess entries; `offset` is the next
entry's excess slot + 1 (entry n_buckets + offset - 1), below 1 at a chain's end; `ptr` is the entry's voxel block,
-1 for a position without one (swapped out) and -2 for a free entry."""
import numpy as np

HASH_DTYPE = np.dtype([("x", "<i2"), ("y", "<i2"), ("z", "<i2"), ("pad", "<i2"), ("offset", "<i4"), ("ptr", "<i4")])
VOXEL_DTYPE = np.dtype([("sdf", "<i2"), ("w", "u1"), ("pad", "u1")])
VOXEL_RESET = 0x00007FFF            # Voxel_s(): sdf 32767, w 0
FOUND_NONE, FOUND_BUCKET, FOUND_CHAIN, FOUND_BUCKET_OUT, FOUND_CHAIN_OUT = range(5)   # (_OUT: swapped out, ptr == -1)


def reset_entry():
    """ResetScene's HashEntry."""
    return np.array((0, 0, 0, 0, 0, -2), HASH_DTYPE)


def empty_hash(n_total):
    return np.full(n_total, reset_entry(), HASH_DTYPE)


def hash_index(x, y, z, n_buckets):
    """hashIndex (RepresentationAccess.hpp:5-7) in uint32 arithmetic: a Python int of scalars, an int64 array of
    arrays."""
    x, y, z = (np.asarray(v).astype(np.int64).astype(np.uint32) for v in (x, y, z))
    with np.errstate(over="ignore"):
        h = ((x * np.uint32(73856093)) ^ (y * np.uint32(19349669)) ^ (z * np.uint32(83492791))) & np.uint32(n_buckets - 1)
    return int(h) if np.ndim(h) == 0 else h.astype(np.int64)


def chain(hash, n_buckets, pos):
    """The entry indices on pos's chain in walk order: the bucket entry, then the excess entries its offsets name.
    The step and the end test of every walk of the reference; which entry matches is the caller's rule."""
    i = hash_index(*pos, n_buckets)
    while True:
        yield i
        offset = int(hash["offset"][i])
        if offset < 1:
            return
        i = n_buckets + offset - 1


def _pos(pos):
    return tuple(int(v) for v in pos)


def _at(hash, i, pos):
    return (int(hash["x"][i]), int(hash["y"][i]), int(hash["z"][i])) == pos


def find_live(hash, n_buckets, pos):
    """findVoxel's walk (RepresentationAccess.hpp:31-49): (entry, ptr) of the first entry at pos with ptr >= 0, or
    (-1, -1).  A coordinate outside int16 is missing."""
    pos = _pos(pos)
    if all(-32768 <= v <= 32767 for v in pos):
        for i in chain(hash, n_buckets, pos):
            if _at(hash, i, pos) and hash["ptr"][i] >= 0:
                return i, int(hash["ptr"][i])
    return -1, -1


def find_held(hash, n_buckets, pos, from_free_bucket=True):
    """(every entry on pos's chain at pos with ptr >= -1, the entries walked).  The whole chain, as findVoxel walks
    it; with from_free_bucket=False as probe() does, which follows no chain from a free bucket entry (ptr < -1)."""
    pos = _pos(pos)
    found, walked = [], 0
    for i in chain(hash, n_buckets, pos):
        if not from_free_bucket and walked == 0 and hash["ptr"][i] < -1:
            break
        walked += 1
        if _at(hash, i, pos) and hash["ptr"][i] >= -1:
            found.append(i)
    return found, walked


def probe(hash, n_buckets, pos):
    """One step's probe of buildHashAllocAndVisibleTypePP (SceneReconstructionEngine.hpp:249-293) in the read-only
    table: (entry, request type, found class).  Type 0: found there; 1: the free bucket entry is requested; 2: an
    excess entry behind the chain's end, which is `entry`."""
    pos = _pos(pos)
    for n, i in enumerate(chain(hash, n_buckets, pos)):
        ptr = int(hash["ptr"][i])
        if _at(hash, i, pos) and ptr >= -1:
            if n == 0:
                return i, 0, FOUND_BUCKET_OUT if ptr == -1 else FOUND_BUCKET
            return i, 0, FOUND_CHAIN_OUT if ptr == -1 else FOUND_CHAIN
        if n == 0 and ptr < -1:
            return i, 1, FOUND_NONE
    return i, 2, FOUND_NONE


def place(hash, n_buckets, pos, ptr, excess, last_excess):
    """allocateVoxelBlocksList's rule (SceneReconstructionEngine_host.cu:350-415) for a position the table does not
    hold: the bucket entry when it is free, else excessList[lastFreeExcessListId--] linked to the end of the chain.
    Writes the entry; -> (entry, lastFreeExcessListId')."""
    t = hash_index(*pos, n_buckets)
    if hash["ptr"][t] >= -1:
        *_, end = chain(hash, n_buckets, pos)
        slot = int(excess[last_excess])
        last_excess -= 1
        hash["offset"][end] = slot + 1
        t = n_buckets + slot
    hash[t] = (*_pos(pos), 0, 0, ptr)
    return t, last_excess
