// tf_scene_ckpt.hip -- scene and map checkpoints for gfx950 (an addition: the reference cannot save its map;
// DESIGN.md §5 Scene checkpoints / Map checkpoints / Resized load, the file in tf_scene_file.h).  Everything that
// is written in order here -- the records in hash-entry order, the lists the block copies walk, the re-hashed
// placement, the visible list -- is made by one ordered compaction, the scheme the mesh passes use: a count per
// 256 items, a prefix, an emit pass, as plain launches on the context stream (the skeleton: tf_compact.h, shared
// with a free view's visible list, tf_view.hip):
//
//   k_ck_pass<false, P> : per 256-item group how many items take a place in each of pass P's (up to three) lists
//   k_ck_prefix         : exclusive scan of the group counts (one workgroup: a count per 256 items) + the totals
//   k_ck_pass<true, P>  : every item with its place in each list -- the group's base, the waves before, the lanes below
//
// and the passes are: CkSavePass (an entry gets a record / holds a block / has a stored block in the GlobalCache:
// the record table and the two lists the gathers walk), CkRzPass (the resized load's placement), CkVisPass (its
// visible list) and CkMergePass (the map merge's placement against a live table, tf_map_merge, further down).  The counts fit 32 bits (records <= n_total, blocks <= n_blocks), so the scan is a small kernel of
// its own over int4 group counts (16 B per 256 items, the fourth lane zero; a pass with fewer lists leaves the
// others zero) rather than k_mesh_prefix over 64-bit per-entry counts, and shares no scratch with a mesh extraction.
// No atomics in these passes, and no workgroup waits on another inside a grid.  Beside them:
//
//   k_ck_copy<GATHER>             : blocks [b0, b0 + nb) of the ptr list between the VBA (and the colour plane) and
//                                   the staging buffer, 16 B per lane: a wave instruction moves 1 KiB, contiguous on
//                                   both sides inside a block; no atomics
//   k_ck_copy_store<GATHER, SKIP> : the same between the GlobalCache's store + entry * 512 and the staging buffer
//   k_ck_apply                    : hash[index], visType[index] (and the cache bytes) from the records (load; the
//                                   block grid is rebuilt after)
//   k_rz_hash, k_rz_round, k_rz_apply : the resized load's re-hash (further down)
//
// A swapping context (tf_map_save / tf_map_load) differs by a uniform `sw`: the GlobalCache's swap state and stored
// flag in the record predicate and in every record (version 2 of the file), the stored blocks as a second payload.
#include "tf_host.h"
#include "tf_compact.h"
#include "tf_scene_file.h"
#include "tf_swap_combine.h"

#include <chrono>
#include <vector>
#include <stdio.h>
#include <stdlib.h>

typedef unsigned ck_u4 __attribute__((ext_vector_type(4)));
typedef unsigned ck_u2 __attribute__((ext_vector_type(2)));

// ---- the record (tf_scene_file.h): 24 bytes as three 8-byte words -- the entry's index, the HashEntry's four words,
// then visType, swapState, hasStoredData, 0.  Without the GlobalCache (version 1) the last three bytes are zero.
struct CkRecord { unsigned idx; ck_u4 e; unsigned tail; };

__device__ __forceinline__ void ck_record_store(ck_u2* __restrict__ records, size_t k, const CkRecord& r)
{
    ck_u2* p = records + 3 * k;
    p[0] = ck_u2{ r.idx, r.e.x };
    p[1] = ck_u2{ r.e.y, r.e.z };
    p[2] = ck_u2{ r.e.w, r.tail };
}

__device__ __forceinline__ CkRecord ck_record_load(const ck_u2* __restrict__ records, size_t k)
{
    const ck_u2 a = records[3 * k], b = records[3 * k + 1], c = records[3 * k + 2];
    return CkRecord{ a.x, ck_u4{ a.y, b.x, b.y, c.x }, c.y };
}

// a record's last word at entry `at` (with sw: swapState / swapFlags were cleared over the whole table before)
__device__ __forceinline__ void ck_tail_apply(unsigned tail, int at, int sw, unsigned char* __restrict__ visType,
                                              unsigned char* __restrict__ swapState, unsigned char* __restrict__ swapFlags)
{
    visType[at] = (unsigned char)tail;
    if (sw) {
        swapState[at] = (unsigned char)(tail >> 8);
        swapFlags[at] = (unsigned char)(tail >> 16);
    }
}

// save: entry idx gets a record (HashEntry not ResetScene's, or visType or a cache byte != 0), the record carries a
// block (ptr >= 0), the entry has a stored block (hasStoredData).  Emit: the record at its place, the block's ptr and
// the flagged entry's index in record order -- the lists the two gathers walk.
struct CkSavePass {
    typedef CkRecord Item;
    const TfHashEntry* hash;
    const unsigned char *visType, *swapState, *swapFlags;
    int sw, n_blocks;
    int* bad;                                              // the count launch's: set when a block lies outside the VBA
    ck_u2* records;                                        // (an uploaded table): not saveable.  The emit launch's:
    int *blockPtr, *storedIdx;                             // the record table and the two lists

    __device__ __forceinline__ unsigned classify(int idx, bool in, CkRecord& r) const
    {
        r = CkRecord{ (unsigned)idx, ck_u4{ 0u, 0u, 0u, 0xfffffffeu }, 0u };
        if (in) {
            r.e = *reinterpret_cast<const ck_u4*>(hash + idx);
            r.tail = visType[idx];
            if (sw) r.tail |= (unsigned)swapState[idx] << 8 | (unsigned)swapFlags[idx] << 16;
        }
        const bool rec = (r.e.x | r.e.y | r.e.z) != 0u || r.e.w != 0xfffffffeu || r.tail != 0u;
        const bool blk = rec && (int)r.e.w >= 0;
        if (bad && blk && (int)r.e.w >= n_blocks) *bad = 1;
        return (unsigned)rec | (unsigned)blk << 1 | (r.tail >> 16 != 0u ? 4u : 0u);
    }
    __device__ __forceinline__ void emit(int idx, const CkRecord& r, unsigned bits, int at_rec, int at_blk, int at_sto) const
    {
        if (bits & 1u) ck_record_store(records, (size_t)at_rec, r);
        if (bits & 2u) blockPtr[at_blk] = (int)r.e.w;
        if (bits & 4u) storedIdx[at_sto] = idx;
    }
};

// 16-byte unit u of the chunk: block u / U, unit u % U of it (U = 128, or 256 with colour: the block's
// voxels, then its colour words)
template <bool GATHER>
__global__ __launch_bounds__(CK_WG) void k_ck_copy(ck_u4* __restrict__ vba, ck_u4* __restrict__ rgb, const int* __restrict__ blockPtr,
                                                   int nb, ck_u4* __restrict__ stage)
{
    const unsigned sh = rgb ? 8u : 7u, U = 1u << sh;
    const size_t n = (size_t)nb << sh;
    for (size_t u = (size_t)blockIdx.x * CK_WG + threadIdx.x; u < n; u += (size_t)gridDim.x * CK_WG) {
        const unsigned b = (unsigned)(u >> sh), r = (unsigned)u & (U - 1u);
        const size_t blk = (size_t)blockPtr[b] * 128u;
        ck_u4* p = r < 128u ? vba + blk + r : rgb + blk + (r - 128u);
        if (GATHER) __builtin_nontemporal_store(*p, stage + u);
        else *p = __builtin_nontemporal_load(stage + u);
    }
}

// blocks [0, nb) of the entry-index list between the GlobalCache's store and the staging buffer: k_ck_copy's
// shape (16 B per lane, a wave instruction per KiB, contiguous inside a block).  The store is indexed by hash
// entry, 2 KiB each, so the offset is formed in 64 bits (it passes 4 GiB above 2^21 entries); it is touched
// once, so its side is nontemporal too.
// SKIP (the resized load): a list value of -1 names no entry, its block stays in the staging buffer
template <bool GATHER, bool SKIP>
__global__ __launch_bounds__(CK_WG) void k_ck_copy_store(ck_u4* __restrict__ store, const int* __restrict__ storedIdx, int nb,
                                                         ck_u4* __restrict__ stage)
{
    const size_t n = (size_t)nb << 7;
    for (size_t u = (size_t)blockIdx.x * CK_WG + threadIdx.x; u < n; u += (size_t)gridDim.x * CK_WG) {
        const int idx = storedIdx[u >> 7];
        if (SKIP && idx < 0) continue;
        ck_u4* p = store + (size_t)idx * 128u + ((unsigned)u & 127u);
        if (GATHER) __builtin_nontemporal_store(__builtin_nontemporal_load(p), stage + u);
        else __builtin_nontemporal_store(__builtin_nontemporal_load(stage + u), p);
    }
}

__global__ __launch_bounds__(CK_WG) void k_ck_apply(const ck_u2* __restrict__ records, long long n_records, int sw,
                                                    TfHashEntry* __restrict__ hash, unsigned char* __restrict__ visType,
                                                    unsigned char* __restrict__ swapState, unsigned char* __restrict__ swapFlags)
{
    for (long long k = (long long)blockIdx.x * CK_WG + threadIdx.x; k < n_records; k += (long long)gridDim.x * CK_WG) {
        const CkRecord r = ck_record_load(records, (size_t)k);
        *reinterpret_cast<ck_u4*>(hash + r.idx) = r.e;
        ck_tail_apply(r.tail, (int)r.idx, sw, visType, swapState, swapFlags);
    }
}

// ---- the resized load (tf_map_load_resized, DESIGN.md §5 Resized load): the file's records re-hashed into tables
// of other capacities.  Record j (file order) with ptr >= -1 is carried; h(j) its bucket in the new table, m(j) its
// rank among the carried records of that bucket by record number, o(j) / b(j) the records before j with m > 0 / with
// ptr >= 0:  t(j) = h if m == 0 else n_buckets + n_excess - 1 - o(j),  ptr'(j) = n_blocks - 1 - b(j) -- what one
// insertion after another by the reference's allocation rule into a reset table gives.
//
//   k_rz_hash   : h(j) (-1: dropped) and the first round's atomicMin of j per bucket
//   k_rz_round  : round r -- the record a bucket's minimum names has rank r and becomes the successor of the
//                 bucket's rank r - 1 record; the others bid (atomicMin) for round r + 1.  Three bucket arrays in
//                 rotation (this round's minima, the last round's winners, the next round's bids), so no array is
//                 read and bid into in one launch; the host runs rounds until no record is left: longest_chain
//                 of them.  A minimum over record numbers does not depend on the order the atomics land in.
//   CkRzPass    : counted -- per 256 records those with m > 0, with ptr >= 0, with a stored block (dropped ones too:
//                 their blocks lie in the file's second payload); emitted -- t(j), ptr'(j), and the two lists the
//                 scatters walk: ptr' per active block, t (-1: a dropped record's, skipped) per stored block
//   k_rz_apply  : hash[t] = {pos, the successor's excess slot + 1, ptr'}, visType and the cache bytes at t
//   CkVisPass   : the ascending entries with visType > 0, the first vis_capacity of them
//
// Everything up to CkRzPass's count writes scratch only: the fit is checked on its totals before the context is touched.
#define RZ_NONE 0x7f7f7f7f                                 // no record (above every record number); memset's 0x7f

__global__ __launch_bounds__(CK_WG) void k_rz_hash(const ck_u2* __restrict__ records, int n, unsigned mask, int sw, int* __restrict__ rzH,
                                                   int* __restrict__ rzRank, int* __restrict__ rzSucc, int* __restrict__ bid,
                                                   int* __restrict__ tally)
{
    const int ng = (n + CK_WG - 1) / CK_WG;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        const int j = g * CK_WG + threadIdx.x;
        bool carried = false, cached = false;
        if (j < n) {
            const ck_u2 a = records[3 * (size_t)j], b = records[3 * (size_t)j + 1], c = records[3 * (size_t)j + 2];
            carried = (int)c.x >= -1;
            cached = carried && sw && ((c.y >> 16) & 0xffu) != 0u;
            int h = -1;
            if (carried) {
                h = tf_hash_index((short)(a.y & 0xffffu), (short)(a.y >> 16), (short)(b.x & 0xffffu), mask);
                atomicMin(bid + h, j);
            }
            rzH[j] = h;
            rzRank[j] = -1;
            rzSucc[j] = -1;
        }
        const int nc = __popcll(__ballot(carried)), ns = __popcll(__ballot(cached));
        if ((threadIdx.x & 63) == 0 && nc) {               // (sums: the order they land in does not show)
            atomicAdd(tally + 0, nc);
            if (ns) atomicAdd(tally + 1, ns);
        }
    }
}

__global__ __launch_bounds__(CK_WG) void k_rz_round(int n, int r, const int* __restrict__ rzH, int* __restrict__ rzRank,
                                                    int* __restrict__ rzSucc, const int* __restrict__ cur, int* __restrict__ prev,
                                                    int* __restrict__ next, int* __restrict__ left)
{
    const int ng = (n + CK_WG - 1) / CK_WG;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        const int j = g * CK_WG + threadIdx.x;
        bool waits = false;
        if (j < n) {
            const int h = rzH[j];
            if (h >= 0 && rzRank[j] < 0) {
                if (cur[h] == j) {
                    rzRank[j] = r;
                    const int p = prev[h];                 // the bucket's record of rank r - 1 (this thread alone reads
                    if (p != RZ_NONE) rzSucc[p] = j;       // and clears it: it is round r + 1's bidding array)
                    prev[h] = RZ_NONE;
                } else {
                    atomicMin(next + h, j);
                    waits = true;
                }
            }
        }
        const int nw = __popcll(__ballot(waits));
        if ((threadIdx.x & 63) == 0 && nw) atomicAdd(left, nw);
    }
}

// after the rounds: record j uses an excess slot, holds a block, names a stored block.  Emit: rzH becomes ptr'(j)
// (its h is spent once t is known); rzT[j] = -1 marks a dropped record
struct CkRzPass {
    struct Item {};
    const ck_u2* records;
    const int* rzRank;
    int sw, n_buckets, n_excess, n_blocks;
    int *rzH, *rzT, *blockPtr, *storedIdx;

    __device__ __forceinline__ unsigned classify(int j, bool in, Item&) const
    {
        if (!in) return 0u;
        const ck_u2 c = records[3 * (size_t)j + 2];
        const bool exc = rzRank[j] > 0, blk = (int)c.x >= 0, sto = sw && ((c.y >> 16) & 0xffu) != 0u;
        return (unsigned)exc | (unsigned)blk << 1 | (unsigned)sto << 2;
    }
    __device__ __forceinline__ void emit(int j, const Item&, unsigned bits, int at_exc, int at_blk, int at_sto) const
    {
        const int h = rzH[j];
        const int at = h < 0 ? -1 : (bits & 1u) ? n_buckets + n_excess - 1 - at_exc : h;
        const int ptr = (bits & 2u) ? n_blocks - 1 - at_blk : -1;
        rzT[j] = at;
        rzH[j] = ptr;
        if (bits & 2u) blockPtr[at_blk] = ptr;
        if (bits & 4u) storedIdx[at_sto] = at;
    }
};

__global__ __launch_bounds__(CK_WG) void k_rz_apply(const ck_u2* __restrict__ records, int n, int sw, int n_buckets,
                                                    const int* __restrict__ rzPtr, const int* __restrict__ rzSucc,
                                                    const int* __restrict__ rzT, TfHashEntry* __restrict__ hash,
                                                    unsigned char* __restrict__ visType, unsigned char* __restrict__ swapState,
                                                    unsigned char* __restrict__ swapFlags)
{
    for (int j = blockIdx.x * CK_WG + threadIdx.x; j < n; j += gridDim.x * CK_WG) {
        const int at = rzT[j];
        if (at < 0) continue;
        const CkRecord r = ck_record_load(records, (size_t)j);
        const int succ = rzSucc[j];
        const unsigned offset = succ >= 0 ? (unsigned)(rzT[succ] - n_buckets + 1) : 0u;
        *reinterpret_cast<ck_u4*>(hash + at) = ck_u4{ r.e.x, r.e.y & 0xffffu, offset, (unsigned)rzPtr[j] };
        ck_tail_apply(r.tail, at, sw, visType, swapState, swapFlags);
    }
}

struct CkVisPass {
    struct Item {};
    const unsigned char* visType;
    int capacity;
    int* visibleIds;

    __device__ __forceinline__ unsigned classify(int idx, bool in, Item&) const { return in && visType[idx] != 0 ? 1u : 0u; }
    __device__ __forceinline__ void emit(int idx, const Item&, unsigned bits, int at, int, int) const
    {
        if ((bits & 1u) && at < capacity) visibleIds[at] = idx;
    }
};

// ---- the map merge (tf_map_merge, DESIGN.md §5 Map merge): a version-1 file's carried records (ptr >= 0, file order),
// moved by a whole-block offset, into the live table.  A position the table holds with a block is combined voxel by
// voxel, one it holds with ptr == -1 gets a block, a new one is inserted by the reference's allocation rule.
//
//   k_mg_find   : the reference's walk per record, read only: the entry that holds pos' (mode combine / revive), or
//                 (mode insert) the bucket h, the end of its chain e(h) (-1: the bucket entry itself is free) and the
//                 first round's atomicMin of j per bucket -- k_rz_hash's part for the records not found
//   k_rz_round  : the ranks m(j) among the records not found, as the resized load's
//   CkMergePass : counted -- per 256 records those that need an excess slot (not found, and m > 0 or no free bucket
//                 entry), a block (inserted or revived), and the carried ones; emitted -- t(j), ptr'(j) from the LIVE
//                 lists (excessList[lastFreeExcessListId - o(j)], allocList[lastFreeBlockId - b(j)]) and, per block of
//                 the file's payload, the word k_mg_blocks reads: the target ptr, bit 31 set to combine
//   k_mg_apply  : the new entries, the revived entries' ptr, the link from e(h), the block grid cells
//   k_mg_blocks : a staged chunk into the VBA, k_ck_copy's shape: copied, or sw_combine(file, context) per voxel
//
// Everything up to CkMergePass's emit writes scratch only; a table or list the walk cannot trust (a chain that leaves
// the excess area or does not end, a ptr or a list value outside its table: uploaded tables) sets `bad`.
enum { MG_SKIP = 0, MG_COMBINE = 1, MG_REVIVE = 2, MG_INSERT = 3 };
enum { MG_N_INSERT = 0, MG_N_COMBINE = 1, MG_LEFT = 2, MG_N_REVIVE = 3, MG_BAD = 4, MG_TALLY = 8 };

struct MgOffset { int x, y, z; };

__global__ __launch_bounds__(CK_WG) void k_mg_find(const ck_u2* __restrict__ records, int n, MgOffset off, const TfHashEntry* __restrict__ hash,
                                                   unsigned mask, int n_buckets, int n_excess, int n_blocks, int* __restrict__ mgH,
                                                   int* __restrict__ mgRank, int* __restrict__ mgSucc, int* __restrict__ mgFound,
                                                   int* __restrict__ mgEnd, int* __restrict__ mgMode, int* __restrict__ bid,
                                                   int* __restrict__ tally)
{
    const int ng = (n + CK_WG - 1) / CK_WG;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        const int j = g * CK_WG + threadIdx.x;
        int mode = MG_SKIP;
        if (j < n) {
            const ck_u2 a = records[3 * (size_t)j], b = records[3 * (size_t)j + 1], c = records[3 * (size_t)j + 2];
            int h = -1, found = -1, end = -1;
            if ((int)c.x >= 0) {
                const int x = (short)(a.y & 0xffffu) + off.x, y = (short)(a.y >> 16) + off.y, z = (short)(b.x & 0xffffu) + off.z;
                const unsigned k0 = ((unsigned)x & 0xffffu) | (unsigned)y << 16, k1 = (unsigned)z & 0xffffu;
                h = tf_hash_index(x, y, z, mask);
                mode = MG_INSERT;
                int i = h, steps = 0;
                ck_u4 e = *reinterpret_cast<const ck_u4*>(hash + i);
                if ((int)e.w >= -1) {                      // (a free bucket entry: its chain is not followed)
                    for (;;) {
                        if (e.x == k0 && (e.y & 0xffffu) == k1 && (int)e.w >= -1) {
                            found = i;
                            mode = (int)e.w >= 0 ? MG_COMBINE : MG_REVIVE;
                            if ((int)e.w >= n_blocks) tally[MG_BAD] = 1;
                            break;
                        }
                        const int o = (int)e.z;
                        if (o < 1) { end = i; break; }
                        if (o > n_excess || ++steps > n_excess) { tally[MG_BAD] = 1; mode = MG_SKIP; break; }
                        i = n_buckets + o - 1;
                        e = *reinterpret_cast<const ck_u4*>(hash + i);
                    }
                }
                if (mode == MG_INSERT) atomicMin(bid + h, j);
                else h = -1;
            }
            mgH[j] = h;
            mgRank[j] = -1;
            mgSucc[j] = -1;
            mgFound[j] = found;
            mgEnd[j] = end;
            mgMode[j] = mode;
        }
        const int ni = __popcll(__ballot(mode == MG_INSERT)), nc = __popcll(__ballot(mode == MG_COMBINE)),
                  nr = __popcll(__ballot(mode == MG_REVIVE));
        if ((threadIdx.x & 63) == 0) {                     // (sums: the order they land in does not show)
            if (ni) atomicAdd(tally + MG_N_INSERT, ni);
            if (nc) atomicAdd(tally + MG_N_COMBINE, nc);
            if (nr) atomicAdd(tally + MG_N_REVIVE, nr);
        }
    }
}

struct CkMergePass {
    struct Item {};
    const int *mgMode, *mgRank, *mgEnd, *mgFound, *mgH;
    const TfHashEntry* hash;
    const int *allocList, *excessList;
    int lastBlock, lastExcess, n_buckets, n_excess, n_blocks;
    int *mgT, *mgPtr;
    unsigned* blockWord;
    int* bad;

    __device__ __forceinline__ unsigned classify(int j, bool in, Item&) const
    {
        if (!in) return 0u;
        const int m = mgMode[j];
        const bool exc = m == MG_INSERT && (mgRank[j] > 0 || mgEnd[j] >= 0), blk = m == MG_INSERT || m == MG_REVIVE;
        return (unsigned)exc | (unsigned)blk << 1 | (unsigned)(m != MG_SKIP) << 2;
    }
    __device__ __forceinline__ void emit(int j, const Item&, unsigned bits, int at_exc, int at_blk, int at_car) const
    {
        const int m = mgMode[j];
        int t = m == MG_INSERT ? mgH[j] : mgFound[j], ptr = -1;
        if (bits & 1u) {
            int x = excessList[lastExcess - at_exc];
            if ((unsigned)x >= (unsigned)n_excess) { *bad = 1; x = 0; }
            t = n_buckets + x;
        }
        if (bits & 2u) ptr = allocList[lastBlock - at_blk];
        else if (m == MG_COMBINE) ptr = hash[t].ptr;
        if ((bits & 4u) && (unsigned)ptr >= (unsigned)n_blocks) { *bad = 1; ptr = 0; }
        mgT[j] = t;
        mgPtr[j] = ptr;
        if (bits & 4u) blockWord[at_car] = (unsigned)ptr | (m == MG_COMBINE ? 0x80000000u : 0u);
    }
};

__global__ __launch_bounds__(CK_WG) void k_mg_apply(const ck_u2* __restrict__ records, int n, MgOffset off, int n_buckets,
                                                    const int* __restrict__ mgMode, const int* __restrict__ mgRank,
                                                    const int* __restrict__ mgSucc, const int* __restrict__ mgEnd,
                                                    const int* __restrict__ mgT, const int* __restrict__ mgPtr, TfHashEntry* __restrict__ hash,
                                                    unsigned char* __restrict__ visType, int2* __restrict__ grid)
{
    for (int j = blockIdx.x * CK_WG + threadIdx.x; j < n; j += gridDim.x * CK_WG) {
        const int m = mgMode[j];
        if (m != MG_INSERT && m != MG_REVIVE) continue;
        const int at = mgT[j];
        TfHashEntry e;
        if (m == MG_REVIVE) {                              // the ptr word alone: another record may link from this entry
            e = hash[at];
            e.ptr = mgPtr[j];
            hash[at].ptr = e.ptr;
        } else {
            const ck_u2 a = records[3 * (size_t)j], b = records[3 * (size_t)j + 1];
            const int succ = mgSucc[j];
            e.x = (short)((short)(a.y & 0xffffu) + off.x);
            e.y = (short)((short)(a.y >> 16) + off.y);
            e.z = (short)((short)(b.x & 0xffffu) + off.z);
            e.pad = 0;
            e.offset = succ >= 0 ? mgT[succ] - n_buckets + 1 : 0;
            e.ptr = mgPtr[j];
            hash[at] = e;
            visType[at] = 0;
            if (mgRank[j] == 0 && mgEnd[j] >= 0) hash[mgEnd[j]].offset = at - n_buckets + 1;     // (the offset word alone)
        }
        grid_set(grid, e, at);
    }
}

// 16-byte unit u of the chunk: block u / 128, unit u % 128 of it; word[b]: the block's ptr, bit 31 -- combine
__global__ __launch_bounds__(CK_WG) void k_mg_blocks(ck_u4* __restrict__ vba, const unsigned* __restrict__ word, int nb, int maxW,
                                                     const ck_u4* __restrict__ stage)
{
    const size_t n = (size_t)nb << 7;
    for (size_t u = (size_t)blockIdx.x * CK_WG + threadIdx.x; u < n; u += (size_t)gridDim.x * CK_WG) {
        const unsigned w = word[u >> 7];
        ck_u4* p = vba + (size_t)(w & 0x7fffffffu) * 128u + ((unsigned)u & 127u);
        ck_u4 v = __builtin_nontemporal_load(stage + u);
        if (w >> 31) {
            const ck_u4 d = *p;
            v = ck_u4{ sw_combine(v.x, d.x, maxW), sw_combine(v.y, d.y, maxW), sw_combine(v.z, d.z, maxW), sw_combine(v.w, d.w, maxW) };
        }
        *p = v;
    }
}

// ---- the launchers (ck_groups, ck_grid, tfk_ck_count, tfk_ck_emit: tf_compact.h) ---------------------
// what the staging buffer and its pinned twin hold: ckpt_chunk_blocks blocks (with their colour)
static size_t ck_stage_bytes(const tf_ctx* c)
{
    return (size_t)c->ckpt_chunk_blocks * TF_SCENE_BLOCK_BYTES * (c->p.voxel_rgb ? 2 : 1);
}

// the context's checkpoint scratch, from the first call on: a pass's scratch over the n_total entries -- the group
// counts, their bases + totals -- and the "not saveable" flag; the device staging buffer and its pinned twin
static hipError_t tfk_ckpt_scratch(tf_ctx* c)
{
    if (c->ckptGroup) return hipSuccess;
    const size_t ng = (size_t)ck_groups(c->n_total);
    return tf_mem_hip(c->mem.alloc_group({ TfCtxMem::dev(&c->ckptGroup, sizeof(int4) * (2 * ng + 2)),
                                           TfCtxMem::dev(&c->ckptStage, ck_stage_bytes(c)),
                                           TfCtxMem::pin(&c->ckptPinned, ck_stage_bytes(c), hipHostMallocDefault) }));
}

static CkSavePass ck_save_pass(const tf_ctx* c)
{
    return CkSavePass{ c->hash, c->visType, c->swapState, c->swapFlags, c->p.use_swapping != 0, c->p.n_blocks, nullptr, nullptr, nullptr, nullptr };
}

// count + prefix; totals[0] = {records, blocks, flagged (0 without swapping), -}, totals[1].x = the "not saveable"
// flag (device addresses)
static hipError_t tfk_ckpt_count(tf_ctx* c, const int4** totals)
{
    CkSavePass p = ck_save_pass(c);
    *totals = c->ckptGroup + 2 * ck_groups(c->n_total);
    p.bad = (int*)(*totals + 1);
    const hipError_t e = hipMemsetAsync(p.bad, 0, sizeof(int4), c->stream);
    return e != hipSuccess ? e : tfk_ck_count(c, p, c->n_total, c->ckptGroup);
}

// after tfk_ckpt_count: records (n_records x 24 B), the stored blocks' ptr list and (swapping) the flagged entries'
// index list, device buffers of the caller
static hipError_t tfk_ckpt_records(tf_ctx* c, void* records, int* blockPtr, int* storedIdx)
{
    CkSavePass p = ck_save_pass(c);
    p.records = (ck_u2*)records;
    p.blockPtr = blockPtr;
    p.storedIdx = storedIdx;
    return tfk_ck_emit(c, p, c->n_total, c->ckptGroup);
}

// nb <= ckpt_chunk_blocks blocks of the ptr list into (gather) / out of the staging buffer
static hipError_t tfk_ckpt_copy(tf_ctx* c, bool gather, const int* blockPtr, int nb)
{
    const auto k = gather ? k_ck_copy<true> : k_ck_copy<false>;
    hipLaunchKernelGGL(k, dim3(ck_grid((size_t)nb * 256)), dim3(CK_WG), 0, c->stream, (ck_u4*)c->vba,
                       (ck_u4*)(c->p.voxel_rgb ? c->vba_rgb : nullptr), blockPtr, nb, (ck_u4*)c->ckptStage);
    return hipGetLastError();
}

// ... and stored blocks of the entry list (skip: -1 in it names no entry)
static hipError_t tfk_ckpt_copy_store(tf_ctx* c, bool gather, bool skip, const int* storedIdx, int nb)
{
    const auto k = gather ? k_ck_copy_store<true, false> : skip ? k_ck_copy_store<false, true> : k_ck_copy_store<false, false>;
    hipLaunchKernelGGL(k, dim3(ck_grid((size_t)nb * 128)), dim3(CK_WG), 0, c->stream, (ck_u4*)c->swapStore, storedIdx, nb,
                       (ck_u4*)c->ckptStage);
    return hipGetLastError();
}

static hipError_t tfk_ckpt_apply(tf_ctx* c, const void* records, long long n_records, int sw)
{
    if (n_records == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ck_apply, dim3(ck_grid((size_t)n_records)), dim3(CK_WG), 0, c->stream, (const ck_u2*)records, n_records, sw, c->hash,
                       c->visType, c->swapState, c->swapFlags);
    return hipGetLastError();
}

// ---- the entry points --------------------------------------------------------------------------------
// what the last save / load spent (tf_scene_ckpt_times): the host clock around the synchronous steps, and,
// on a context created with TFUSION_CKPT_TIMING=1, the kernels by HIP events on the stream
enum { CK_T_INDEX = 0, CK_T_BLOCKS = 1, CK_T_COPY = 2, CK_T_FILE = 3, CK_T_CALL = 4, CK_T_BLOCK_BYTES = 5, CK_T_CHECK = 6 };
static double ck_now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// the kernels enqueued by `launch`; with ckpt_timing waited for and timed into slot `which`
template <class F>
static tf_status ck_timed_kernels(tf_ctx* c, int which, F launch)
{
    if (!c->ckpt_timing) {
        TF_CHECK(launch());
        return TF_OK;
    }
    if (!c->ckptEv[0]) {
        TF_CHECK(hipEventCreate(&c->ckptEv[0]));
        TF_CHECK(hipEventCreate(&c->ckptEv[1]));
    }
    TF_CHECK(hipEventRecord(c->ckptEv[0], c->stream));
    TF_CHECK(launch());
    TF_CHECK(hipEventRecord(c->ckptEv[1], c->stream));
    TF_CHECK(hipEventSynchronize(c->ckptEv[1]));
    float ms = 0;
    TF_CHECK(hipEventElapsedTime(&ms, c->ckptEv[0], c->ckptEv[1]));
    c->ckpt_ms[which] += ms;
    return TF_OK;
}

// `bytes` of device memory through the pinned buffer, a staging chunk at a time: sink(the chunk, its offset, its
// size) takes each on the host (and accounts for its own time)
template <class Sink>
static tf_status ckpt_d2h(tf_ctx* c, const void* dev, size_t bytes, Sink sink)
{
    const size_t cap = ck_stage_bytes(c);
    for (size_t o = 0; o < bytes; o += cap) {
        const size_t n = bytes - o < cap ? bytes - o : cap;
        const double t0 = ck_now_ms();
        TF_CHECK(hipMemcpyAsync(c->ckptPinned, (const char*)dev + o, n, hipMemcpyDeviceToHost, c->stream));
        TF_CHECK(hipStreamSynchronize(c->stream));
        c->ckpt_ms[CK_T_COPY] += ck_now_ms() - t0;
        const tf_status s = sink((const unsigned char*)c->ckptPinned, o, n);
        if (s != TF_OK) return s;
    }
    return TF_OK;
}

// ... to the file (bound > 0: the bytes are a list of ints that must lie in [0, bound), as load will require)
static tf_status ckpt_d2h_write(tf_ctx* c, FILE* f, const void* dev, size_t bytes, int bound = 0)
{
    return ckpt_d2h(c, dev, bytes, [&](const unsigned char* chunk, size_t, size_t n) -> tf_status {
        const double t0 = ck_now_ms();
        if (bound > 0 && !tf_scene_list_within(chunk, n / 4, bound)) return TF_INVALID_ARG;
        if (fwrite(chunk, 1, n, f) != n) return TF_INVALID_ARG;
        c->ckpt_ms[CK_T_FILE] += ck_now_ms() - t0;
        return TF_OK;
    });
}

// ... and host bytes to device memory the same way
static tf_status ckpt_h2d(tf_ctx* c, void* dev, const unsigned char* host, size_t bytes)
{
    const size_t cap = ck_stage_bytes(c);
    for (size_t o = 0; o < bytes; o += cap) {
        const size_t n = bytes - o < cap ? bytes - o : cap;
        const double t0 = ck_now_ms();
        memcpy(c->ckptPinned, host + o, n);
        TF_CHECK(hipMemcpyAsync((char*)dev + o, c->ckptPinned, n, hipMemcpyHostToDevice, c->stream));
        TF_CHECK(hipStreamSynchronize(c->stream));
        c->ckpt_ms[CK_T_COPY] += ck_now_ms() - t0;
    }
    return TF_OK;
}

// one block payload, n blocks of block_bytes each in list order, between the file and where the list says, in chunks
// of at most ckpt_chunk_blocks blocks through the staging buffer; kernels(b0, nb) enqueues the copy of blocks
// [b0, b0 + nb) of the list.  Save (f): the gather, then the chunk D2H and into the file.  Load (data, the payload in
// memory): the chunk H2D, then the scatter -- waited for, so the staging buffer is free again.
template <class K>
static tf_status ckpt_payload(tf_ctx* c, long long n, size_t block_bytes, FILE* f, const unsigned char* data, K kernels)
{
    for (long long b0 = 0; b0 < n; b0 += c->ckpt_chunk_blocks) {
        const int nb = (int)(n - b0 < c->ckpt_chunk_blocks ? n - b0 : c->ckpt_chunk_blocks);
        tf_status s = TF_OK;
        if (data) s = ckpt_h2d(c, c->ckptStage, data + (size_t)b0 * block_bytes, (size_t)nb * block_bytes);
        if (s == TF_OK) s = ck_timed_kernels(c, CK_T_BLOCKS, [&] { return kernels(b0, nb); });
        if (s == TF_OK && f) s = ckpt_d2h_write(c, f, c->ckptStage, (size_t)nb * block_bytes);
        if (s != TF_OK) return s;
        c->ckpt_ms[CK_T_BLOCK_BYTES] += 2.0 * (double)nb * (double)block_bytes;        // read + written
    }
    return TF_OK;
}

// version 1, or on a swapping context version 2 (tf_map_save): the cache's bytes in the records, the stored
// blocks as a second payload
static tf_status scene_save(tf_ctx* c, FILE* f)
{
    TfCtxMem tmp(c->mem.fns());                            // the record table and the lists, freed when this returns
    unsigned char* rec_dev = nullptr;
    int* ptr_dev = nullptr;
    int* sto_dev = nullptr;                                // swapping: the entries with a stored block, in record order
    const bool sw = c->p.use_swapping != 0;
    TF_CHECK(tfk_ckpt_scratch(c));
    tf_status s = sync_state(c);                           // counters, pose; TF_HIP_ERROR on a context in error
    if (s != TF_OK) return s;
    const TfDevState* st = c->st_host;
    struct tf_map_file_info minfo;
    memset(&minfo, 0, sizeof(minfo));
    minfo.version = sw ? (int)TF_MAP_VERSION : (int)TF_SCENE_VERSION;
    struct tf_scene_file_info& info = minfo.scene;
    info.params = c->p;
    if (sw) info.params.use_swapping = 1;                  // (tf_create takes any non-zero value; the file holds 1)
    info.pose_algebra = c->pose_alg;
    info.frame_counter = st->frame_counter;
    info.lastFreeBlockId = st->lastFreeBlockId;
    info.lastFreeExcessListId = st->lastFreeExcessListId;
    info.noVisibleEntries = st->noVisibleEntries;
    memcpy(info.pose, st->pose, sizeof(info.pose));
    const int4* totals_dev = nullptr;
    s = ck_timed_kernels(c, CK_T_INDEX, [&] { return tfk_ckpt_count(c, &totals_dev); });
    if (s != TF_OK) return s;
    int4 totals[2];
    TF_CHECK(hipMemcpyAsync(totals, totals_dev, sizeof(totals), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    if (totals[1].x) return TF_INVALID_ARG;                // an entry's ptr lies outside the VBA (uploaded tables)
    info.n_records = totals[0].x;
    info.n_blocks_stored = totals[0].y;
    minfo.n_cache_blocks = totals[0].z;                    // (0 without swapping)
    TfSceneLayout lay;
    if (!tf_map_layout(&minfo, &lay)) return TF_INVALID_ARG;       // counters outside their lists (tf_set_counters)
    info.file_bytes = (long long)lay.file_bytes;
    unsigned char hdr[TF_MAP_HEADER_BYTES];
    const size_t hdr_bytes = lay.records_off;
    uint32_t records_crc = 0;
    const auto encode = [&] {                              // (rewritten at the end with the records' checksum)
        if (sw) tf_map_header_encode(&minfo, records_crc, hdr);
        else tf_scene_header_encode(&info, records_crc, hdr);
    };
    encode();
    if (fwrite(hdr, 1, hdr_bytes, f) != hdr_bytes) return TF_INVALID_ARG;
    const size_t rec_bytes = (size_t)info.n_records * TF_SCENE_RECORD_BYTES;
    TF_CHECK(tf_mem_hip(tmp.alloc(&rec_dev, rec_bytes)));
    TF_CHECK(tf_mem_hip(tmp.alloc(&ptr_dev, sizeof(int) * (size_t)info.n_blocks_stored)));
    if (sw) TF_CHECK(tf_mem_hip(tmp.alloc(&sto_dev, sizeof(int) * (size_t)minfo.n_cache_blocks)));
    s = ck_timed_kernels(c, CK_T_INDEX, [&] { return tfk_ckpt_records(c, rec_dev, ptr_dev, sto_dev); });
    if (s != TF_OK) return s;
    {   // the record table: to the host whole (24 B per record), checked by load's own rule before any block
        // moves -- chain offsets, duplicate ptr (tables that came through tf_upload) -- then summed and written
        std::vector<unsigned char> rec(rec_bytes);
        s = ckpt_d2h(c, rec_dev, rec_bytes, [&](const unsigned char* chunk, size_t o, size_t n) -> tf_status {
            const double t0 = ck_now_ms();
            memcpy(rec.data() + o, chunk, n);
            c->ckpt_ms[CK_T_COPY] += ck_now_ms() - t0;
            return TF_OK;
        });
        if (s != TF_OK) return s;
        const double t1 = ck_now_ms();
        s = sw ? tf_map_records_check(rec.data(), info.n_records, &info.params, info.n_blocks_stored, minfo.n_cache_blocks)
               : tf_scene_records_check(rec.data(), info.n_records, &info.params, info.n_blocks_stored);
        if (s != TF_OK) return s;
        records_crc = tf_scene_crc32(0u, rec.data(), rec_bytes);
        const double t0 = ck_now_ms();
        c->ckpt_ms[CK_T_CHECK] += t0 - t1;
        if (fwrite(rec.data(), 1, rec_bytes, f) != rec_bytes) return TF_INVALID_ARG;
        c->ckpt_ms[CK_T_FILE] += ck_now_ms() - t0;
    }
    s = ckpt_payload(c, info.n_blocks_stored, lay.block_bytes, f, nullptr,
                     [&](long long b0, int nb) { return tfk_ckpt_copy(c, true, ptr_dev + b0, nb); });
    if (s == TF_OK) s = ckpt_payload(c, minfo.n_cache_blocks, TF_SCENE_BLOCK_BYTES, f, nullptr,          // the GlobalCache's
                                     [&](long long b0, int nb) { return tfk_ckpt_copy_store(c, true, false, sto_dev + b0, nb); });
    if (s == TF_OK) s = ckpt_d2h_write(c, f, c->visibleIds, 4 * lay.n_vis, c->n_total);
    if (s == TF_OK) s = ckpt_d2h_write(c, f, c->allocList, 4 * lay.n_alloc, c->p.n_blocks);
    if (s == TF_OK) s = ckpt_d2h_write(c, f, c->excessList, 4 * lay.n_excess, c->p.n_excess);
    for (int l = 0; l < TF_LEVELS && s == TF_OK; ++l) {
        s = ckpt_d2h_write(c, f, c->prev_pts[l], lay.map_bytes[l]);
        if (s == TF_OK) s = ckpt_d2h_write(c, f, c->prev_nrm[l], lay.map_bytes[l]);
    }
    if (s != TF_OK) return s;
    encode();
    if (fseeko(f, 0, SEEK_SET) != 0 || fwrite(hdr, 1, hdr_bytes, f) != hdr_bytes) return TF_INVALID_ARG;
    return TF_OK;
}

extern "C" tf_status tf_map_save(tf_ctx* c, const char* path)
{
    TF_FLUSH(c);
    if (!c || !path) return TF_INVALID_ARG;
    static_assert(TF_LEVELS == TF_SCENE_LEVELS, "the file stores the tracker's pyramid");
    {   // a context in error saves nothing (checked before the file is created)
        const tf_status s0 = sync_checked(c);
        if (s0 != TF_OK) return s0;
    }
    FILE* f = fopen(path, "wb");
    if (!f) return TF_INVALID_ARG;
    const double t_call = ck_now_ms();
    memset(c->ckpt_ms, 0, sizeof(c->ckpt_ms));
    tf_status s = scene_save(c, f);
    if (fclose(f) != 0 && s == TF_OK) s = TF_INVALID_ARG;
    if (s != TF_OK) remove(path);                          // no half-written checkpoint
    c->ckpt_ms[CK_T_CALL] = ck_now_ms() - t_call;
    return s;
}

extern "C" tf_status tf_scene_save(tf_ctx* c, const char* path)
{
    if (c && c->p.use_swapping) {                          // (after the deferred frame's tail, as every entry point)
        TF_FLUSH(c);
        return TF_INVALID_ARG;
    }
    return tf_map_save(c, path);
}

static bool bits_equal(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }

// what every load opens its writes to the context with: a full ResetScene (hash, VBA, colour, both lists (identity),
// block grid cells), visType zeroed; swapping: the loader's own states and flags of entries the file does not name
// must not survive; the store itself is not cleared: a stored block whose flag is 0 is read by nobody
static tf_status ckpt_clear_context(tf_ctx* c, bool sw)
{
    TF_CHECK(tfk_reset_scene(c));
    TF_CHECK(hipMemsetAsync(c->visType, 0, (size_t)c->n_total, c->stream));
    if (sw) {
        TF_CHECK(hipMemsetAsync(c->swapState, 0, (size_t)c->n_total, c->stream));
        TF_CHECK(hipMemsetAsync(c->swapFlags, 0, (size_t)c->n_total, c->stream));
    }
    return TF_OK;
}

// the file's two block payloads through the staging buffer to where the lists say: active blocks to ptr * 512 (and
// the colour plane), stored ones to store + entry * 512 (`skip`: -1 in that list names no entry)
static tf_status ckpt_load_blocks(tf_ctx* c, const unsigned char* data, const struct tf_map_file_info& minfo, const TfSceneLayout& lay,
                                  const int* ptr_dev, const int* sto_dev, bool skip)
{
    const tf_status s = ckpt_payload(c, minfo.scene.n_blocks_stored, lay.block_bytes, nullptr, data + lay.blocks_off,
                                     [&](long long b0, int nb) { return tfk_ckpt_copy(c, false, ptr_dev + b0, nb); });
    if (s != TF_OK) return s;
    return ckpt_payload(c, minfo.n_cache_blocks, TF_SCENE_BLOCK_BYTES, nullptr, data + lay.stored_off,
                        [&](long long b0, int nb) { return tfk_ckpt_copy_store(c, false, skip, sto_dev + b0, nb); });
}

// the end of a load: the file's previous maps, pose and frame counter; the counters as given
static tf_status ckpt_load_finish(tf_ctx* c, const unsigned char* data, const struct tf_scene_file_info& info, const TfSceneLayout& lay,
                                  int lastFreeBlockId, int lastFreeExcessListId, int noVisibleEntries)
{
    tf_status s = TF_OK;
    size_t o = lay.maps_off;
    for (int l = 0; l < TF_LEVELS && s == TF_OK; ++l) {
        s = ckpt_h2d(c, c->prev_pts[l], data + o, lay.map_bytes[l]);
        if (s == TF_OK) s = ckpt_h2d(c, c->prev_nrm[l], data + o + lay.map_bytes[l], lay.map_bytes[l]);
        o += 2 * lay.map_bytes[l];
    }
    if (s != TF_OK) return s;
    // what is not stored must not be seen stale: the next CreateExpectedDepths clears the whole range
    // image, the raycast pair starts from the default tile order with zero costs (mesh scratch is
    // recomputed by every extraction)
    TF_CHECK(ed_spill_all(c));
    TF_CHECK(tfk_tile_order_init(c));
    s = sync_state(c);
    if (s != TF_OK) return s;
    TfDevState* st = c->st_host;
    memcpy(st->pose, info.pose, sizeof(info.pose));
    st->lastFreeBlockId = lastFreeBlockId;
    st->lastFreeExcessListId = lastFreeExcessListId;
    st->noVisibleEntries = noVisibleEntries;
    st->vis_stale = 1;                                     // (the stored list may have been a capped one)
    st->frame_counter = info.frame_counter;
    // the free lists and the blocks in use need not be what frames alone leave (a scene that came
    // through tf_upload): every later reset clears everything (tf_reset.h)
    st->scene_external = 1;
    TF_CHECK(hipMemcpyAsync(c->st, c->st_host, sizeof(TfDevState), hipMemcpyHostToDevice, c->stream));
    s = sync_checked(c);
    if (s == TF_OK) c->frame_counter = info.frame_counter;
    return s;
}

// the validated file into the context (nothing here fails on the file's contents)
static tf_status scene_load(tf_ctx* c, const unsigned char* data, const struct tf_map_file_info& minfo, const TfSceneLayout& lay)
{
    TfCtxMem tmp(c->mem.fns());                            // the record table and the lists, freed when this returns
    unsigned char* rec_dev = nullptr;
    int* ptr_dev = nullptr;
    int* sto_dev = nullptr;
    const struct tf_scene_file_info& info = minfo.scene;
    const bool sw = minfo.version == (int)TF_MAP_VERSION;
    TF_CHECK(tfk_ckpt_scratch(c));
    tf_status s = ckpt_clear_context(c, sw);
    if (s != TF_OK) return s;
    const size_t rec_bytes = (size_t)info.n_records * TF_SCENE_RECORD_BYTES;
    TF_CHECK(tf_mem_hip(tmp.alloc(&rec_dev, rec_bytes)));
    TF_CHECK(tf_mem_hip(tmp.alloc(&ptr_dev, sizeof(int) * (size_t)info.n_blocks_stored)));
    s = ckpt_h2d(c, rec_dev, data + lay.records_off, rec_bytes);
    if (s != TF_OK) return s;
    {   // the stored blocks' ptr, in record order; version 2: and the entries with a block in the GlobalCache
        std::vector<int> ptrs, stored;
        ptrs.reserve((size_t)info.n_blocks_stored);
        stored.reserve((size_t)minfo.n_cache_blocks);
        const unsigned char* r = data + lay.records_off;
        for (long long k = 0; k < info.n_records; ++k, r += TF_SCENE_RECORD_BYTES) {
            int idx, ptr;
            memcpy(&idx, r, sizeof(int));
            memcpy(&ptr, r + 16, sizeof(int));
            if (ptr >= 0) ptrs.push_back(ptr);
            if (sw && r[22]) stored.push_back(idx);
        }
        s = ckpt_h2d(c, ptr_dev, (const unsigned char*)ptrs.data(), sizeof(int) * ptrs.size());
        if (s != TF_OK) return s;
        if (sw) {
            TF_CHECK(tf_mem_hip(tmp.alloc(&sto_dev, sizeof(int) * stored.size())));
            s = ckpt_h2d(c, sto_dev, (const unsigned char*)stored.data(), sizeof(int) * stored.size());
            if (s != TF_OK) return s;
        }
    }
    s = ckpt_load_blocks(c, data, minfo, lay, ptr_dev, sto_dev, false);
    if (s != TF_OK) return s;
    s = ck_timed_kernels(c, CK_T_INDEX, [&] {              // the block grid from the hash, as after a hash upload
        const hipError_t e = tfk_ckpt_apply(c, rec_dev, info.n_records, sw);
        return e == hipSuccess ? tfk_grid_rebuild(c) : e;
    });
    if (s != TF_OK) return s;
    s = ckpt_h2d(c, c->visibleIds, data + lay.vis_off, 4 * lay.n_vis);
    if (s == TF_OK) s = ckpt_h2d(c, c->allocList, data + lay.alloc_off, 4 * lay.n_alloc);
    if (s == TF_OK) s = ckpt_h2d(c, c->excessList, data + lay.excess_off, 4 * lay.n_excess);
    if (s != TF_OK) return s;
    return ckpt_load_finish(c, data, info, lay, info.lastFreeBlockId, info.lastFreeExcessListId, info.noVisibleEntries);
}

// the rank rounds over n records, `left` of which bid (rzH >= 0, rzRank < 0, the first bids in bid[0, nbk)): a round
// ranks one record of every bucket that has any left; *rounds of them were needed.  `counter` is a device word.
static tf_status ck_rank_rounds(tf_ctx* c, int n, int left, const int* rzH, int* rzRank, int* rzSucc, int* bid, int* counter, int* rounds)
{
    const int nbk = c->p.n_buckets;
    const dim3 grid(ck_grid((size_t)n)), wg(CK_WG);
    for (*rounds = 0; left > 0; ++*rounds) {
        const int r = *rounds;
        int* cur = bid + (size_t)(r % 3) * nbk;
        int* prev = bid + (size_t)((r + 2) % 3) * nbk;
        int* next = bid + (size_t)((r + 1) % 3) * nbk;
        const tf_status s = ck_timed_kernels(c, CK_T_INDEX, [&] {
            const hipError_t e = hipMemsetAsync(counter, 0, sizeof(int), c->stream);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k_rz_round, grid, wg, 0, c->stream, n, r, rzH, rzRank, rzSucc, cur, prev, next, counter);
            return hipGetLastError();
        });
        if (s != TF_OK) return s;
        TF_CHECK(hipMemcpyAsync(&left, counter, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        TF_CHECK(hipStreamSynchronize(c->stream));
    }
    return TF_OK;
}

// the validated file into a context of other capacities: the placement into scratch, the fit check, then the commit
// in scene_load's order.  TF_CAPACITY leaves the context as it was.
static tf_status scene_load_resized(tf_ctx* c, const unsigned char* data, const struct tf_map_file_info& minfo, const TfSceneLayout& lay,
                                    struct tf_resize_report* report)
{
    TfCtxMem tmp(c->mem.fns());
    unsigned char* rec_dev = nullptr;
    int *ptr_dev = nullptr, *sto_dev = nullptr, *rz = nullptr, *bid = nullptr, *tally = nullptr;
    int4* grp = nullptr;
    const struct tf_scene_file_info& info = minfo.scene;
    const int sw = minfo.version == (int)TF_MAP_VERSION;
    if (info.n_records > 0x7fffffffll / 4) return TF_INVALID_ARG;      // (a valid file has at most n_total of them)
    const int n = (int)info.n_records, ng = ck_groups(n), nbk = c->p.n_buckets;
    const size_t rec_bytes = (size_t)n * TF_SCENE_RECORD_BYTES;
    TF_CHECK(tfk_ckpt_scratch(c));
    TF_CHECK(tf_mem_hip(tmp.alloc(&rec_dev, rec_bytes)));
    TF_CHECK(tf_mem_hip(tmp.alloc(&ptr_dev, sizeof(int) * (size_t)info.n_blocks_stored)));
    TF_CHECK(tf_mem_hip(tmp.alloc(&sto_dev, sizeof(int) * (size_t)minfo.n_cache_blocks)));
    TF_CHECK(tf_mem_hip(tmp.alloc(&rz, sizeof(int) * 4 * (size_t)n)));             // h / ptr', rank, successor, t per record
    TF_CHECK(tf_mem_hip(tmp.alloc(&bid, sizeof(int) * 3 * (size_t)nbk)));          // the rounds' three bucket arrays
    TF_CHECK(tf_mem_hip(tmp.alloc(&grp, sizeof(int4) * (2 * (size_t)ng + 1))));    // the placement pass's scratch
    TF_CHECK(tf_mem_hip(tmp.alloc(&tally, sizeof(int) * 4)));                      // carried, carried with a stored block, left
    int *rzH = rz, *rzRank = rz + n, *rzSucc = rz + 2 * (size_t)n, *rzT = rz + 3 * (size_t)n;
    tf_status s = ckpt_h2d(c, rec_dev, data + lay.records_off, rec_bytes);
    if (s != TF_OK) return s;
    const ck_u2* rec = (const ck_u2*)rec_dev;
    const dim3 grid(ck_grid((size_t)n)), wg(CK_WG);
    int host_tally[4] = { 0, 0, 0, 0 };
    s = ck_timed_kernels(c, CK_T_INDEX, [&] {
        hipError_t e = hipMemsetAsync(bid, 0x7f, sizeof(int) * 3 * (size_t)nbk, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(tally, 0, sizeof(int) * 4, c->stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rz_hash, grid, wg, 0, c->stream, rec, n, (unsigned)(nbk - 1), sw, rzH, rzRank, rzSucc, bid, tally);
        return hipGetLastError();
    });
    if (s != TF_OK) return s;
    TF_CHECK(hipMemcpyAsync(host_tally, tally, sizeof(host_tally), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    int rounds = 0;
    s = ck_rank_rounds(c, n, host_tally[0], rzH, rzRank, rzSucc, bid, tally + 2, &rounds);
    if (s != TF_OK) return s;
    const CkRzPass place = { rec, rzRank, sw, nbk, c->p.n_excess, c->p.n_blocks, rzH, rzT, ptr_dev, sto_dev };
    s = ck_timed_kernels(c, CK_T_INDEX, [&] { return tfk_ck_count(c, place, n, grp); });
    if (s != TF_OK) return s;
    int4 totals;                                           // excess slots, active blocks, stored blocks in the file
    TF_CHECK(hipMemcpyAsync(&totals, grp + 2 * (size_t)ng, sizeof(totals), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    if (report) {
        report->records_carried = host_tally[0];
        report->records_dropped = (long long)n - host_tally[0];
        report->blocks = totals.y;
        report->cache_blocks = host_tally[1];
        report->excess_used = totals.x;
        report->longest_chain = rounds;
    }
    if (totals.y != info.n_blocks_stored || totals.z != minfo.n_cache_blocks) return TF_INVALID_ARG;      // (the validation's counts)
    if (totals.y > c->p.n_blocks || totals.x > c->p.n_excess) return TF_CAPACITY;
    // ---- the commit ----
    s = ckpt_clear_context(c, sw != 0);
    if (s != TF_OK) return s;
    s = ck_timed_kernels(c, CK_T_INDEX, [&] { return tfk_ck_emit(c, place, n, grp); });
    if (s != TF_OK) return s;
    s = ckpt_load_blocks(c, data, minfo, lay, ptr_dev, sto_dev, true);
    if (s != TF_OK) return s;
    const CkVisPass vis = { c->visType, c->p.vis_capacity, c->visibleIds };        // over the context's own group scratch
    s = ck_timed_kernels(c, CK_T_INDEX, [&] {
        hipLaunchKernelGGL(k_rz_apply, grid, wg, 0, c->stream, rec, n, sw, nbk, rzH, rzSucc, rzT, c->hash, c->visType, c->swapState,
                           c->swapFlags);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = tfk_grid_rebuild(c);
        if (e == hipSuccess) e = tfk_ck_count(c, vis, c->n_total, c->ckptGroup);
        return e == hipSuccess ? tfk_ck_emit(c, vis, c->n_total, c->ckptGroup) : e;
    });
    if (s != TF_OK) return s;
    int4 nvis;
    TF_CHECK(hipMemcpyAsync(&nvis, c->ckptGroup + 2 * (size_t)ck_groups(c->n_total), sizeof(nvis), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    return ckpt_load_finish(c, data, info, lay, c->p.n_blocks - 1 - totals.y, c->p.n_excess - 1 - totals.x,
                            nvis.x < c->p.vis_capacity ? nvis.x : c->p.vis_capacity);
}

// a checkpoint file read whole and validated (the file and check times of tf_scene_ckpt_times start here).  *data is
// the caller's to free whenever it is not null, also when the validation refused the file
static tf_status ckpt_read_file(tf_ctx* c, const char* path, double t_call, unsigned char** data, struct tf_map_file_info* minfo,
                                TfSceneLayout* lay)
{
    FILE* f = fopen(path, "rb");
    if (!f) return TF_INVALID_ARG;
    long long size = -1;
    if (fseeko(f, 0, SEEK_END) == 0) size = (long long)ftello(f);
    if (size < TF_SCENE_HEADER_BYTES || fseeko(f, 0, SEEK_SET) != 0) { fclose(f); return TF_INVALID_ARG; }    // (shorter than either header)
    memset(c->ckpt_ms, 0, sizeof(c->ckpt_ms));
    *data = (unsigned char*)malloc((size_t)size);
    if (!*data) { fclose(f); return TF_OOM; }
    const size_t got = fread(*data, 1, (size_t)size, f);
    fclose(f);
    c->ckpt_ms[CK_T_FILE] = ck_now_ms() - t_call;
    const double t_check = ck_now_ms();
    const tf_status s = got == (size_t)size ? tf_map_file_validate(*data, got, minfo, lay) : TF_INVALID_ARG;
    c->ckpt_ms[CK_T_CHECK] = ck_now_ms() - t_check;
    return s;
}

// tf_map_load, or with `resized` tf_map_load_resized: the capacities need not agree, the records are re-hashed
static tf_status map_load(tf_ctx* c, const char* path, bool resized, struct tf_resize_report* report)
{
    if (!c || !path) return TF_INVALID_ARG;
    {
        const tf_status s0 = sync_checked(c);
        if (s0 != TF_OK) return s0;
    }
    const double t_call = ck_now_ms();
    unsigned char* data = nullptr;
    struct tf_map_file_info minfo;
    TfSceneLayout lay;
    tf_status s = ckpt_read_file(c, path, t_call, &data, &minfo, &lay);
    if (s != TF_OK && !data) return s;
    if (s == TF_OK) {
        const tf_params& a = minfo.scene.params;
        const tf_params& b = c->p;
        // (a version-2 file has use_swapping == 1, a version-1 file 0: the layout's rule; the context's may be any non-zero value)
        if (a.cols != b.cols || a.rows != b.rows || a.voxel_rgb != b.voxel_rgb || (a.use_swapping != 0) != (b.use_swapping != 0) ||
            !bits_equal(a.voxelSize, b.voxelSize) || !bits_equal(a.mu, b.mu) || a.maxW != b.maxW)
            s = TF_INVALID_ARG;
        if (!resized && (a.n_buckets != b.n_buckets || a.n_excess != b.n_excess || a.n_blocks != b.n_blocks ||
                         minfo.scene.noVisibleEntries > b.vis_capacity))
            s = TF_INVALID_ARG;
    }
    if (s == TF_OK) s = resized ? scene_load_resized(c, data, minfo, lay, report) : scene_load(c, data, minfo, lay);
    free(data);
    c->ckpt_ms[CK_T_CALL] = ck_now_ms() - t_call;
    return s;
}

extern "C" tf_status tf_map_load(tf_ctx* c, const char* path)
{
    TF_FLUSH(c);
    return map_load(c, path, false, nullptr);
}

extern "C" tf_status tf_map_load_resized(tf_ctx* c, const char* path, struct tf_resize_report* report)
{
    TF_FLUSH(c);
    if (report) memset(report, 0, sizeof(*report));
    return map_load(c, path, true, report);
}

// the validated version-1 file into the live scene (DESIGN.md §5 Map merge): find, rank, count into scratch; the
// refusals; then the commit -- entries, links and grid cells, the blocks, the two counters.  Nothing before the
// commit writes the context.
static tf_status scene_merge(tf_ctx* c, const unsigned char* data, const struct tf_map_file_info& minfo, const TfSceneLayout& lay,
                             const int block_offset[3], struct tf_merge_report* report)
{
    TfCtxMem tmp(c->mem.fns());
    unsigned char* rec_dev = nullptr;
    int *mg = nullptr, *bid = nullptr, *tally = nullptr;
    unsigned* word = nullptr;
    int4* grp = nullptr;
    const struct tf_scene_file_info& info = minfo.scene;
    if (info.n_records > 0x7fffffffll / 8) return TF_INVALID_ARG;      // (a valid file has at most n_total of them)
    const int n = (int)info.n_records, ng = ck_groups(n), nbk = c->p.n_buckets;
    const size_t rec_bytes = (size_t)n * TF_SCENE_RECORD_BYTES;
    long long carried = 0;
    const double t_check = ck_now_ms();
    tf_status s = tf_merge_records_check(data + lay.records_off, n, block_offset, &carried);
    c->ckpt_ms[CK_T_CHECK] += ck_now_ms() - t_check;
    if (s != TF_OK) return s;
    if (carried != info.n_blocks_stored) return TF_INVALID_ARG;        // (the validation's count)
    s = sync_state(c);                                     // the live counters; TF_HIP_ERROR on a context in error
    if (s != TF_OK) return s;
    const int lastBlock = c->st_host->lastFreeBlockId, lastExcess = c->st_host->lastFreeExcessListId;
    if (lastBlock < -1 || lastBlock >= c->p.n_blocks || lastExcess < -1 || lastExcess >= c->p.n_excess) return TF_INVALID_ARG;     // (tf_set_counters)
    TF_CHECK(tfk_ckpt_scratch(c));
    TF_CHECK(tf_mem_hip(tmp.alloc(&rec_dev, rec_bytes)));
    TF_CHECK(tf_mem_hip(tmp.alloc(&mg, sizeof(int) * 8 * (size_t)n)));             // h, rank, successor, t, found, chain end, ptr', mode
    TF_CHECK(tf_mem_hip(tmp.alloc(&word, sizeof(unsigned) * (size_t)carried)));    // per block of the payload
    TF_CHECK(tf_mem_hip(tmp.alloc(&bid, sizeof(int) * 3 * (size_t)nbk)));          // the rounds' three bucket arrays
    TF_CHECK(tf_mem_hip(tmp.alloc(&grp, sizeof(int4) * (2 * (size_t)ng + 1))));    // the placement pass's scratch
    TF_CHECK(tf_mem_hip(tmp.alloc(&tally, sizeof(int) * MG_TALLY)));
    int *mgH = mg, *mgRank = mg + n, *mgSucc = mg + 2 * (size_t)n, *mgT = mg + 3 * (size_t)n, *mgFound = mg + 4 * (size_t)n,
        *mgEnd = mg + 5 * (size_t)n, *mgPtr = mg + 6 * (size_t)n, *mgMode = mg + 7 * (size_t)n;
    s = ckpt_h2d(c, rec_dev, data + lay.records_off, rec_bytes);
    if (s != TF_OK) return s;
    const ck_u2* rec = (const ck_u2*)rec_dev;
    const dim3 grid(ck_grid((size_t)n)), wg(CK_WG);
    const MgOffset off = { block_offset ? block_offset[0] : 0, block_offset ? block_offset[1] : 0, block_offset ? block_offset[2] : 0 };
    int host_tally[MG_TALLY];
    s = ck_timed_kernels(c, CK_T_INDEX, [&] {
        hipError_t e = hipMemsetAsync(bid, 0x7f, sizeof(int) * 3 * (size_t)nbk, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(tally, 0, sizeof(int) * MG_TALLY, c->stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_mg_find, grid, wg, 0, c->stream, rec, n, off, (const TfHashEntry*)c->hash, (unsigned)(nbk - 1), nbk, c->p.n_excess,
                           c->p.n_blocks, mgH, mgRank, mgSucc, mgFound, mgEnd, mgMode, bid, tally);
        return hipGetLastError();
    });
    if (s != TF_OK) return s;
    TF_CHECK(hipMemcpyAsync(host_tally, tally, sizeof(host_tally), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    if (host_tally[MG_BAD]) return TF_INVALID_ARG;         // a chain or a ptr of the live table leaves its table
    int rounds = 0;
    s = ck_rank_rounds(c, n, host_tally[MG_N_INSERT], mgH, mgRank, mgSucc, bid, tally + MG_LEFT, &rounds);
    if (s != TF_OK) return s;
    const CkMergePass place = { mgMode, mgRank, mgEnd, mgFound, mgH, c->hash, c->allocList, c->excessList, lastBlock, lastExcess, nbk,
                                c->p.n_excess, c->p.n_blocks, mgT, mgPtr, word, tally + MG_BAD };
    s = ck_timed_kernels(c, CK_T_INDEX, [&] { return tfk_ck_count(c, place, n, grp); });
    if (s != TF_OK) return s;
    int4 totals;                                           // excess slots, blocks, carried records
    TF_CHECK(hipMemcpyAsync(&totals, grp + 2 * (size_t)ng, sizeof(totals), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    if (totals.z != carried) return TF_INVALID_ARG;
    struct tf_merge_report rep;
    rep.records_combined = host_tally[MG_N_COMBINE];
    rep.records_inserted = host_tally[MG_N_INSERT];
    rep.records_revived = host_tally[MG_N_REVIVE];
    rep.records_skipped = (long long)n - carried;
    rep.blocks_used = totals.y;
    rep.excess_used = totals.x;
    if (totals.y > lastBlock + 1 || totals.x > lastExcess + 1) {
        if (report) *report = rep;
        return TF_CAPACITY;
    }
    s = ck_timed_kernels(c, CK_T_INDEX, [&] { return tfk_ck_emit(c, place, n, grp); });     // (scratch still)
    if (s != TF_OK) return s;
    TF_CHECK(hipMemcpyAsync(host_tally, tally, sizeof(host_tally), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    if (host_tally[MG_BAD]) return TF_INVALID_ARG;         // a free-list value outside its table
    // ---- the commit ----
    s = ck_timed_kernels(c, CK_T_INDEX, [&] {
        hipLaunchKernelGGL(k_mg_apply, grid, wg, 0, c->stream, rec, n, off, nbk, (const int*)mgMode, (const int*)mgRank, (const int*)mgSucc,
                           (const int*)mgEnd, (const int*)mgT, (const int*)mgPtr, c->hash, c->visType, c->bgrid);
        return hipGetLastError();
    });
    if (s != TF_OK) return s;
    s = ckpt_payload(c, carried, TF_SCENE_BLOCK_BYTES, nullptr, data + lay.blocks_off, [&](long long b0, int nb) {
        hipLaunchKernelGGL(k_mg_blocks, dim3(ck_grid((size_t)nb * 128)), dim3(CK_WG), 0, c->stream, (ck_u4*)c->vba, (const unsigned*)(word + b0), nb,
                           c->p.maxW, (const ck_u4*)c->ckptStage);
        return hipGetLastError();
    });
    if (s != TF_OK) return s;
    TfDevState* st = c->st_host;                           // (no frame ran since the sync above)
    st->lastFreeBlockId = lastBlock - totals.y;
    st->lastFreeExcessListId = lastExcess - totals.x;
    st->scene_external = 1;                                // as after a hash upload: every later reset clears everything
    TF_CHECK(hipMemcpyAsync(c->st, c->st_host, sizeof(TfDevState), hipMemcpyHostToDevice, c->stream));
    s = sync_checked(c);
    if (s == TF_OK && report) *report = rep;
    return s;
}

extern "C" tf_status tf_map_merge(tf_ctx* c, const char* path, const int block_offset[3], struct tf_merge_report* report)
{
    TF_FLUSH(c);
    if (report) memset(report, 0, sizeof(*report));
    if (!c || !path) return TF_INVALID_ARG;
    if (c->p.use_swapping || c->p.voxel_rgb) return TF_INVALID_ARG;
    {
        const tf_status s0 = sync_checked(c);
        if (s0 != TF_OK) return s0;
    }
    const double t_call = ck_now_ms();
    unsigned char* data = nullptr;
    struct tf_map_file_info minfo;
    TfSceneLayout lay;
    tf_status s = ckpt_read_file(c, path, t_call, &data, &minfo, &lay);
    if (s == TF_OK) {
        const tf_params& a = minfo.scene.params;
        if (minfo.version != (int)TF_SCENE_VERSION || a.use_swapping || a.voxel_rgb || !bits_equal(a.voxelSize, c->p.voxelSize) ||
            !bits_equal(a.mu, c->p.mu) || a.maxW != c->p.maxW)
            s = TF_INVALID_ARG;
    }
    if (s == TF_OK) s = scene_merge(c, data, minfo, lay, block_offset, report);
    free(data);
    c->ckpt_ms[CK_T_CALL] = ck_now_ms() - t_call;
    return s;
}

extern "C" tf_status tf_scene_load(tf_ctx* c, const char* path)
{
    if (c && c->p.use_swapping) {                          // (after the deferred frame's tail, as every entry point)
        TF_FLUSH(c);
        return TF_INVALID_ARG;
    }
    return tf_map_load(c, path);
}

extern "C" tf_status tf_scene_ckpt_times(tf_ctx* c, double ms[8])
{
    TF_FLUSH(c);
    if (!c || !ms) return TF_INVALID_ARG;
    memcpy(ms, c->ckpt_ms, sizeof(c->ckpt_ms));
    return TF_OK;
}
