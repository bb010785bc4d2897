// tf_scene_ckpt.hip -- scene checkpoints for gfx950 (an addition: the reference cannot save its map;
// DESIGN.md §5 Scene checkpoints, the file in tf_scene_file.h).  The scene is written in hash-entry order
// by the scheme the mesh passes use -- an ordered count, a prefix, an emit pass -- as plain launches on
// the context stream:
//
//   k_ckpt_count   : per 256-entry group the entries that get a record (HashEntry not ResetScene's, or
//                    visType != 0) and those of them with a stored block (ptr >= 0)
//   k_ckpt_prefix  : exclusive scan of the group counts (one workgroup: a group count per 256 entries)
//   k_ckpt_records : every record at its base (24 B, three 8-byte stores), and the stored blocks' ptr in
//                    record order -- the list the gather walks
//   k_ckpt_gather  : blocks [b0, b0 + nb) of that list from the VBA (and the colour plane) into the
//                    staging buffer, 16 B per lane: a wave instruction moves 1 KiB, contiguous on both
//                    sides inside a block; no atomics
//   k_ckpt_scatter : the reverse (load): staging -> ptr * 512
//   k_ckpt_apply   : hash[index], visType[index] from the records (the block grid is rebuilt after)
//
// The counts fit 32 bits (records <= n_total, blocks <= n_blocks), so the scan is a small kernel of its
// own over int2 group counts (8 B per 256 entries) rather than k_mesh_prefix over 64-bit per-entry
// counts, and shares no scratch with a mesh extraction.  No workgroup waits on another inside a grid.
//
// Map checkpoints (tf_map_save / tf_map_load, DESIGN.md §5 Map checkpoints) are the same calls; on a swapping
// context they write version 2 of the file with the k_map_* forms further down: the GlobalCache's swap state
// and stored flag in every record, the stored blocks gathered from store + index * 512 as a second payload.
//
// The resized load (tf_map_load_resized, DESIGN.md §5 Resized load) takes either version into a context of other
// capacities: the k_rz_* kernels below re-hash the records into the new table before the same scatters run.
#include "tf_host.h"
#include "tf_scene_file.h"

#include <chrono>
#include <vector>
#include <stdio.h>
#include <stdlib.h>

#define CK_WG 256
typedef unsigned ck_u4 __attribute__((ext_vector_type(4)));
typedef unsigned ck_u2 __attribute__((ext_vector_type(2)));

// does entry idx get a record, does the record carry a block; e: its four words
__device__ __forceinline__ void ck_classify(const TfHashEntry* __restrict__ hash, const unsigned char* __restrict__ visType, int idx,
                                            int n_total, ck_u4& e, unsigned& vis, bool& rec, bool& blk)
{
    e = ck_u4{ 0u, 0u, 0u, 0xfffffffeu };
    vis = 0;
    if (idx < n_total) {
        e = *reinterpret_cast<const ck_u4*>(hash + idx);
        vis = visType[idx];
    }
    rec = idx < n_total && ((e.x | e.y | e.z) != 0u || e.w != 0xfffffffeu || vis != 0u);
    blk = rec && (int)e.w >= 0;
}

__global__ __launch_bounds__(CK_WG) void k_ckpt_count(const TfHashEntry* __restrict__ hash, const unsigned char* __restrict__ visType,
                                                      int n_total, int n_blocks, int2* __restrict__ groupCnt, int* __restrict__ bad)
{
    __shared__ int2 wcnt[CK_WG / 64];
    const int t = threadIdx.x, ng = (n_total + CK_WG - 1) / CK_WG;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        ck_u4 e; unsigned vis; bool rec, blk;
        ck_classify(hash, visType, g * CK_WG + t, n_total, e, vis, rec, blk);
        if (blk && (int)e.w >= n_blocks) *bad = 1;            // a block outside the VBA (an uploaded table): not saveable
        const int nr = __popcll(__ballot(rec)), nb = __popcll(__ballot(blk));
        __syncthreads();
        if ((t & 63) == 0) wcnt[t >> 6] = make_int2(nr, nb);
        __syncthreads();
        if (t == 0) {
            int2 s = make_int2(0, 0);
            for (int w = 0; w < CK_WG / 64; ++w) { s.x += wcnt[w].x; s.y += wcnt[w].y; }
            groupCnt[g] = s;
        }
    }
}

// base[g] = sum of cnt[0, g), base[ng] = the totals.  One workgroup: thread t owns a contiguous slice.
__global__ __launch_bounds__(CK_WG) void k_ckpt_prefix(const int2* __restrict__ cnt, int ng, int2* __restrict__ base)
{
    __shared__ int2 part[CK_WG];
    const int t = threadIdx.x, per = (ng + CK_WG - 1) / CK_WG;
    const int first = min(t * per, ng), last = min(first + per, ng);
    int2 s = make_int2(0, 0);
    for (int g = first; g < last; ++g) { s.x += cnt[g].x; s.y += cnt[g].y; }
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int2 run = make_int2(0, 0);
        for (int k = 0; k < CK_WG; ++k) { const int2 v = part[k]; part[k] = run; run.x += v.x; run.y += v.y; }
        base[ng] = run;
    }
    __syncthreads();
    s = part[t];
    for (int g = first; g < last; ++g) { base[g] = s; s.x += cnt[g].x; s.y += cnt[g].y; }
}

__global__ __launch_bounds__(CK_WG) void k_ckpt_records(const TfHashEntry* __restrict__ hash, const unsigned char* __restrict__ visType,
                                                        int n_total, const int2* __restrict__ base, ck_u2* __restrict__ records,
                                                        int* __restrict__ blockPtr)
{
    __shared__ int2 wcnt[CK_WG / 64];
    const int t = threadIdx.x, ng = (n_total + CK_WG - 1) / CK_WG, lane = t & 63, w = t >> 6;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        const int idx = g * CK_WG + t;
        ck_u4 e; unsigned vis; bool rec, blk;
        ck_classify(hash, visType, idx, n_total, e, vis, rec, blk);
        const unsigned long long mr = __ballot(rec), mb = __ballot(blk), below = (1ull << lane) - 1ull;
        __syncthreads();
        if (lane == 0) wcnt[w] = make_int2(__popcll(mr), __popcll(mb));
        __syncthreads();
        int2 b = base[g];
        for (int k = 0; k < w; ++k) { b.x += wcnt[k].x; b.y += wcnt[k].y; }
        if (rec) {
            ck_u2* r = records + 3 * (size_t)(b.x + __popcll(mr & below));
            r[0] = ck_u2{ (unsigned)idx, e.x };
            r[1] = ck_u2{ e.y, e.z };
            r[2] = ck_u2{ e.w, vis };
        }
        if (blk) blockPtr[b.y + __popcll(mb & below)] = (int)e.w;
    }
}

// 16-byte unit u of the chunk: block u / U, unit u % U of it (U = 128, or 256 with colour: the block's
// voxels, then its colour words)
template <bool GATHER>
__device__ __forceinline__ void ck_copy(ck_u4* __restrict__ vba, ck_u4* __restrict__ rgb, const int* __restrict__ blockPtr,
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

__global__ __launch_bounds__(CK_WG) void k_ckpt_gather(const TfVoxel* vba, const unsigned* rgb, const int* __restrict__ blockPtr, int nb,
                                                       ck_u4* __restrict__ stage)
{
    ck_copy<true>((ck_u4*)vba, (ck_u4*)rgb, blockPtr, nb, stage);
}

__global__ __launch_bounds__(CK_WG) void k_ckpt_scatter(TfVoxel* vba, unsigned* rgb, const int* __restrict__ blockPtr, int nb,
                                                        const ck_u4* __restrict__ stage)
{
    ck_copy<false>((ck_u4*)vba, (ck_u4*)rgb, blockPtr, nb, (ck_u4*)stage);
}

__global__ __launch_bounds__(CK_WG) void k_ckpt_apply(const ck_u2* __restrict__ records, long long n_records, TfHashEntry* __restrict__ hash,
                                                      unsigned char* __restrict__ visType)
{
    for (long long k = (long long)blockIdx.x * CK_WG + threadIdx.x; k < n_records; k += (long long)gridDim.x * CK_WG) {
        const ck_u2 a = records[3 * k], b = records[3 * k + 1], c = records[3 * k + 2];
        *reinterpret_cast<ck_u4*>(hash + a.x) = ck_u4{ a.y, b.x, b.y, c.x };
        visType[a.x] = (unsigned char)c.y;
    }
}

// ---- the swapping forms (map checkpoints, version 2 of the file): the same passes with the GlobalCache's two
// bytes per entry in the record predicate and in the record, a third tally (entries with hasStoredData) from
// the same ballots, and a second list -- the entry indices of flagged records, in record order -- that the
// store's gather walks.  The version-1 kernels above are launched as they were.
// cache: swapState | hasStoredData << 8; sto: the entry's stored block is state
__device__ __forceinline__ void ck_classify_map(const TfHashEntry* __restrict__ hash, const unsigned char* __restrict__ visType,
                                                const unsigned char* __restrict__ swapState, const unsigned char* __restrict__ swapFlags,
                                                int idx, int n_total, ck_u4& e, unsigned& vis, unsigned& cache, bool& rec, bool& blk,
                                                bool& sto)
{
    ck_classify(hash, visType, idx, n_total, e, vis, rec, blk);
    cache = 0;
    if (idx < n_total) cache = (unsigned)swapState[idx] | (unsigned)swapFlags[idx] << 8;
    rec = rec || cache != 0u;                              // (blk implies rec already: ptr >= 0 is not ResetScene's)
    sto = (cache >> 8) != 0u;
}

__global__ __launch_bounds__(CK_WG) void k_map_count(const TfHashEntry* __restrict__ hash, const unsigned char* __restrict__ visType,
                                                     const unsigned char* __restrict__ swapState,
                                                     const unsigned char* __restrict__ swapFlags, int n_total, int n_blocks,
                                                     int4* __restrict__ groupCnt, int* __restrict__ bad)
{
    __shared__ int4 wcnt[CK_WG / 64];
    const int t = threadIdx.x, ng = (n_total + CK_WG - 1) / CK_WG;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        ck_u4 e; unsigned vis, cache; bool rec, blk, sto;
        ck_classify_map(hash, visType, swapState, swapFlags, g * CK_WG + t, n_total, e, vis, cache, rec, blk, sto);
        if (blk && (int)e.w >= n_blocks) *bad = 1;
        const int nr = __popcll(__ballot(rec)), nb = __popcll(__ballot(blk)), ns = __popcll(__ballot(sto));
        __syncthreads();
        if ((t & 63) == 0) wcnt[t >> 6] = make_int4(nr, nb, ns, 0);
        __syncthreads();
        if (t == 0) {
            int4 s = make_int4(0, 0, 0, 0);
            for (int w = 0; w < CK_WG / 64; ++w) { s.x += wcnt[w].x; s.y += wcnt[w].y; s.z += wcnt[w].z; }
            groupCnt[g] = s;
        }
    }
}

// k_ckpt_prefix over three counts (.w unused)
__global__ __launch_bounds__(CK_WG) void k_map_prefix(const int4* __restrict__ cnt, int ng, int4* __restrict__ base)
{
    __shared__ int4 part[CK_WG];
    const int t = threadIdx.x, per = (ng + CK_WG - 1) / CK_WG;
    const int first = min(t * per, ng), last = min(first + per, ng);
    int4 s = make_int4(0, 0, 0, 0);
    for (int g = first; g < last; ++g) { s.x += cnt[g].x; s.y += cnt[g].y; s.z += cnt[g].z; }
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int4 run = make_int4(0, 0, 0, 0);
        for (int k = 0; k < CK_WG; ++k) { const int4 v = part[k]; part[k] = run; run.x += v.x; run.y += v.y; run.z += v.z; }
        base[ng] = run;
    }
    __syncthreads();
    s = part[t];
    for (int g = first; g < last; ++g) { base[g] = s; s.x += cnt[g].x; s.y += cnt[g].y; s.z += cnt[g].z; }
}

__global__ __launch_bounds__(CK_WG) void k_map_records(const TfHashEntry* __restrict__ hash, const unsigned char* __restrict__ visType,
                                                       const unsigned char* __restrict__ swapState,
                                                       const unsigned char* __restrict__ swapFlags, int n_total,
                                                       const int4* __restrict__ base, ck_u2* __restrict__ records,
                                                       int* __restrict__ blockPtr, int* __restrict__ storedIdx)
{
    __shared__ int4 wcnt[CK_WG / 64];
    const int t = threadIdx.x, ng = (n_total + CK_WG - 1) / CK_WG, lane = t & 63, w = t >> 6;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        const int idx = g * CK_WG + t;
        ck_u4 e; unsigned vis, cache; bool rec, blk, sto;
        ck_classify_map(hash, visType, swapState, swapFlags, idx, n_total, e, vis, cache, rec, blk, sto);
        const unsigned long long mr = __ballot(rec), mb = __ballot(blk), ms = __ballot(sto), below = (1ull << lane) - 1ull;
        __syncthreads();
        if (lane == 0) wcnt[w] = make_int4(__popcll(mr), __popcll(mb), __popcll(ms), 0);
        __syncthreads();
        int4 b = base[g];
        for (int k = 0; k < w; ++k) { b.x += wcnt[k].x; b.y += wcnt[k].y; b.z += wcnt[k].z; }
        if (rec) {
            ck_u2* r = records + 3 * (size_t)(b.x + __popcll(mr & below));
            r[0] = ck_u2{ (unsigned)idx, e.x };
            r[1] = ck_u2{ e.y, e.z };
            r[2] = ck_u2{ e.w, vis | cache << 8 };         // visType, swapState, hasStoredData, 0
        }
        if (blk) blockPtr[b.y + __popcll(mb & below)] = (int)e.w;
        if (sto) storedIdx[b.z + __popcll(ms & below)] = idx;
    }
}

// blocks [0, nb) of the entry-index list between the GlobalCache's store and the staging buffer: ck_copy's
// shape (16 B per lane, a wave instruction per KiB, contiguous inside a block).  The store is indexed by hash
// entry, 2 KiB each, so the offset is formed in 64 bits (it passes 4 GiB above 2^21 entries); it is touched
// once, so its side is nontemporal too.
// SKIP (the resized load): a list value of -1 names no entry, its block stays in the staging buffer
template <bool GATHER, bool SKIP = false>
__device__ __forceinline__ void ck_copy_store(ck_u4* __restrict__ store, const int* __restrict__ storedIdx, int nb,
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

__global__ __launch_bounds__(CK_WG) void k_map_gather(const TfVoxel* store, const int* __restrict__ storedIdx, int nb,
                                                      ck_u4* __restrict__ stage)
{
    ck_copy_store<true>((ck_u4*)store, storedIdx, nb, stage);
}

__global__ __launch_bounds__(CK_WG) void k_map_scatter(TfVoxel* store, const int* __restrict__ storedIdx, int nb,
                                                       const ck_u4* __restrict__ stage)
{
    ck_copy_store<false>((ck_u4*)store, storedIdx, nb, (ck_u4*)stage);
}

// k_ckpt_apply with the two cache bytes (swapState / swapFlags were cleared over the whole table before)
__global__ __launch_bounds__(CK_WG) void k_map_apply(const ck_u2* __restrict__ records, long long n_records, TfHashEntry* __restrict__ hash,
                                                     unsigned char* __restrict__ visType, unsigned char* __restrict__ swapState,
                                                     unsigned char* __restrict__ swapFlags)
{
    for (long long k = (long long)blockIdx.x * CK_WG + threadIdx.x; k < n_records; k += (long long)gridDim.x * CK_WG) {
        const ck_u2 a = records[3 * k], b = records[3 * k + 1], c = records[3 * k + 2];
        *reinterpret_cast<ck_u4*>(hash + a.x) = ck_u4{ a.y, b.x, b.y, c.x };
        visType[a.x] = (unsigned char)c.y;
        swapState[a.x] = (unsigned char)(c.y >> 8);
        swapFlags[a.x] = (unsigned char)(c.y >> 16);
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
//   k_rz_count  : per 256 records those with m > 0, with ptr >= 0, with a stored block (dropped ones too: their
//                 blocks lie in the file's second payload); k_map_prefix scans them
//   k_rz_place  : t(j), ptr'(j), and the two lists the scatters walk: ptr' per active block, t (-1: a dropped
//                 record's, skipped) per stored block
//   k_rz_apply  : hash[t] = {pos, the successor's excess slot + 1, ptr'}, visType and the cache bytes at t
//   k_rz_vis_*  : the ascending entries with visType > 0, the first vis_capacity of them, by count / prefix / emit
//
// Everything up to k_rz_count writes scratch only: the fit is checked on its totals before the context is touched.
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

// does record j use an excess slot, hold a block, name a stored block (after the rounds)
__device__ __forceinline__ void rz_classify(const ck_u2* __restrict__ records, const int* __restrict__ rzRank, int j, int n, int sw,
                                            bool& exc, bool& blk, bool& sto)
{
    exc = blk = sto = false;
    if (j < n) {
        const ck_u2 c = records[3 * (size_t)j + 2];
        exc = rzRank[j] > 0;
        blk = (int)c.x >= 0;
        sto = sw && ((c.y >> 16) & 0xffu) != 0u;
    }
}

__global__ __launch_bounds__(CK_WG) void k_rz_count(const ck_u2* __restrict__ records, const int* __restrict__ rzRank, int n, int sw,
                                                    int4* __restrict__ groupCnt)
{
    __shared__ int4 wcnt[CK_WG / 64];
    const int t = threadIdx.x, ng = (n + CK_WG - 1) / CK_WG;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        bool exc, blk, sto;
        rz_classify(records, rzRank, g * CK_WG + t, n, sw, exc, blk, sto);
        const int ne = __popcll(__ballot(exc)), nb = __popcll(__ballot(blk)), ns = __popcll(__ballot(sto));
        __syncthreads();
        if ((t & 63) == 0) wcnt[t >> 6] = make_int4(ne, nb, ns, 0);
        __syncthreads();
        if (t == 0) {
            int4 s = make_int4(0, 0, 0, 0);
            for (int w = 0; w < CK_WG / 64; ++w) { s.x += wcnt[w].x; s.y += wcnt[w].y; s.z += wcnt[w].z; }
            groupCnt[g] = s;
        }
    }
}

// rzH becomes ptr'(j) (its h is spent once t is known); rzT[j] = -1 marks a dropped record
__global__ __launch_bounds__(CK_WG) void k_rz_place(const ck_u2* __restrict__ records, int n, int sw, const int4* __restrict__ base,
                                                    int n_buckets, int n_excess, int n_blocks, int* __restrict__ rzH,
                                                    const int* __restrict__ rzRank, int* __restrict__ rzT, int* __restrict__ blockPtr,
                                                    int* __restrict__ storedIdx)
{
    __shared__ int4 wcnt[CK_WG / 64];
    const int t = threadIdx.x, ng = (n + CK_WG - 1) / CK_WG, lane = t & 63, w = t >> 6;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        const int j = g * CK_WG + t;
        bool exc, blk, sto;
        rz_classify(records, rzRank, j, n, sw, exc, blk, sto);
        const unsigned long long me = __ballot(exc), mb = __ballot(blk), ms = __ballot(sto), below = (1ull << lane) - 1ull;
        __syncthreads();
        if (lane == 0) wcnt[w] = make_int4(__popcll(me), __popcll(mb), __popcll(ms), 0);
        __syncthreads();
        int4 b = base[g];
        for (int k = 0; k < w; ++k) { b.x += wcnt[k].x; b.y += wcnt[k].y; b.z += wcnt[k].z; }
        if (j < n) {
            const int h = rzH[j];
            const int at = h < 0 ? -1 : exc ? n_buckets + n_excess - 1 - (b.x + __popcll(me & below)) : h;
            const int ptr = blk ? n_blocks - 1 - (b.y + __popcll(mb & below)) : -1;
            rzT[j] = at;
            rzH[j] = ptr;
            if (blk) blockPtr[b.y + __popcll(mb & below)] = ptr;
            if (sto) storedIdx[b.z + __popcll(ms & below)] = at;
        }
    }
}

__global__ __launch_bounds__(CK_WG) void k_rz_apply(const ck_u2* __restrict__ records, int n, int sw, int n_buckets,
                                                    const int* __restrict__ rzPtr, const int* __restrict__ rzSucc,
                                                    const int* __restrict__ rzT, TfHashEntry* __restrict__ hash,
                                                    unsigned char* __restrict__ visType, unsigned char* __restrict__ swapState,
                                                    unsigned char* __restrict__ swapFlags)
{
    for (int j = blockIdx.x * CK_WG + threadIdx.x; j < n; j += gridDim.x * CK_WG) {
        const int at = rzT[j];
        if (at < 0) continue;
        const ck_u2 a = records[3 * (size_t)j], b = records[3 * (size_t)j + 1], c = records[3 * (size_t)j + 2];
        const int succ = rzSucc[j];
        const unsigned offset = succ >= 0 ? (unsigned)(rzT[succ] - n_buckets + 1) : 0u;
        *reinterpret_cast<ck_u4*>(hash + at) = ck_u4{ a.y, b.x & 0xffffu, offset, (unsigned)rzPtr[j] };
        visType[at] = (unsigned char)c.y;
        if (sw) {
            swapState[at] = (unsigned char)(c.y >> 8);
            swapFlags[at] = (unsigned char)(c.y >> 16);
        }
    }
}

__global__ __launch_bounds__(CK_WG) void k_rz_vis_count(const unsigned char* __restrict__ visType, int n_total, int2* __restrict__ groupCnt)
{
    __shared__ int wcnt[CK_WG / 64];
    const int t = threadIdx.x, ng = (n_total + CK_WG - 1) / CK_WG;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        const int idx = g * CK_WG + t;
        const int nv = __popcll(__ballot(idx < n_total && visType[idx] != 0));
        __syncthreads();
        if ((t & 63) == 0) wcnt[t >> 6] = nv;
        __syncthreads();
        if (t == 0) {
            int s = 0;
            for (int w = 0; w < CK_WG / 64; ++w) s += wcnt[w];
            groupCnt[g] = make_int2(s, 0);
        }
    }
}

__global__ __launch_bounds__(CK_WG) void k_rz_vis_emit(const unsigned char* __restrict__ visType, int n_total, const int2* __restrict__ base,
                                                       int capacity, int* __restrict__ visibleIds)
{
    __shared__ int wcnt[CK_WG / 64];
    const int t = threadIdx.x, ng = (n_total + CK_WG - 1) / CK_WG, lane = t & 63, w = t >> 6;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        const int idx = g * CK_WG + t;
        const bool v = idx < n_total && visType[idx] != 0;
        const unsigned long long mv = __ballot(v);
        __syncthreads();
        if (lane == 0) wcnt[w] = __popcll(mv);
        __syncthreads();
        int at = base[g].x + __popcll(mv & ((1ull << lane) - 1ull));
        for (int k = 0; k < w; ++k) at += wcnt[k];
        if (v && at < capacity) visibleIds[at] = idx;
    }
}

// k_map_scatter over a list in which -1 stands for a block that is not carried
__global__ __launch_bounds__(CK_WG) void k_rz_scatter_store(TfVoxel* store, const int* __restrict__ storedIdx, int nb,
                                                            const ck_u4* __restrict__ stage)
{
    ck_copy_store<false, true>((ck_u4*)store, storedIdx, nb, (ck_u4*)stage);
}

static int ck_groups(const tf_ctx* c) { return (c->n_total + CK_WG - 1) / CK_WG; }
static int ck_grid(size_t items) { const size_t g = (items + CK_WG - 1) / CK_WG; return (int)(g < 1 ? 1 : g > 2048 ? 2048 : g); }

// the context's checkpoint scratch, from the first call on: the group counts, their bases + totals and
// the "not saveable" flag; the device staging buffer and its pinned twin, ckpt_chunk_blocks blocks each
static hipError_t tfk_ckpt_scratch(tf_ctx* c)
{
    if (c->ckptGroup) return hipSuccess;
    const size_t ng = (size_t)ck_groups(c);
    const size_t stage = (size_t)c->ckpt_chunk_blocks * TF_SCENE_BLOCK_BYTES * (c->p.voxel_rgb ? 2 : 1);
    const size_t cnt = c->p.use_swapping ? sizeof(int4) : sizeof(int2);      // three tallies per group with the GlobalCache
    return tf_mem_hip(c->mem.alloc_group({ TfCtxMem::dev(&c->ckptGroup, cnt * (2 * ng + 2)), TfCtxMem::dev(&c->ckptStage, stage),
                                           TfCtxMem::pin(&c->ckptPinned, stage, hipHostMallocDefault) }));
}

static size_t tfk_ckpt_stage_bytes(const tf_ctx* c)
{
    return (size_t)c->ckpt_chunk_blocks * TF_SCENE_BLOCK_BYTES * (c->p.voxel_rgb ? 2 : 1);
}

// count + prefix; totals[0] = {records, blocks}, totals[1].x = the "not saveable" flag (device addresses)
static hipError_t tfk_ckpt_count(tf_ctx* c, const int2** totals)
{
    const int ng = ck_groups(c);
    int2* cnt = c->ckptGroup;
    int2* base = cnt + ng;
    int* bad = (int*)(base + ng + 1);
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int2), c->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ckpt_count, dim3(ck_grid((size_t)c->n_total)), dim3(CK_WG), 0, c->stream, c->hash, c->visType, c->n_total,
                       c->p.n_blocks, cnt, bad);
    hipLaunchKernelGGL(k_ckpt_prefix, dim3(1), dim3(CK_WG), 0, c->stream, cnt, ng, base);
    *totals = base + ng;
    return hipGetLastError();
}

// after tfk_ckpt_count: records (n_records x 24 B) and the stored blocks' ptr list, device buffers of the caller
static hipError_t tfk_ckpt_records(tf_ctx* c, void* records, int* blockPtr)
{
    hipLaunchKernelGGL(k_ckpt_records, dim3(ck_grid((size_t)c->n_total)), dim3(CK_WG), 0, c->stream, c->hash, c->visType, c->n_total,
                       c->ckptGroup + ck_groups(c), (ck_u2*)records, blockPtr);
    return hipGetLastError();
}

// nb <= ckpt_chunk_blocks blocks of the list into / out of the staging buffer
static hipError_t tfk_ckpt_gather(tf_ctx* c, const int* blockPtr, int nb)
{
    hipLaunchKernelGGL(k_ckpt_gather, dim3(ck_grid((size_t)nb * 256)), dim3(CK_WG), 0, c->stream, c->vba,
                       c->p.voxel_rgb ? c->vba_rgb : nullptr, blockPtr, nb, (ck_u4*)c->ckptStage);
    return hipGetLastError();
}

static hipError_t tfk_ckpt_scatter(tf_ctx* c, const int* blockPtr, int nb)
{
    hipLaunchKernelGGL(k_ckpt_scatter, dim3(ck_grid((size_t)nb * 256)), dim3(CK_WG), 0, c->stream, c->vba,
                       c->p.voxel_rgb ? c->vba_rgb : nullptr, blockPtr, nb, (const ck_u4*)c->ckptStage);
    return hipGetLastError();
}

static hipError_t tfk_ckpt_apply(tf_ctx* c, const void* records, long long n_records)
{
    if (n_records == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ckpt_apply, dim3(ck_grid((size_t)n_records)), dim3(CK_WG), 0, c->stream, (const ck_u2*)records, n_records, c->hash,
                       c->visType);
    return hipGetLastError();
}

// the swapping forms: totals[0] = {records, blocks, flagged, -}, totals[1].x = the "not saveable" flag
static hipError_t tfk_map_count(tf_ctx* c, const int4** totals)
{
    const int ng = ck_groups(c);
    int4* cnt = (int4*)c->ckptGroup;
    int4* base = cnt + ng;
    int* bad = (int*)(base + ng + 1);
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int4), c->stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_map_count, dim3(ck_grid((size_t)c->n_total)), dim3(CK_WG), 0, c->stream, c->hash, c->visType, c->swapState,
                       c->swapFlags, c->n_total, c->p.n_blocks, cnt, bad);
    hipLaunchKernelGGL(k_map_prefix, dim3(1), dim3(CK_WG), 0, c->stream, cnt, ng, base);
    *totals = base + ng;
    return hipGetLastError();
}

static hipError_t tfk_map_records(tf_ctx* c, void* records, int* blockPtr, int* storedIdx)
{
    hipLaunchKernelGGL(k_map_records, dim3(ck_grid((size_t)c->n_total)), dim3(CK_WG), 0, c->stream, c->hash, c->visType, c->swapState,
                       c->swapFlags, c->n_total, (const int4*)c->ckptGroup + ck_groups(c), (ck_u2*)records, blockPtr, storedIdx);
    return hipGetLastError();
}

// nb <= ckpt_chunk_blocks stored blocks of the entry list into / out of the staging buffer
static hipError_t tfk_map_gather(tf_ctx* c, const int* storedIdx, int nb)
{
    hipLaunchKernelGGL(k_map_gather, dim3(ck_grid((size_t)nb * 128)), dim3(CK_WG), 0, c->stream, c->swapStore, storedIdx, nb,
                       (ck_u4*)c->ckptStage);
    return hipGetLastError();
}

static hipError_t tfk_map_scatter(tf_ctx* c, const int* storedIdx, int nb, bool skip = false)
{
    hipLaunchKernelGGL(skip ? k_rz_scatter_store : k_map_scatter, dim3(ck_grid((size_t)nb * 128)), dim3(CK_WG), 0, c->stream, c->swapStore,
                       storedIdx, nb, (const ck_u4*)c->ckptStage);
    return hipGetLastError();
}

static hipError_t tfk_map_apply(tf_ctx* c, const void* records, long long n_records)
{
    if (n_records == 0) return hipSuccess;
    hipLaunchKernelGGL(k_map_apply, dim3(ck_grid((size_t)n_records)), dim3(CK_WG), 0, c->stream, (const ck_u2*)records, n_records, c->hash,
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

// `bytes` of device memory to the file through the pinned buffer, a staging chunk at a time
// (bound > 0: the bytes are a list of ints that must lie in [0, bound), as load will require)
static tf_status ckpt_d2h_write(tf_ctx* c, FILE* f, const void* dev, size_t bytes, int bound = 0)
{
    const size_t cap = tfk_ckpt_stage_bytes(c);
    for (size_t o = 0; o < bytes; o += cap) {
        const size_t n = bytes - o < cap ? bytes - o : cap;
        const double t0 = ck_now_ms();
        TF_CHECK(hipMemcpyAsync(c->ckptPinned, (const char*)dev + o, n, hipMemcpyDeviceToHost, c->stream));
        TF_CHECK(hipStreamSynchronize(c->stream));
        const double t1 = ck_now_ms();
        if (bound > 0 && !tf_scene_list_within(c->ckptPinned, n / 4, bound)) return TF_INVALID_ARG;
        if (fwrite(c->ckptPinned, 1, n, f) != n) return TF_INVALID_ARG;
        c->ckpt_ms[CK_T_COPY] += t1 - t0;
        c->ckpt_ms[CK_T_FILE] += ck_now_ms() - t1;
    }
    return TF_OK;
}

// ... and host bytes to device memory the same way
static tf_status ckpt_h2d(tf_ctx* c, void* dev, const unsigned char* host, size_t bytes)
{
    const size_t cap = tfk_ckpt_stage_bytes(c);
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
    if (sw) {
        const int4* totals_dev = nullptr;
        s = ck_timed_kernels(c, CK_T_INDEX, [&] { return tfk_map_count(c, &totals_dev); });
        if (s != TF_OK) return s;
        int4 totals[2];
        TF_CHECK(hipMemcpyAsync(totals, totals_dev, sizeof(totals), hipMemcpyDeviceToHost, c->stream));
        TF_CHECK(hipStreamSynchronize(c->stream));
        if (totals[1].x) return TF_INVALID_ARG;
        info.n_records = totals[0].x;
        info.n_blocks_stored = totals[0].y;
        minfo.n_cache_blocks = totals[0].z;
    } else {
        const int2* totals_dev = nullptr;
        s = ck_timed_kernels(c, CK_T_INDEX, [&] { return tfk_ckpt_count(c, &totals_dev); });
        if (s != TF_OK) return s;
        int2 totals[2];
        TF_CHECK(hipMemcpyAsync(totals, totals_dev, sizeof(totals), hipMemcpyDeviceToHost, c->stream));
        TF_CHECK(hipStreamSynchronize(c->stream));
        if (totals[1].x) return TF_INVALID_ARG;            // an entry's ptr lies outside the VBA (uploaded tables)
        info.n_records = totals[0].x;
        info.n_blocks_stored = totals[0].y;
    }
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
    s = ck_timed_kernels(c, CK_T_INDEX, [&] { return sw ? tfk_map_records(c, rec_dev, ptr_dev, sto_dev) : tfk_ckpt_records(c, rec_dev, ptr_dev); });
    if (s != TF_OK) return s;
    {   // the record table: to the host whole (24 B per record), checked by load's own rule before any block
        // moves -- chain offsets, duplicate ptr (tables that came through tf_upload) -- then summed and written
        std::vector<unsigned char> rec(rec_bytes);
        double t0 = ck_now_ms();
        const size_t cap = tfk_ckpt_stage_bytes(c);
        for (size_t o = 0; o < rec_bytes; o += cap) {
            const size_t n = rec_bytes - o < cap ? rec_bytes - o : cap;
            TF_CHECK(hipMemcpyAsync(c->ckptPinned, (const char*)rec_dev + o, n, hipMemcpyDeviceToHost, c->stream));
            TF_CHECK(hipStreamSynchronize(c->stream));
            memcpy(rec.data() + o, c->ckptPinned, n);
        }
        double t1 = ck_now_ms();
        c->ckpt_ms[CK_T_COPY] += t1 - t0;
        s = sw ? tf_map_records_check(rec.data(), info.n_records, &info.params, info.n_blocks_stored, minfo.n_cache_blocks)
               : tf_scene_records_check(rec.data(), info.n_records, &info.params, info.n_blocks_stored);
        if (s != TF_OK) return s;
        records_crc = tf_scene_crc32(0u, rec.data(), rec_bytes);
        t0 = ck_now_ms();
        c->ckpt_ms[CK_T_CHECK] += t0 - t1;
        if (fwrite(rec.data(), 1, rec_bytes, f) != rec_bytes) return TF_INVALID_ARG;
        c->ckpt_ms[CK_T_FILE] += ck_now_ms() - t0;
    }
    for (long long b0 = 0; b0 < info.n_blocks_stored && s == TF_OK; b0 += c->ckpt_chunk_blocks) {
        const int nb = (int)(info.n_blocks_stored - b0 < c->ckpt_chunk_blocks ? info.n_blocks_stored - b0 : c->ckpt_chunk_blocks);
        s = ck_timed_kernels(c, CK_T_BLOCKS, [&] { return tfk_ckpt_gather(c, ptr_dev + b0, nb); });
        if (s == TF_OK) s = ckpt_d2h_write(c, f, c->ckptStage, (size_t)nb * lay.block_bytes);
        c->ckpt_ms[CK_T_BLOCK_BYTES] += 2.0 * (double)nb * (double)lay.block_bytes;     // read + written
    }
    for (long long b0 = 0; b0 < minfo.n_cache_blocks && s == TF_OK; b0 += c->ckpt_chunk_blocks) {      // the GlobalCache's
        const int nb = (int)(minfo.n_cache_blocks - b0 < c->ckpt_chunk_blocks ? minfo.n_cache_blocks - b0 : c->ckpt_chunk_blocks);
        s = ck_timed_kernels(c, CK_T_BLOCKS, [&] { return tfk_map_gather(c, sto_dev + b0, nb); });
        if (s == TF_OK) s = ckpt_d2h_write(c, f, c->ckptStage, (size_t)nb * TF_SCENE_BLOCK_BYTES);
        c->ckpt_ms[CK_T_BLOCK_BYTES] += 2.0 * (double)nb * (double)TF_SCENE_BLOCK_BYTES;
    }
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

// the two halves every load ends with (below scene_load)
static tf_status ckpt_load_blocks(tf_ctx* c, const unsigned char* data, const struct tf_map_file_info& minfo, const TfSceneLayout& lay,
                                  const int* ptr_dev, const int* sto_dev, bool skip);
static tf_status ckpt_load_finish(tf_ctx* c, const unsigned char* data, const struct tf_scene_file_info& info, const TfSceneLayout& lay,
                                  int lastFreeBlockId, int lastFreeExcessListId, int noVisibleEntries);

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
    TF_CHECK(tfk_reset_scene(c));                          // full: hash, VBA, colour, both lists (identity), block grid cells
    TF_CHECK(hipMemsetAsync(c->visType, 0, (size_t)c->n_total, c->stream));
    if (sw) {   // the loader's own states and flags of entries the file does not name must not survive; the store
                // itself is not cleared: a stored block whose flag is 0 is read by nobody
        TF_CHECK(hipMemsetAsync(c->swapState, 0, (size_t)c->n_total, c->stream));
        TF_CHECK(hipMemsetAsync(c->swapFlags, 0, (size_t)c->n_total, c->stream));
    }
    const size_t rec_bytes = (size_t)info.n_records * TF_SCENE_RECORD_BYTES;
    TF_CHECK(tf_mem_hip(tmp.alloc(&rec_dev, rec_bytes)));
    TF_CHECK(tf_mem_hip(tmp.alloc(&ptr_dev, sizeof(int) * (size_t)info.n_blocks_stored)));
    tf_status s = ckpt_h2d(c, rec_dev, data + lay.records_off, rec_bytes);
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
        const hipError_t e = sw ? tfk_map_apply(c, rec_dev, info.n_records) : tfk_ckpt_apply(c, rec_dev, info.n_records);
        return e == hipSuccess ? tfk_grid_rebuild(c) : e;
    });
    if (s != TF_OK) return s;
    s = ckpt_h2d(c, c->visibleIds, data + lay.vis_off, 4 * lay.n_vis);
    if (s == TF_OK) s = ckpt_h2d(c, c->allocList, data + lay.alloc_off, 4 * lay.n_alloc);
    if (s == TF_OK) s = ckpt_h2d(c, c->excessList, data + lay.excess_off, 4 * lay.n_excess);
    if (s != TF_OK) return s;
    return ckpt_load_finish(c, data, info, lay, info.lastFreeBlockId, info.lastFreeExcessListId, info.noVisibleEntries);
}

// the file's two block payloads through the staging buffer to where the lists say: active blocks to ptr * 512 (and
// the colour plane), stored ones to store + entry * 512 (`skip`: -1 in that list names no entry)
static tf_status ckpt_load_blocks(tf_ctx* c, const unsigned char* data, const struct tf_map_file_info& minfo, const TfSceneLayout& lay,
                                  const int* ptr_dev, const int* sto_dev, bool skip)
{
    const struct tf_scene_file_info& info = minfo.scene;
    tf_status s = TF_OK;
    for (long long b0 = 0; b0 < info.n_blocks_stored; b0 += c->ckpt_chunk_blocks) {
        const int nb = (int)(info.n_blocks_stored - b0 < c->ckpt_chunk_blocks ? info.n_blocks_stored - b0 : c->ckpt_chunk_blocks);
        s = ckpt_h2d(c, c->ckptStage, data + lay.blocks_off + (size_t)b0 * lay.block_bytes, (size_t)nb * lay.block_bytes);
        if (s != TF_OK) return s;
        s = ck_timed_kernels(c, CK_T_BLOCKS, [&] { return tfk_ckpt_scatter(c, ptr_dev + b0, nb); });   // (waited for: the
        if (s != TF_OK) return s;                                                                          // staging buffer is free again)
        c->ckpt_ms[CK_T_BLOCK_BYTES] += 2.0 * (double)nb * (double)lay.block_bytes;
    }
    for (long long b0 = 0; b0 < minfo.n_cache_blocks; b0 += c->ckpt_chunk_blocks) {        // the GlobalCache's, to store + index * 512
        const int nb = (int)(minfo.n_cache_blocks - b0 < c->ckpt_chunk_blocks ? minfo.n_cache_blocks - b0 : c->ckpt_chunk_blocks);
        s = ckpt_h2d(c, c->ckptStage, data + lay.stored_off + (size_t)b0 * TF_SCENE_BLOCK_BYTES, (size_t)nb * TF_SCENE_BLOCK_BYTES);
        if (s != TF_OK) return s;
        s = ck_timed_kernels(c, CK_T_BLOCKS, [&] { return tfk_map_scatter(c, sto_dev + b0, nb, skip); });
        if (s != TF_OK) return s;
        c->ckpt_ms[CK_T_BLOCK_BYTES] += 2.0 * (double)nb * (double)TF_SCENE_BLOCK_BYTES;
    }
    return TF_OK;
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
    st->frame_counter = info.frame_counter;
    // the free lists and the blocks in use need not be what frames alone leave (a scene that came
    // through tf_upload): every later reset clears everything (tf_reset.h)
    st->scene_external = 1;
    TF_CHECK(hipMemcpyAsync(c->st, c->st_host, sizeof(TfDevState), hipMemcpyHostToDevice, c->stream));
    s = sync_checked(c);
    if (s == TF_OK) c->frame_counter = info.frame_counter;
    return s;
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
    const int n = (int)info.n_records, ng = (n + CK_WG - 1) / CK_WG, nbk = c->p.n_buckets;
    const size_t rec_bytes = (size_t)n * TF_SCENE_RECORD_BYTES;
    TF_CHECK(tfk_ckpt_scratch(c));
    TF_CHECK(tf_mem_hip(tmp.alloc(&rec_dev, rec_bytes)));
    TF_CHECK(tf_mem_hip(tmp.alloc(&ptr_dev, sizeof(int) * (size_t)info.n_blocks_stored)));
    TF_CHECK(tf_mem_hip(tmp.alloc(&sto_dev, sizeof(int) * (size_t)minfo.n_cache_blocks)));
    TF_CHECK(tf_mem_hip(tmp.alloc(&rz, sizeof(int) * 4 * (size_t)n)));             // h / ptr', rank, successor, t per record
    TF_CHECK(tf_mem_hip(tmp.alloc(&bid, sizeof(int) * 3 * (size_t)nbk)));          // the rounds' three bucket arrays
    TF_CHECK(tf_mem_hip(tmp.alloc(&grp, sizeof(int4) * (2 * (size_t)ng + 1))));
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
    for (int left = host_tally[0]; left > 0; ++rounds) {   // a round ranks one record of every bucket that has any left
        int* cur = bid + (size_t)(rounds % 3) * nbk;
        int* prev = bid + (size_t)((rounds + 2) % 3) * nbk;
        int* next = bid + (size_t)((rounds + 1) % 3) * nbk;
        s = ck_timed_kernels(c, CK_T_INDEX, [&] {
            const hipError_t e = hipMemsetAsync(tally + 2, 0, sizeof(int), c->stream);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k_rz_round, grid, wg, 0, c->stream, n, rounds, rzH, rzRank, rzSucc, cur, prev, next, tally + 2);
            return hipGetLastError();
        });
        if (s != TF_OK) return s;
        TF_CHECK(hipMemcpyAsync(&left, tally + 2, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        TF_CHECK(hipStreamSynchronize(c->stream));
    }
    s = ck_timed_kernels(c, CK_T_INDEX, [&] {
        hipLaunchKernelGGL(k_rz_count, grid, wg, 0, c->stream, rec, rzRank, n, sw, grp);
        hipLaunchKernelGGL(k_map_prefix, dim3(1), wg, 0, c->stream, grp, ng, grp + ng);
        return hipGetLastError();
    });
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
    TF_CHECK(tfk_reset_scene(c));                          // full: hash, VBA, colour, both lists (identity), block grid cells
    TF_CHECK(hipMemsetAsync(c->visType, 0, (size_t)c->n_total, c->stream));
    if (sw) {
        TF_CHECK(hipMemsetAsync(c->swapState, 0, (size_t)c->n_total, c->stream));
        TF_CHECK(hipMemsetAsync(c->swapFlags, 0, (size_t)c->n_total, c->stream));
    }
    s = ck_timed_kernels(c, CK_T_INDEX, [&] {
        hipLaunchKernelGGL(k_rz_place, grid, wg, 0, c->stream, rec, n, sw, (const int4*)(grp + ng), nbk, c->p.n_excess, c->p.n_blocks, rzH,
                           rzRank, rzT, ptr_dev, sto_dev);
        return hipGetLastError();
    });
    if (s != TF_OK) return s;
    s = ckpt_load_blocks(c, data, minfo, lay, ptr_dev, sto_dev, true);
    if (s != TF_OK) return s;
    int2* vcnt = (int2*)c->ckptGroup;                      // the context's own group scratch: a count per 256 entries
    const int ngt = ck_groups(c);
    s = ck_timed_kernels(c, CK_T_INDEX, [&] {
        hipLaunchKernelGGL(k_rz_apply, grid, wg, 0, c->stream, rec, n, sw, nbk, rzH, rzSucc, rzT, c->hash, c->visType, c->swapState,
                           c->swapFlags);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = tfk_grid_rebuild(c);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rz_vis_count, dim3(ck_grid((size_t)c->n_total)), wg, 0, c->stream, c->visType, c->n_total, vcnt);
        hipLaunchKernelGGL(k_ckpt_prefix, dim3(1), wg, 0, c->stream, vcnt, ngt, vcnt + ngt);
        hipLaunchKernelGGL(k_rz_vis_emit, dim3(ck_grid((size_t)c->n_total)), wg, 0, c->stream, c->visType, c->n_total, vcnt + ngt,
                           c->p.vis_capacity, c->visibleIds);
        return hipGetLastError();
    });
    if (s != TF_OK) return s;
    int2 nvis;
    TF_CHECK(hipMemcpyAsync(&nvis, vcnt + 2 * (size_t)ngt, sizeof(nvis), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    return ckpt_load_finish(c, data, info, lay, c->p.n_blocks - 1 - totals.y, c->p.n_excess - 1 - totals.x,
                            nvis.x < c->p.vis_capacity ? nvis.x : c->p.vis_capacity);
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
    FILE* f = fopen(path, "rb");
    if (!f) return TF_INVALID_ARG;
    long long size = -1;
    if (fseeko(f, 0, SEEK_END) == 0) size = (long long)ftello(f);
    if (size < TF_SCENE_HEADER_BYTES || fseeko(f, 0, SEEK_SET) != 0) { fclose(f); return TF_INVALID_ARG; }    // (shorter than either header)
    memset(c->ckpt_ms, 0, sizeof(c->ckpt_ms));
    unsigned char* data = (unsigned char*)malloc((size_t)size);
    if (!data) { fclose(f); return TF_OOM; }
    const size_t got = fread(data, 1, (size_t)size, f);
    fclose(f);
    c->ckpt_ms[CK_T_FILE] = ck_now_ms() - t_call;
    struct tf_map_file_info minfo;
    TfSceneLayout lay;
    const double t_check = ck_now_ms();
    tf_status s = got == (size_t)size ? tf_map_file_validate(data, got, &minfo, &lay) : TF_INVALID_ARG;
    c->ckpt_ms[CK_T_CHECK] = ck_now_ms() - t_check;
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
