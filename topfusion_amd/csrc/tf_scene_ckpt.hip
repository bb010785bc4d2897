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
#include "tf_internal.h"
#include "tf_scene_file.h"

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

static int ck_groups(const tf_ctx* c) { return (c->n_total + CK_WG - 1) / CK_WG; }
static int ck_grid(size_t items) { const size_t g = (items + CK_WG - 1) / CK_WG; return (int)(g < 1 ? 1 : g > 2048 ? 2048 : g); }

// the context's checkpoint scratch, from the first call on: the group counts, their bases + totals and
// the "not saveable" flag; the device staging buffer and its pinned twin, ckpt_chunk_blocks blocks each
hipError_t tfk_ckpt_scratch(tf_ctx* c)
{
    if (c->ckptGroup) return hipSuccess;
    const size_t ng = (size_t)ck_groups(c);
    const size_t stage = (size_t)c->ckpt_chunk_blocks * TF_SCENE_BLOCK_BYTES * (c->p.voxel_rgb ? 2 : 1);
    hipError_t e = hipMalloc((void**)&c->ckptGroup, sizeof(int2) * (2 * ng + 2));
    if (e == hipSuccess) e = hipMalloc((void**)&c->ckptStage, stage);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->ckptPinned, stage, hipHostMallocDefault);
    if (e != hipSuccess) {
        if (c->ckptGroup) (void)hipFree(c->ckptGroup);
        if (c->ckptStage) (void)hipFree(c->ckptStage);
        c->ckptGroup = nullptr; c->ckptStage = nullptr; c->ckptPinned = nullptr;
    }
    return e;
}

size_t tfk_ckpt_stage_bytes(const tf_ctx* c)
{
    return (size_t)c->ckpt_chunk_blocks * TF_SCENE_BLOCK_BYTES * (c->p.voxel_rgb ? 2 : 1);
}

// count + prefix; totals[0] = {records, blocks}, totals[1].x = the "not saveable" flag (device addresses)
hipError_t tfk_ckpt_count(tf_ctx* c, const int2** totals)
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
hipError_t tfk_ckpt_records(tf_ctx* c, void* records, int* blockPtr)
{
    hipLaunchKernelGGL(k_ckpt_records, dim3(ck_grid((size_t)c->n_total)), dim3(CK_WG), 0, c->stream, c->hash, c->visType, c->n_total,
                       c->ckptGroup + ck_groups(c), (ck_u2*)records, blockPtr);
    return hipGetLastError();
}

// nb <= ckpt_chunk_blocks blocks of the list into / out of the staging buffer
hipError_t tfk_ckpt_gather(tf_ctx* c, const int* blockPtr, int nb)
{
    hipLaunchKernelGGL(k_ckpt_gather, dim3(ck_grid((size_t)nb * 256)), dim3(CK_WG), 0, c->stream, c->vba,
                       c->p.voxel_rgb ? c->vba_rgb : nullptr, blockPtr, nb, (ck_u4*)c->ckptStage);
    return hipGetLastError();
}

hipError_t tfk_ckpt_scatter(tf_ctx* c, const int* blockPtr, int nb)
{
    hipLaunchKernelGGL(k_ckpt_scatter, dim3(ck_grid((size_t)nb * 256)), dim3(CK_WG), 0, c->stream, c->vba,
                       c->p.voxel_rgb ? c->vba_rgb : nullptr, blockPtr, nb, (const ck_u4*)c->ckptStage);
    return hipGetLastError();
}

hipError_t tfk_ckpt_apply(tf_ctx* c, const void* records, long long n_records)
{
    if (n_records == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ckpt_apply, dim3(ck_grid((size_t)n_records)), dim3(CK_WG), 0, c->stream, (const ck_u2*)records, n_records, c->hash,
                       c->visType);
    return hipGetLastError();
}
