// tf_compact.h -- the ordered compaction of the checkpoint passes (tf_scene_ckpt.hip) and of a free view's
// visible list (tf_view.hip): a count per 256 items, a prefix, an emit pass, as plain launches on the context
// stream.  No atomics, and no workgroup waits on another inside a grid.
//
//   k_ck_pass<false, P> : per 256-item group how many items take a place in each of pass P's (up to three) lists
//   k_ck_prefix         : exclusive scan of the group counts (one workgroup: a count per 256 items) + the totals
//   k_ck_pass<true, P>  : every item with its place in each list -- the group's base, the waves before, the lanes below
//
// The counts fit 32 bits, so the scan is a small kernel over int4 group counts (16 B per 256 items, the fourth lane
// zero; a pass with fewer lists leaves the others zero).  Included by each translation unit that has a pass: the
// kernels are templates or static, one copy per unit.
#pragma once
#include "tf_internal.h"

#define CK_WG 256

// A pass P names its items 0 .. n - 1 and gives
//   unsigned P::classify(i, i < n, item) : bit q set -- item i takes a place in list q (0 for i >= n); `item` is what
//                                          emit needs of it again
//   void P::emit(i, item, bits, at0, at1, at2) : for every i < n; at_q is the number of items below i with bit q
// The skeleton owns the ballots, the per-wave tally in LDS and its two barriers (the first ends the previous group's
// reads of the tally), the group count (count mode: grp[g]) and base + waves before + lanes below (emit mode: the
// bases stand behind the counts, grp[ng + g]).  All 256 threads of a group reach both barriers.
__device__ __forceinline__ void ck_add(int4& s, const int4 v) { s.x += v.x; s.y += v.y; s.z += v.z; }

template <bool EMIT, class Pass>
__global__ __launch_bounds__(CK_WG) void k_ck_pass(const Pass p, int n, int4* __restrict__ grp)
{
    __shared__ int4 wcnt[CK_WG / 64];
    const int t = threadIdx.x, ng = (n + CK_WG - 1) / CK_WG, lane = t & 63, w = t >> 6;
    for (int g = blockIdx.x; g < ng; g += gridDim.x) {
        const int i = g * CK_WG + t;
        typename Pass::Item item;
        const unsigned bits = p.classify(i, i < n, item);
        const unsigned long long m0 = __ballot(bits & 1u), m1 = __ballot(bits & 2u), m2 = __ballot(bits & 4u);
        __syncthreads();
        if (lane == 0) wcnt[w] = make_int4(__popcll(m0), __popcll(m1), __popcll(m2), 0);
        __syncthreads();
        if (!EMIT) {
            if (t == 0) {
                int4 s = make_int4(0, 0, 0, 0);
                for (int k = 0; k < CK_WG / 64; ++k) ck_add(s, wcnt[k]);
                grp[g] = s;
            }
        } else {
            int4 b = grp[ng + g];
            for (int k = 0; k < w; ++k) ck_add(b, wcnt[k]);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (i < n) p.emit(i, item, bits, b.x + __popcll(m0 & below), b.y + __popcll(m1 & below), b.z + __popcll(m2 & below));
        }
    }
}

// base[g] = sum of cnt[0, g), base[ng] = the totals.  One workgroup: thread t owns a contiguous slice.
static __global__ __launch_bounds__(CK_WG) void k_ck_prefix(const int4* __restrict__ cnt, int ng, int4* __restrict__ base)
{
    __shared__ int4 part[CK_WG];
    const int t = threadIdx.x, per = (ng + CK_WG - 1) / CK_WG;
    const int first = min(t * per, ng), last = min(first + per, ng);
    int4 s = make_int4(0, 0, 0, 0);
    for (int g = first; g < last; ++g) ck_add(s, cnt[g]);
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int4 run = make_int4(0, 0, 0, 0);
        for (int k = 0; k < CK_WG; ++k) { const int4 v = part[k]; part[k] = run; ck_add(run, v); }
        base[ng] = run;
    }
    __syncthreads();
    s = part[t];
    for (int g = first; g < last; ++g) { base[g] = s; ck_add(s, cnt[g]); }
}

// ---- the launchers -----------------------------------------------------------------------------------
static inline int ck_groups(int n) { return (n + CK_WG - 1) / CK_WG; }
// grid-stride over the groups: at most 2048 workgroups (8 per CU of the device), whatever n is
static inline int ck_grid(size_t items) { const size_t g = (items + CK_WG - 1) / CK_WG; return (int)(g < 1 ? 1 : g > 2048 ? 2048 : g); }

// a pass over n items with its scratch grp: [0, ng) the group counts, [ng, 2 ng] their bases and the totals.
// count + prefix (nothing but grp is written); then, once the caller has seen the totals, emit
template <class Pass>
static hipError_t tfk_ck_count(tf_ctx* c, const Pass& p, int n, int4* grp)
{
    hipLaunchKernelGGL((k_ck_pass<false, Pass>), dim3(ck_grid((size_t)n)), dim3(CK_WG), 0, c->stream, p, n, grp);
    hipLaunchKernelGGL(k_ck_prefix, dim3(1), dim3(CK_WG), 0, c->stream, (const int4*)grp, ck_groups(n), grp + ck_groups(n));
    return hipGetLastError();
}

template <class Pass>
static hipError_t tfk_ck_emit(tf_ctx* c, const Pass& p, int n, int4* grp)
{
    hipLaunchKernelGGL((k_ck_pass<true, Pass>), dim3(ck_grid((size_t)n)), dim3(CK_WG), 0, c->stream, p, n, grp);
    return hipGetLastError();
}
