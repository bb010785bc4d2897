// tf_view.hip -- free views for gfx950 (DESIGN.md §5 Free views): a second render state bound to a context, with
// its own size, visible list, range image, raycast result, image, expected-depth scratch and device state block,
// so that the map can be looked at from any pose, at any size, without a trace in the tracker's state.
//
// The one new kernel path is VisualisationEngine::FindVisibleBlocks (buildCompleteVisibleList_device,
// VisualisationHelper.cu:17-50): the scan of the whole hash for allocated blocks that project into the view.  The
// reference appends with an atomic counter, so its order is a race; here the list is in ascending entry order, by
// the ordered compaction of tf_compact.h:
//
//   k_ck_pass<false, ViewScanPass> : one hash entry per lane, loaded as one 16-byte vector (a wave reads 1 KiB,
//                                    contiguous).  Most entries end at ptr < 0 after that load; a wave with no live
//                                    entry skips the projections together, the others run vis_block (tf_vis.h:
//                                    checkBlockVisibility<false>, the plain frustum) for their live lanes.  The
//                                    wave's ballot is kept (8 B per 64 entries) and the group counts go to the scan.
//   k_ck_prefix                    : the exclusive scan of the group counts + the total.  The host reads the total:
//                                    past vis_capacity nothing more runs and the view's buffers stay as they were.
//   k_ck_pass<true, ViewEmitPass>  : reads the kept ballots (1/128 of the table's bytes), not the table again, and
//                                    writes every visible entry's index at its place.
//
// The grid is ck_grid's: a grid-stride over the 256-entry groups with at most 2048 workgroups (8 per CU), whatever
// the table's size.  No atomics.  Expected depths, the raycast, the pixel stages and renderICP are tf_render.hip's
// kernels over the view's buffers (TfTarget) and the view's state block.
//
// A view has a reading (tf_set_view_reading, kept in its TfTarget): resident, the blocks in the VBA; or whole, both
// tiers of a swapping context -- the scan then takes the entries that resolve in either tier (ViewScanT<true>, the
// rule is tf_tier.h's), and tf_render.hip's kernels over both tiers are launched for the target (the
// whole reading).  On a context without a GlobalCache the whole reading runs the resident kernels.
//
// No view call writes anything of the context's: not a TF_BUF_* buffer, not its device state, not its host
// parameters (the call's intrinsics go into the view's TfTarget, not through an IntrScope), not the raycast pair's
// tile costs.  Every call flushes a pending per-call frame first and runs on the context stream, after the caller's
// work on the default stream.
#include "tf_host.h"
#include "tf_compact.h"
#include "tf_env.h"
#include "tf_pose.h"
#include "tf_tier.h"
#include "tf_vis.h"

#include <limits.h>
#include <stdlib.h>
#include <new>

typedef unsigned vw_u4 __attribute__((ext_vector_type(4)));

struct tf_view {
    tf_ctx* c;
    TfTarget t;                      // the view's render state; every buffer in it is the context registry's
    int4* grp;                       // the compaction's scratch: [2 * groups + 2] (tf_compact.h)
    unsigned long long* masks;       // per 64 entries the visible lanes (count pass -> emit pass): [4 * groups]
    float4* maps[2];                 // renderICP's points / normals, three levels each; from the first tf_view_icp_maps
    // the reading (tf_set_view_reading) lives in t.whole: every stage takes it from the call's TfTarget
};

// ---- the scan ------------------------------------------------------------------------------------------
// WHOLE: live = the entry resolves in either tier (tf_tier.h) -- one flag byte per entry more, fetched only where
// ptr == -1; the ballots, the prefix and the emit pass are the same
template <bool WHOLE>
struct ViewScanT {
    struct Item {};
    const TfHashEntry* hash;
    const unsigned char* flags;      // hasStoredData per entry (WHOLE)
    const TfDevState* st;            // the view's: M_alloc is the world -> camera matrix
    VisArgs v;
    unsigned long long* masks;

    __device__ __forceinline__ unsigned classify(int i, bool in, Item&) const
    {
        TfHashEntry e;
        e.ptr = -2;
        if (in) {
            const vw_u4 w = *reinterpret_cast<const vw_u4*>(hash + i);
            e.x = (short)(w.x & 0xffffu); e.y = (short)(w.x >> 16); e.z = (short)(w.y & 0xffffu); e.pad = 0;
            e.offset = (int)w.z; e.ptr = (int)w.w;
        }
        const bool live = WHOLE ? tier_ptr_resolves(flags, i, e.ptr) : e.ptr >= 0;     // (past n: ptr -2)
        bool vis = false;
        if (__ballot(live) != 0ull) {          // (wave-uniform: an empty wave does no projection)
            if (live) vis = vis_block(e, st->M_alloc, v);
        }
        const unsigned long long m = __ballot(vis);
        if ((i & 63) == 0) masks[i >> 6] = m;  // a wave is 64 consecutive entries (CK_WG = 4 waves)
        return vis ? 1u : 0u;
    }
    __device__ __forceinline__ void emit(int, const Item&, unsigned, int, int, int) const {}
};
struct ViewScanPass : ViewScanT<false> {};
struct ViewScanWholePass : ViewScanT<true> {};

struct ViewEmitPass {
    struct Item {};
    const unsigned long long* masks;
    int capacity;
    int* visibleIds;

    __device__ __forceinline__ unsigned classify(int i, bool in, Item&) const
    {
        return in ? (unsigned)((masks[i >> 6] >> (i & 63)) & 1ull) : 0u;
    }
    __device__ __forceinline__ void emit(int i, const Item&, unsigned bits, int at, int, int) const
    {
        if ((bits & 1u) && at < capacity) visibleIds[at] = i;
    }
};

// the call's pose into the view's state block.  ALLOC_MODE 2: world -> camera as given (M_alloc); 0: camera ->
// world (M_ray) alone; 1: camera -> world, and world -> camera = its tf_rigid_inv, as the frame path inverts
// poses_.back() (topfu.cpp:281, 306).  mode / abort stay 1 / 0: a view always takes the tracking-path kernels.
// (One kernel per mode: with the mode as a run-time argument the single-thread code came out of the compiler
// with a wrong M_alloc for mode 2 -- elements of the rotation and the x, y translation undefined.)
template <int ALLOC_MODE>
__global__ void k_view_pose(TfDevState* st)
{
    float pose[12];
    for (int i = 0; i < 12; ++i) pose[i] = st->pose_in[i];
    tf_set_pose_matrices(st, pose, ALLOC_MODE);
    st->mode = 1;
    st->abort = 0;
}

__global__ void k_view_set_n(TfDevState* st, const int4* totals) { st->noVisibleEntries = totals->x; }

// ---- host ----------------------------------------------------------------------------------------------
static size_t view_npx(const tf_view* v) { return (size_t)v->t.W * v->t.H; }

static void view_release(tf_view* v)
{
    TfCtxMem& m = v->c->mem;
    TfTarget& t = v->t;
    (void)m.release(t.visibleIds); (void)m.release(t.range); (void)m.release(t.raycast); (void)m.release(t.image);
    (void)m.release(t.blockRec); (void)m.release(t.blockTiles); (void)m.release(t.blockOff); (void)m.release(t.edChunk);
    (void)m.release(t.edBins); (void)m.release(t.edBinCnt); (void)m.release(t.edSpill); (void)m.release(t.st);
    (void)m.release(v->grp); (void)m.release(v->masks); (void)m.release(v->maps[0]); (void)m.release(v->maps[1]);
}

extern "C" tf_status tf_view_create(tf_ctx* c, const tf_view_params* vp, tf_view** out)
{
    TF_FLUSH(c);
    if (!c || !vp || !out) return TF_INVALID_ARG;
    *out = nullptr;
    // the size as tf_create takes it (params_valid, tf_capi.hip)
    if (vp->cols <= 0 || vp->rows <= 0 || (vp->cols % 4) || (vp->rows % 4) || vp->cols > 65535 || vp->rows > 65535) return TF_INVALID_ARG;
    if ((double)vp->cols * vp->rows * 64.0 > 2147483000.0) return TF_INVALID_ARG;
    if (vp->vis_capacity < 0 || vp->max_render_blocks < 0) return TF_INVALID_ARG;
    tf_view* v = new (std::nothrow) tf_view();
    if (!v) return TF_OOM;
    v->c = c;
    TfTarget& t = v->t;
    t.W = vp->cols; t.H = vp->rows;
    t.fx = c->p.fx; t.fy = c->p.fy; t.cx = c->p.cx; t.cy = c->p.cy;
    t.vis_capacity = vp->vis_capacity ? vp->vis_capacity : c->n_total;
    t.max_render_blocks = vp->max_render_blocks ? vp->max_render_blocks : c->p.max_render_blocks;
    // k_ed_fill's LDS-row path, limited as tf_create limits the context's
    t.ed_lds_max_n = tf_env_int("TFUSION_ED_LDS_MAX_N", ED_LDS_MAX_N, 0, INT_MAX, 0);
    if (t.ed_lds_max_n > ED_LDS_MAX_N) t.ed_lds_max_n = ED_LDS_MAX_N;
    if (t.ed_lds_max_n > t.vis_capacity) t.ed_lds_max_n = t.vis_capacity;
    if (t.W > ED_MAX_W || t.H > ED_MAX_W) t.ed_lds_max_n = 0;
    const size_t npx = view_npx(v), cap = (size_t)t.vis_capacity, nrows = (size_t)ed_nrows(t.H);
    const size_t ng = (size_t)ck_groups(c->n_total);
    hipError_t e = tf_mem_hip(c->mem.alloc_group({
        TfCtxMem::dev(&t.visibleIds, sizeof(int) * cap), TfCtxMem::dev(&t.range, sizeof(float) * 2 * npx),
        TfCtxMem::dev(&t.raycast, sizeof(float) * 4 * npx), TfCtxMem::dev(&t.image, sizeof(uchar4) * npx),
        TfCtxMem::dev(&t.blockRec, sizeof(uint4) * cap), TfCtxMem::dev(&t.blockTiles, sizeof(int) * cap),
        TfCtxMem::dev(&t.blockOff, sizeof(int) * cap), TfCtxMem::dev(&t.edChunk, sizeof(int) * (cap / 256 + 1)),    // per ED_CHUNK entries
        TfCtxMem::dev(&t.edBinCnt, sizeof(int) * 2 * nrows), TfCtxMem::dev(&t.edSpill, sizeof(int2) * nrows),
        TfCtxMem::dev(&t.st, sizeof(TfDevState)), TfCtxMem::dev(&v->grp, sizeof(int4) * (2 * ng + 2)),
        TfCtxMem::dev(&v->masks, sizeof(unsigned long long) * 4 * ng) }));
    if (e == hipSuccess && t.ed_lds_max_n > 0) e = tf_mem_hip(c->mem.alloc(&t.edBins, sizeof(uint4) * 2 * nrows * (size_t)t.ed_lds_max_n));
    // the state block: identity pose, tracking path, nothing visible; the buffers as tf_create leaves the context's
    TfDevState* s0 = e == hipSuccess ? (TfDevState*)calloc(1, sizeof(TfDevState)) : nullptr;
    float2* r0 = e == hipSuccess ? (float2*)malloc(sizeof(float2) * npx) : nullptr;
    if (e == hipSuccess && (!s0 || !r0)) e = hipErrorOutOfMemory;
    if (e == hipSuccess) {
        for (int i = 0; i < 12; ++i) s0->pose[i] = (i % 5 == 0) ? 1.0f : 0.0f;
        s0->icp_ok = 1;
        s0->mode = 1;
        // RenderState ctor: renderingRangeImage = (viewFrustum_min, viewFrustum_max) (RenderState.hpp:56-76)
        for (size_t i = 0; i < npx; ++i) r0[i] = make_float2(c->p.viewFrustum_min, c->p.viewFrustum_max);
        e = hipMemcpyAsync(t.st, s0, sizeof(TfDevState), hipMemcpyHostToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(t.range, r0, sizeof(float2) * npx, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t.visibleIds, 0, sizeof(int) * cap, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t.raycast, 0, sizeof(float) * 4 * npx, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t.image, 0, sizeof(uchar4) * npx, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t.edBinCnt, 0, sizeof(int) * 2 * nrows, c->stream);
    if (e == hipSuccess) e = ed_spill_all(c, t);         // the first CreateExpectedDepths clears the whole buffer (waits)
    else (void)hipStreamSynchronize(c->stream);
    free(s0);
    free(r0);
    if (e == hipSuccess && c->views.add(v, [](void* p) { delete (tf_view*)p; }, 1) != 0) e = hipErrorOutOfMemory;
    if (e != hipSuccess) {
        view_release(v);
        delete v;
        return tf_from_hip(e);
    }
    *out = v;
    return TF_OK;
}

extern "C" void tf_view_destroy(tf_view* v)
{
    if (!v) return;
    tf_ctx* c = v->c;
    (void)flush_tail(c);
    (void)hipStreamSynchronize(c->stream);
    if (!c->views.remove(v)) return;
    view_release(v);
    delete v;
}

// what every view call does first: the pending per-call frame, the caller's work, the call's pose and intrinsics
static tf_status view_begin(tf_view* v, const float* intr, const float* rt, int alloc_mode, TfTarget* t)
{
    tf_ctx* c = v->c;
    TF_CHECK(order_after_caller(c));
    *t = v->t;
    if (intr) { t->fx = intr[0]; t->fy = intr[1]; t->cx = intr[2]; t->cy = intr[3]; }
    TF_CHECK(hipMemcpyAsync(t->st->pose_in, rt, sizeof(float) * 12, hipMemcpyHostToDevice, c->stream));
    if (alloc_mode == 2) hipLaunchKernelGGL(k_view_pose<2>, dim3(1), dim3(1), 0, c->stream, t->st);
    else if (alloc_mode == 1) hipLaunchKernelGGL(k_view_pose<1>, dim3(1), dim3(1), 0, c->stream, t->st);
    else hipLaunchKernelGGL(k_view_pose<0>, dim3(1), dim3(1), 0, c->stream, t->st);
    TF_CHECK(hipGetLastError());
    return TF_OK;
}

// FindVisibleBlocks over the view's matrices: count, the capacity check on the host, emit.  TF_CAPACITY leaves
// the list and the view's count as they were.
template <class Scan>
static tf_status view_scan_as(tf_view* v, const TfTarget& t, int* n_visible)
{
    tf_ctx* c = v->c;
    Scan scan;
    scan.hash = c->hash; scan.flags = c->swapFlags; scan.st = t.st; scan.masks = v->masks;
    scan.v.fx = t.fx; scan.v.fy = t.fy; scan.v.cx = t.cx; scan.v.cy = t.cy;
    scan.v.factor = (float)TF_BLK * c->p.voxelSize;
    scan.v.W = t.W; scan.v.H = t.H;
    scan.v.n_total = c->n_total; scan.v.cap = t.vis_capacity;
    scan.v.enlarged = 0;                  // the reference kernel takes isVisible, also on a swapping scene
    TF_CHECK(tfk_ck_count(c, scan, c->n_total, v->grp));
    const int4* totals = v->grp + 2 * ck_groups(c->n_total);
    int4 tot = make_int4(0, 0, 0, 0);
    TF_CHECK(hipMemcpyAsync(&tot, totals, sizeof(int4), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    if (n_visible) *n_visible = tot.x;
    if (tot.x > t.vis_capacity) return TF_CAPACITY;
    const ViewEmitPass emit = { v->masks, t.vis_capacity, t.visibleIds };
    TF_CHECK(tfk_ck_emit(c, emit, c->n_total, v->grp));
    hipLaunchKernelGGL(k_view_set_n, dim3(1), dim3(1), 0, c->stream, t.st, totals);
    TF_CHECK(hipGetLastError());
    return TF_OK;
}

// the whole reading on a context without a GlobalCache is the resident one
static tf_status view_scan(tf_view* v, const TfTarget& t, int* n_visible)
{
    return (t.whole && v->c->p.use_swapping) ? view_scan_as<ViewScanWholePass>(v, t, n_visible) : view_scan_as<ViewScanPass>(v, t, n_visible);
}

static bool type_ok(int type) { return type >= TF_RENDER_SHADED_GREYSCALE && type <= TF_RENDER_COLOUR_FROM_CONFIDENCE; }

static hipError_t view_image_out(tf_view* v, uint8_t* dev_rgba, size_t step)
{
    if (!dev_rgba) return hipSuccess;
    const size_t row = (size_t)v->t.W * 4;
    return hipMemcpy2DAsync(dev_rgba, step ? step : row, v->t.image, row, row, v->t.H, hipMemcpyDeviceToDevice, v->c->stream);
}

extern "C" tf_status tf_view_find_visible(tf_view* v, const float intr[4], const float pose_rt[12], int* n_visible)
{
    if (!v || !pose_rt) return TF_INVALID_ARG;
    TF_FLUSH(v->c);
    TfTarget t;
    tf_status s = view_begin(v, intr, pose_rt, 2, &t);
    if (s == TF_OK) s = view_scan(v, t, n_visible);
    return s == TF_OK ? sync_checked(v->c) : s;
}

extern "C" tf_status tf_view_expected_depths(tf_view* v, const float intr[4], const float pose_rt[12])
{
    if (!v || !pose_rt) return TF_INVALID_ARG;
    TF_FLUSH(v->c);
    TfTarget t;
    const tf_status s = view_begin(v, intr, pose_rt, 2, &t);
    if (s != TF_OK) return s;
    TF_CHECK(tfk_expected_depths(v->c, t, 0, 0));
    return sync_checked(v->c);
}

extern "C" tf_status tf_view_raycast(tf_view* v, const float intr[4], const float invM_rt[12])
{
    if (!v || !invM_rt) return TF_INVALID_ARG;
    TF_FLUSH(v->c);
    TfTarget t;
    const tf_status s = view_begin(v, intr, invM_rt, 0, &t);
    if (s != TF_OK) return s;
    TF_CHECK(tfk_raycast(v->c, t, nullptr));             // castRay<false>: no visibility marks
    return sync_checked(v->c);
}

extern "C" tf_status tf_view_shade(tf_view* v, const float intr[4], const float invM_rt[12], int type, uint8_t* dev_rgba,
                                   size_t step)
{
    if (!v || !invM_rt || !type_ok(type)) return TF_INVALID_ARG;
    TF_FLUSH(v->c);
    TfTarget t;
    const tf_status s = view_begin(v, intr, invM_rt, 0, &t);
    if (s != TF_OK) return s;
    TF_CHECK(tfk_render_type(v->c, t, type));
    TF_CHECK(view_image_out(v, dev_rgba, step));
    return sync_checked(v->c);
}

extern "C" tf_status tf_view_icp_maps(tf_view* v, const float intr[4], const float invM_rt[12], void* points, size_t pstep,
                                      void* normals, size_t nstep)
{
    if (!v || !invM_rt) return TF_INVALID_ARG;
    tf_ctx* c = v->c;
    TF_FLUSH(c);
    const size_t npx = view_npx(v), nlev = npx + npx / 4 + npx / 16;      // cols, rows are multiples of 4
    if (!v->maps[0])
        TF_CHECK(tf_mem_hip(c->mem.alloc_group({ TfCtxMem::dev(&v->maps[0], sizeof(float4) * nlev),
                                                 TfCtxMem::dev(&v->maps[1], sizeof(float4) * nlev) })));
    TfTarget t;
    const tf_status s = view_begin(v, intr, invM_rt, 0, &t);
    if (s != TF_OK) return s;
    float4 *pts[TF_LEVELS], *nrm[TF_LEVELS];
    pts[0] = v->maps[0]; nrm[0] = v->maps[1];
    for (int l = 1; l < TF_LEVELS; ++l) {
        const size_t off = (size_t)(t.W >> (l - 1)) * (size_t)(t.H >> (l - 1));
        pts[l] = pts[l - 1] + off; nrm[l] = nrm[l - 1] + off;
    }
    TF_CHECK(tfk_icp_maps(c, t, pts, nrm));               // renderICP on the view's raycast result
    const size_t row = sizeof(float4) * (size_t)t.W;
    if (points) TF_CHECK(hipMemcpy2DAsync(points, pstep ? pstep : row, pts[0], row, row, t.H, hipMemcpyDeviceToDevice, c->stream));
    if (normals) TF_CHECK(hipMemcpy2DAsync(normals, nstep ? nstep : row, nrm[0], row, row, t.H, hipMemcpyDeviceToDevice, c->stream));
    return sync_checked(c);
}

extern "C" tf_status tf_view_render(tf_view* v, const float intr[4], const float c2w_rt[12], int type, uint8_t* dev_rgba,
                                    size_t step)
{
    if (!v || !c2w_rt || !type_ok(type)) return TF_INVALID_ARG;
    tf_ctx* c = v->c;
    TF_FLUSH(c);
    TfTarget t;
    tf_status s = view_begin(v, intr, c2w_rt, 1, &t);
    if (s == TF_OK) s = view_scan(v, t, nullptr);
    if (s != TF_OK) return s;
    TF_CHECK(tfk_expected_depths(c, t, 0, 0));
    TF_CHECK(tfk_raycast(c, t, nullptr));
    TF_CHECK(tfk_render_type(c, t, type));
    TF_CHECK(view_image_out(v, dev_rgba, step));
    return sync_checked(c);
}

extern "C" tf_status tf_view_download(tf_view* v, int which, void* host, size_t bytes)
{
    if (!v || !host) return TF_INVALID_ARG;
    TF_FLUSH(v->c);
    const size_t npx = view_npx(v);
    const void* p = nullptr;
    size_t n = 0;
    switch (which) {
    case TF_VIEW_VISIBLE_IDS: p = v->t.visibleIds; n = sizeof(int) * (size_t)v->t.vis_capacity; break;
    case TF_VIEW_RANGE: p = v->t.range; n = sizeof(float) * 2 * npx; break;
    case TF_VIEW_RAYCAST: p = v->t.raycast; n = sizeof(float) * 4 * npx; break;
    case TF_VIEW_IMAGE: p = v->t.image; n = sizeof(uchar4) * npx; break;
    }
    if (!p || n != bytes) return TF_INVALID_ARG;
    TF_CHECK(hipMemcpyAsync(host, p, n, hipMemcpyDeviceToHost, v->c->stream));
    return sync_checked(v->c);
}

extern "C" tf_status tf_view_stats(tf_view* v, int* n_visible, int* n_render_blocks)
{
    if (!v) return TF_INVALID_ARG;
    TF_FLUSH(v->c);
    int two[2] = { 0, 0 };                                 // noVisibleEntries, noTotalBlocks: adjacent in TfDevState
    static_assert(offsetof(TfDevState, noTotalBlocks) == offsetof(TfDevState, noVisibleEntries) + sizeof(int), "adjacent");
    TF_CHECK(hipMemcpyAsync(two, (const char*)v->t.st + offsetof(TfDevState, noVisibleEntries), sizeof(two), hipMemcpyDeviceToHost,
                            v->c->stream));
    const tf_status s = sync_checked(v->c);
    if (s != TF_OK) return s;
    if (n_visible) *n_visible = two[0];
    if (n_render_blocks) *n_render_blocks = two[1];
    return TF_OK;
}

extern "C" tf_status tf_set_view_reading(tf_view* v, int reading)
{
    if (!v || (reading != TF_VIEW_RESIDENT && reading != TF_VIEW_WHOLE)) return TF_INVALID_ARG;
    v->t.whole = reading == TF_VIEW_WHOLE;
    return TF_OK;
}

extern "C" tf_status tf_get_view_reading(tf_view* v, int* reading)
{
    if (!v || !reading) return TF_INVALID_ARG;
    *reading = v->t.whole ? TF_VIEW_WHOLE : TF_VIEW_RESIDENT;
    return TF_OK;
}

extern "C" tf_status tf_view_get_params(tf_view* v, tf_view_params* p)
{
    if (!v || !p) return TF_INVALID_ARG;
    p->cols = v->t.W; p->rows = v->t.H; p->vis_capacity = v->t.vis_capacity; p->max_render_blocks = v->t.max_render_blocks;
    return TF_OK;
}
