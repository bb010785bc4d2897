// tf_capi.hip -- the context of libtfusion_hip's C-ABI: status strings, device queries, parameters, the
// persistent-ICP ordering among contexts, tf_create / tf_destroy / tf_reset, the getters and setters, and
// the state transfer (tf_download*, tf_upload, tf_set_pose, tf_set_counters, the totals).  The frames are
// tf_frame.hip's, the stage and engine entry points tf_engines.hip's; the mesh and checkpoint entry points
// stand below their launchers in tf_mesh.hip and tf_scene_ckpt.hip.
#include "tf_host.h"
#include "tf_env.h"

#include <vector>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <new>

extern "C" const char* tf_status_string(tf_status s)
{
    switch (s) {
    case TF_OK: return "ok";
    case TF_ICP_FAIL: return "icp failed (scene reset)";
    case TF_INVALID_ARG: return "invalid argument";
    case TF_OOM: return "out of device memory";
    case TF_HIP_ERROR: return "HIP error";
    case TF_NO_DEVICE: return "no HIP device";
    case TF_INDEX_RANGE: return "more mesh vertices than a 32-bit index can number";
    case TF_CAPACITY: return "the content does not fit: a map's live content the context's tables, a view's visible entries its list";
    }
    return "unknown";
}

extern "C" tf_status tf_device_count(int* count)
{
    if (!count) return TF_INVALID_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e == hipErrorNoDevice) { *count = 0; return TF_OK; }
    if (e != hipSuccess) { *count = 0; return tf_from_hip(e); }
    *count = n;
    return TF_OK;
}

extern "C" tf_status tf_set_device(int device) { return tf_from_hip(hipSetDevice(device)); }

extern "C" tf_status tf_default_params(tf_params* p)
{   // TopFuParams::default_params (topfu.cpp:12-53) + SceneParams(0.02, 100, 0.005, 0.2, 3.0) (:50)
    if (!p) return TF_INVALID_ARG;
    memset(p, 0, sizeof(*p));
    p->cols = 640; p->rows = 480;
    p->fx = 504.261f; p->fy = 503.905f; p->cx = 352.457f; p->cy = 272.202f;
    p->bilateral_sigma_depth = 0.04f;
    p->bilateral_sigma_spatial = 4.5f;
    p->bilateral_kernel_size = 7;
    p->icp_truncate_depth_dist = 2.0f;
    p->icp_dist_thres = 0.1f;
    p->icp_angle_thres = 30.f * 0.017453293f;
    p->icp_iter_num[0] = 10; p->icp_iter_num[1] = 5; p->icp_iter_num[2] = 4; p->icp_iter_num[3] = 0;
    p->mu = 0.02f; p->maxW = 100; p->voxelSize = 0.005f;
    p->viewFrustum_min = 0.2f; p->viewFrustum_max = 3.0f;
    p->n_buckets = 0x100000; p->n_excess = 0x20000; p->n_blocks = 0x10000;
    p->vis_capacity = 0x40000;
    p->max_render_blocks = 65536 * 4;
    p->use_swapping = 0;                          // Scene(params, false), topfu.cpp:67
    p->swap_transfer_blocks = 0x1000;             // SDF_TRANSFER_BLOCK_NUM, VoxelBlockHash.hpp:27
    p->voxel_rgb = 0;                             // Voxel_s (Defines.hpp:5)
    p->depth_to_rgb[0] = p->depth_to_rgb[5] = p->depth_to_rgb[10] = 1.0f;   // registered RGB-D
    return TF_OK;
}

static bool params_valid(const tf_params* p)
{
    if (p->cols <= 0 || p->rows <= 0 || (p->cols % 4) || (p->rows % 4)) return false;
    if (p->n_buckets <= 0 || (p->n_buckets & (p->n_buckets - 1))) return false;
    if (p->n_excess <= 0 || p->n_blocks <= 0 || p->vis_capacity <= 0 || p->max_render_blocks <= 0) return false;
    // The render side forms 32-bit byte offsets (voff + guard shift + lin) * 4 from the guard
    // block before the VBA (tf_render.hip vox_at): block ptr p reads up to 4 * ((p + 2) * 512 - 1)
    // bytes past the guard, which fits 2^32 only for p <= 2^21 - 2, i.e. n_blocks <= 2^21 - 1.
    if (p->n_blocks > (1 << 21) - 1) return false;
    if ((p->n_buckets + p->n_excess) % 16) return false;
    if (p->bilateral_kernel_size < 1 || p->bilateral_kernel_size > 7) return false;
    // the tracker's iteration counts, as tf_icp_set_params takes them: none negative, three pyramid levels (TF_LEVELS)
    for (int l = 0; l < 4; ++l) if (p->icp_iter_num[l] < 0) return false;
    if (p->icp_iter_num[3] != 0) return false;
    if (p->voxelSize <= 0 || p->mu <= 0) return false;
    // steps per pixel ceil(2*|e-s|) with |e-s| ~ 2*mu/(8*voxel) must fit the 6-bit key field
    if (4.0f * p->mu / (8.0f * p->voxelSize) + 2.0f > 60.0f) return false;
    if ((double)p->cols * p->rows * 64.0 > 2147483000.0) return false;
    if (p->cols > 65535 || p->rows > 65535) return false;               // k_ed_fill's 16-bit box records
    if (p->use_swapping && (p->swap_transfer_blocks <= 0 || p->swap_transfer_blocks > p->n_buckets + p->n_excess)) return false;
    // the mesher's whole reading addresses a stored voxel as entry * 512 + lin in an int (tf_tier.h, TierBlk):
    // the table must stay below 2^22 entries (the reference's has 1.18 M; 2^22 would be 8 GiB of GlobalCache)
    if (p->use_swapping && (long long)p->n_buckets + p->n_excess > (1 << 22) - 1) return false;
    // the GlobalCache holds Voxel_s blocks: a swapping colour scene would need the colour half
    // swapped too (CombineVoxelInformation's colour part) -- not built
    if (p->voxel_rgb && p->use_swapping) return false;
    return true;
}

// ---------------------------------------------------------------------------------------
// persistent-ICP ordering among the contexts of one device (see tf_internal.h)
// ---------------------------------------------------------------------------------------
#include <mutex>
#define TF_MAX_DEVICES 64
static std::mutex g_icp_mu;
static int g_icp_ctx_count[TF_MAX_DEVICES];          // live contexts per device
static tf_ctx* g_icp_last[TF_MAX_DEVICES];          // context of the last persistent ICP launch

static void icp_order_register(tf_ctx* c, int add)
{
    if (c->device < 0 || c->device >= TF_MAX_DEVICES) return;
    std::lock_guard<std::mutex> lk(g_icp_mu);
    g_icp_ctx_count[c->device] += add;
    if (add < 0 && g_icp_last[c->device] == c) g_icp_last[c->device] = nullptr;
    // a single context records nothing (an event record per frame costs the device ~4 us): when
    // a second one arrives, the last launcher's stream is marked here, so the newcomer's first
    // ICP waits for everything already enqueued there
    tf_ctx* last = g_icp_last[c->device];
    if (add > 0 && last && last != c) (void)hipEventRecord(last->icp_ev, last->stream);
}

// called with the launch enqueued between before() and after(), from one host thread per context
hipError_t tf_icp_order_before(tf_ctx* c)
{
    if (c->device < 0 || c->device >= TF_MAX_DEVICES || !c->icp_ev) return hipSuccess;
    g_icp_mu.lock();                                  // released by tf_icp_order_after
    tf_ctx* last = g_icp_last[c->device];
    if (g_icp_ctx_count[c->device] > 1 && last && last != c) return hipStreamWaitEvent(c->stream, last->icp_ev, 0);
    return hipSuccess;
}

hipError_t tf_icp_order_after(tf_ctx* c)
{
    if (c->device < 0 || c->device >= TF_MAX_DEVICES || !c->icp_ev) return hipSuccess;
    const hipError_t e = g_icp_ctx_count[c->device] > 1 ? hipEventRecord(c->icp_ev, c->stream) : hipSuccess;
    g_icp_last[c->device] = c;
    g_icp_mu.unlock();
    return e;
}

static void ctx_free(tf_ctx* c)
{
    if (!c) return;
    if (c->icp_ev) {
        icp_order_register(c, -1);
        (void)hipEventDestroy(c->icp_ev);
    }
    if (c->caller_ev) (void)hipEventDestroy(c->caller_ev);
    for (hipEvent_t ev : c->ckptEv) if (ev) (void)hipEventDestroy(ev);
    for (int i = 0; i < 2 * TF_NUM_STAGES * TF_PROF_RING; ++i) if (c->prof_ev[i]) (void)hipEventDestroy(c->prof_ev[i]);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                         // c->mem frees every buffer the context still holds
}

// HIP's allocators, as every context's registry (tf_ctx::mem) and its scoped temporaries get them: the one
// place of the library that names them
static const TfMemFns tf_hip_mem_fns = {
    [](void** p, size_t bytes) { return (int)hipMalloc(p, bytes); },
    [](void* p) { return (int)hipFree(p); },
    [](void** p, size_t bytes, unsigned flags) { return (int)hipHostMalloc(p, bytes, flags); },
    [](void* p) { return (int)hipHostFree(p); },
    (int)hipErrorOutOfMemory
};

tf_status sync_state(tf_ctx* c)
{
    TF_CHECK(hipMemcpyAsync(c->st_host, c->st, sizeof(TfDevState), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    // a frame that failed past its ICP (tf_reset.h: frame_ok -3) left the context in error until
    // tf_reset -- also when the call that enqueued it had already returned (per-call frames)
    if (c->st_host->sticky_error) return TF_HIP_ERROR;
    return TF_OK;
}

// the end of every synchronous entry point: wait for the stream, then report a context left in
// error by a device-side failure past an ICP (tf_reset.h: frame_ok -3) or by an engine-level
// launch's failed wait (k_vis_build) -- TF_HIP_ERROR from every call until tf_reset
tf_status sync_checked(tf_ctx* c)
{
    TF_CHECK(hipMemcpyAsync(&c->st_host->sticky_error, &c->st->sticky_error, sizeof(int), hipMemcpyDeviceToHost,
                            c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    return c->st_host->sticky_error ? TF_HIP_ERROR : TF_OK;
}

// TopFu::reset (topfu.cpp:141-152): pose history -> [I], ResetScene.  The render state
// (visible list / types / range image) is deliberately left as is, like the reference.
__global__ void k_host_reset(TfDevState* st)
{
    st->halt = 0;                      // (a device-side failure is cleared by the reset)
    st->sticky_error = 0;
    if (st->frame_counter) st->n_resets++;
    st->frame_counter = 0;
    for (int i = 0; i < 12; ++i) st->pose[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

static tf_status ctx_reset(tf_ctx* c)
{
    hipLaunchKernelGGL(k_host_reset, dim3(1), dim3(1), 0, c->stream, c->st);
    TF_CHECK(hipGetLastError());
    TF_CHECK(tfk_reset_scene(c));
    const tf_status s = sync_state(c);
    if (s != TF_OK) return s;
    c->frame_counter = c->st_host->frame_counter;
    c->n_resets = c->st_host->n_resets;
    return TF_OK;
}

// The environment switches, read once per context (tf_env.h: how a flag and an integer are read).  A/B: kept
// for measurements, the default is the product.
//
//   switch                      default     meaning                                                       test
//   TFUSION_VIS_FUSED           on          0: the visible list in two launches (k_vis_count +             (A/B)
//                                           k_vis_apply) instead of one k_vis_build
//   TFUSION_ED_LDS_MAX_N        16384       k_ed_fill reduces a /8 row in LDS up to this many visible      test_gpu_parity, test_gpu_failures
//                                           entries, device-scope atomics past it; clamped to
//                                           [0, ED_LDS_MAX_N] and to vis_capacity, 0 on images wider
//                                           or taller than ED_MAX_W (tf_create)
//   TFUSION_TILE_ORDER          on          0: the raycast pair's tiles in the plain XCD-swizzled order    test_gpu_tile_order
//                                           instead of longest first
//   TFUSION_TILE_MAP            (bands)     rows: XCD x takes the tile rows = x (mod 8) instead of the     test_gpu_tile_order
//                                           x-th band of consecutive tiles
//   TFUSION_ICP_FAULT           (none)      launch:iteration -- that persistent ICP launch of the          test_gpu_failures
//                                           context reports a lost peer at that iteration, so the
//                                           run-time fallback to the per-iteration schedule runs
//   TFUSION_FILL_FAULT          0 (never)   launch -- that k_raycast_pair launch's wait for the range      test_gpu_failures
//                                           image fails (past the ICP: the sticky-error path)
//   TFUSION_VIS_FAULT           0 (never)   launch -- that k_vis_build launch's wait for the lower         test_gpu_failures
//                                           chunks' counts fails
//   TFUSION_FUSE_TAIL           on          0: engine batches in the 7-launch form                         test_gpu_hash_stress
//   TFUSION_CKPT_CHUNK_BLOCKS   4096        blocks per staging chunk of tf_scene_save / tf_scene_load;     test_gpu_scene_ckpt
//                                           outside [1, 2^18]: the default
//   TFUSION_MESH_CHUNK_BYTES    8388608     bytes of the pinned chunk through which                        test_gpu_mesh_indexed_whole
//                                           tf_mesh_save_ply_indexed_whole brings the columns to the
//                                           host; outside [24, 2^30]: the default
//   TFUSION_CKPT_TIMING         off         1: HIP events (and a wait) around the checkpoint kernels,      (tools)
//                                           for tf_scene_ckpt_times
//   TFUSION_PERCALL_EARLY       on          0: per-call frames wait for the whole frame                    test_gpu_percall, test_gpu_failures
//   TFUSION_PERCALL_DEFER       on          0: per-call frames enqueue all their launches                  test_gpu_percall
//   TFUSION_INTEG_WG_FRAME      768         integration workgroups of the frame path; outside              (A/B)
//                                           [64, TF_INTEG_WG]: TF_INTEG_WG
//   TFUSION_ICP_SOLVE           (opencv4)   the ICP iterations' pose algebra (tf_set_pose_algebra): by     test_gpu_pose_algebra
//                                           default the reference's own, cv::determinant / cv::solve
//                                           (DECOMP_SVD) / Affine3f as OpenCV 3.x-4.x write them;
//                                           opencv2 (OpenCV 2.4.9) or canonical (the short block-Schur tail)
//   TFUSION_ICP_PERSISTENT      on          0: one k_icp_iter launch per iteration even where the          test_gpu_parity, test_gpu_pose_algebra
//                                           persistent launch would fit (tf_create checks that it does)
static void tf_read_env(tf_ctx* c)
{
    c->vis_fused = tf_env_flag("TFUSION_VIS_FUSED", 1);
    c->ed_lds_max_n = tf_env_int("TFUSION_ED_LDS_MAX_N", ED_LDS_MAX_N, 0, INT_MAX, 0);
    if (c->ed_lds_max_n > ED_LDS_MAX_N) c->ed_lds_max_n = ED_LDS_MAX_N;
    c->tile_ljf = tf_env_flag("TFUSION_TILE_ORDER", 1);
    const char* env = getenv("TFUSION_TILE_MAP");
    c->tile_rows = env && strcmp(env, "rows") == 0;
    env = getenv("TFUSION_ICP_FAULT");
    long long fl = 0; int fi = -1;
    if (env && sscanf(env, "%lld:%d", &fl, &fi) == 2 && fl > 0 && fi >= 0) { c->icp_fault_launch = fl; c->icp_fault_iter = fi; }
    else { c->icp_fault_launch = 0; c->icp_fault_iter = -1; }
    c->fill_fault_launch = tf_env_count("TFUSION_FILL_FAULT");
    c->vis_fault_launch = tf_env_count("TFUSION_VIS_FAULT");
    c->fuse_tail = tf_env_flag("TFUSION_FUSE_TAIL", 1);
    c->ckpt_chunk_blocks = tf_env_int("TFUSION_CKPT_CHUNK_BLOCKS", TF_CKPT_CHUNK_BLOCKS, 1, 1 << 18, TF_CKPT_CHUNK_BLOCKS);
    c->mesh_chunk_bytes = tf_env_int("TFUSION_MESH_CHUNK_BYTES", TF_MESH_CHUNK_BYTES, 24, 1 << 30, TF_MESH_CHUNK_BYTES);
    c->ckpt_timing = tf_env_flag("TFUSION_CKPT_TIMING", 0);
    c->percall_early = tf_env_flag("TFUSION_PERCALL_EARLY", 1);
    c->percall_defer = tf_env_flag("TFUSION_PERCALL_DEFER", 1);
    c->integ_wg_frame = tf_env_int("TFUSION_INTEG_WG_FRAME", TF_INTEG_WG_FRAME, 64, TF_INTEG_WG, TF_INTEG_WG);
    env = getenv("TFUSION_ICP_SOLVE");
    c->pose_alg = !env ? TF_POSE_ALGEBRA_OPENCV4
                : !strcmp(env, "canonical") ? TF_POSE_ALGEBRA_CANONICAL
                : !strcmp(env, "opencv2") ? TF_POSE_ALGEBRA_OPENCV2 : TF_POSE_ALGEBRA_OPENCV4;
    c->icp_persistent = tf_env_flag("TFUSION_ICP_PERSISTENT", 1);
}

extern "C" tf_status tf_create(const tf_params* pin, tf_ctx** out)
{
    if (!pin || !out) return TF_INVALID_ARG;
    *out = nullptr;
    if (!params_valid(pin)) return TF_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return TF_NO_DEVICE;
    tf_ctx* c = new (std::nothrow) tf_ctx{ TfCtxMem(tf_hip_mem_fns) };     // every other member zero
    if (!c) return TF_OOM;
    c->p = *pin;
    c->prof_period = 1;
    hipError_t e = hipGetDevice(&c->device);
    if (e != hipSuccess) { ctx_free(c); return tf_from_hip(e); }
    c->W = pin->cols; c->H = pin->rows;
    c->n_total = pin->n_buckets + pin->n_excess;
    for (int l = 0, w = c->W, h = c->H; l < TF_LEVELS; ++l, w /= 2, h /= 2) { c->lw[l] = w; c->lh[l] = h; }
    c->alloc_chunks = (c->n_total + 4095) / 4096;
    c->vis_chunks = c->alloc_chunks;
    const size_t npx = (size_t)c->W * c->H;
    const size_t ntot_pad = (size_t)c->alloc_chunks * 4096;
    c->icp_max_cta = ((c->W + 31) / 32) * ((c->H + 7) / 8);
    // ComputeIcpHelper ctor (projective_icp.cpp:11-15), evaluated on the host like the reference
    c->min_cosine = cosf(pin->icp_angle_thres);
    c->dist2_thres = pin->icp_dist_thres * pin->icp_dist_thres;
    tf_read_env(c);
#define ALLOC(ptr, bytes) do { e = tf_mem_hip(c->mem.alloc(&(ptr), (bytes))); if (e != hipSuccess) { ctx_free(c); return tf_from_hip(e); } } while (0)
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->caller_ev, hipEventDisableTiming);
    if (e != hipSuccess) { ctx_free(c); return tf_from_hip(e); }
    ALLOC(c->hash, sizeof(TfHashEntry) * (size_t)c->n_total);
    ALLOC(c->excessList, sizeof(int) * (size_t)pin->n_excess);
    ALLOC(c->vba_guard, sizeof(TfVoxel) * ((size_t)pin->n_blocks + 1) * TF_BLK3);
    c->vba = c->vba_guard + TF_BLK3;
    ALLOC(c->allocList, sizeof(int) * (size_t)pin->n_blocks);
    ALLOC(c->bgrid, sizeof(int2) * (size_t)TF_GRID_DIM * TF_GRID_DIM * TF_GRID_DIM);
    ALLOC(c->allocType, ntot_pad);
    ALLOC(c->winnerKey, sizeof(int) * ntot_pad);
    ALLOC(c->allocCounts, sizeof(int) * 2 * (size_t)c->alloc_chunks);
    ALLOC(c->visCounts, sizeof(int) * (size_t)c->vis_chunks);
    ALLOC(c->visAgg, sizeof(unsigned long long) * (size_t)c->vis_chunks);
    ALLOC(c->visibleIds, sizeof(int) * (size_t)pin->vis_capacity);
    ALLOC(c->visType, ntot_pad);
    ALLOC(c->range, sizeof(float) * 2 * npx);
    ALLOC(c->range_render, sizeof(float) * 2 * npx);
    ALLOC(c->raycast, sizeof(float) * 4 * npx);
    ALLOC(c->grey, sizeof(uchar4) * npx);
    ALLOC(c->blockRec, sizeof(uint4) * (size_t)pin->vis_capacity);
    ALLOC(c->blockTiles, sizeof(int) * (size_t)pin->vis_capacity);
    ALLOC(c->blockOff, sizeof(int) * (size_t)pin->vis_capacity);
    ALLOC(c->edChunk, sizeof(int) * ((size_t)pin->vis_capacity / 256 + 1));
    ALLOC(c->edSpill, sizeof(int2) * (size_t)ed_nrows(c->H));
    // k_ed_fill: LDS rows up to ed_lds_max_n visible entries, device-scope atomics past that
    if (c->ed_lds_max_n > pin->vis_capacity) c->ed_lds_max_n = pin->vis_capacity;   // (a bin holds <= n boxes)
    // the binned boxes hold 12-bit coordinates (tf_ed.h ed_bin_pack), the fill's LDS rows ED_MAX_ROWS
    if (c->W > ED_MAX_W || c->H > ED_MAX_W) c->ed_lds_max_n = 0;
    // the row bins exist only where binning can run: 2 bins per fill row of ed_lds_max_n boxes each
    if (c->ed_lds_max_n > 0) ALLOC(c->edBins, sizeof(uint4) * 2 * (size_t)ed_nrows(c->H) * (size_t)c->ed_lds_max_n);
    ALLOC(c->edBinCnt, sizeof(int) * 2 * (size_t)ed_nrows(c->H));
    ALLOC(c->edDone, 64);
    {   // the raycast tiles' dispatch order, longest first per XCD region (k_raycast_pair, sorted in
        // k_icp_maps_end's grid from the last frame's workgroup times), where one LDS sort holds an XCD's share;
        // tile_rows: XCD x takes the tile rows = x (mod 8) instead of the x-th band
        const int tx = (c->W + 15) / 16, ty = (c->H + 15) / 16, nt = tx * ty;
        c->tile_slots = c->tile_rows ? 8 * ((ty + 7) / 8) * tx : (nt + 7) / 8 * 8;
        c->tile_ljf = c->tile_slots / 8 <= TF_LJF_MAX && c->tile_ljf;
        ALLOC(c->tile_cost, sizeof(unsigned) * 2 * (size_t)nt);
        ALLOC(c->tile_order, sizeof(int) * 2 * (size_t)c->tile_slots);
    }
    ALLOC(c->depth_in, sizeof(uint16_t) * npx);
    ALLOC(c->dists, sizeof(float) * npx);
    {   // each map's three pyramid levels are contiguous in one allocation
        size_t ntot = 0;
        for (int l = 0; l < TF_LEVELS; ++l) ntot += (size_t)c->lw[l] * c->lh[l];
        ALLOC(c->curr_pts[0], sizeof(float4) * ntot);
        ALLOC(c->curr_nrm[0], sizeof(float4) * ntot);
        ALLOC(c->prev_pts[0], sizeof(float4) * ntot);
        ALLOC(c->prev_nrm[0], sizeof(float4) * ntot);
        for (int l = 1; l < TF_LEVELS; ++l) {
            const size_t off = (size_t)c->lw[l - 1] * c->lh[l - 1];
            c->curr_pts[l] = c->curr_pts[l - 1] + off; c->curr_nrm[l] = c->curr_nrm[l - 1] + off;
            c->prev_pts[l] = c->prev_pts[l - 1] + off; c->prev_nrm[l] = c->prev_nrm[l - 1] + off;
        }
        for (int l = 1; l < TF_LEVELS; ++l) ALLOC(c->depth_pyr[l], sizeof(uint16_t) * (size_t)c->lw[l] * c->lh[l]);
        for (int k = 0; k < 2; ++k) ALLOC(c->d0_buf[k], sizeof(uint16_t) * (size_t)c->lw[0] * c->lh[0]);
        c->depth_pyr[0] = c->d0_buf[0];
    }
    ALLOC(c->icp_partial, sizeof(float) * 28 * 256);
    ALLOC(c->icp_ticket, 64);
    ALLOC(c->icp_tagged, sizeof(unsigned long long) * TF_ICP_TAG_WORDS);
    // the device state, then the per-slot ok / mode rings: one copy back per host sync
    ALLOC(c->st, TF_ST_BYTES);
    c->frame_ok = (int*)(c->st + 1);
    c->frame_mode = c->frame_ok + TF_PROF_RING;
    ALLOC(c->integ_cnt, sizeof(long long) * 2 * TF_INTEG_WG);
    if (pin->use_swapping) {        // the GlobalCache in HBM: 2 KiB per hash entry + flags
        ALLOC(c->swapState, ntot_pad);
        ALLOC(c->swapFlags, ntot_pad);
        ALLOC(c->swapStore, sizeof(TfVoxel) * (size_t)c->n_total * TF_BLK3);
        ALLOC(c->swapCounts, sizeof(int) * 2 * (size_t)c->alloc_chunks);
        e = hipMemsetAsync(c->swapState, 0, ntot_pad, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->swapFlags, 0, ntot_pad, c->stream);
        if (e != hipSuccess) { ctx_free(c); return tf_from_hip(e); }
    }
    if (pin->voxel_rgb) {           // the Voxel_s_rgb colour plane (guard block + n_blocks blocks of 2 KiB)
        const size_t nb = sizeof(unsigned) * ((size_t)pin->n_blocks + 1) * TF_BLK3;
        ALLOC(c->vba_rgb_guard, nb);
        c->vba_rgb = c->vba_rgb_guard + TF_BLK3;
        ALLOC(c->rgb_in, sizeof(uchar4) * npx);
        e = hipMemsetAsync(c->vba_rgb_guard, 0, nb, c->stream);
        if (e != hipSuccess) { ctx_free(c); return tf_from_hip(e); }
    }
#undef ALLOC
    e = tf_mem_hip(c->mem.alloc(TfCtxMem::pin(&c->st_host, TF_ST_BYTES, hipHostMallocDefault)));
    // per-call frames: the verdict record in fine-grained host memory (written by the ICP launch
    // with system-scope stores)
    if (e == hipSuccess)
        e = tf_mem_hip(c->mem.alloc(TfCtxMem::pin(&c->verdict_host, sizeof(unsigned long long) * TF_VERDICT_WORDS, hipHostMallocCoherent)));
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&c->verdict_dev, c->verdict_host, 0);
    if (e != hipSuccess) { ctx_free(c); return tf_from_hip(e); }
    memset(c->verdict_host, 0, sizeof(unsigned long long) * TF_VERDICT_WORDS);
    // initial device state
    TfDevState s0;
    memset(&s0, 0, sizeof(s0));
    for (int i = 0; i < 12; ++i) s0.pose[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    s0.icp_ok = 1;
    e = hipMemcpyAsync(c->st, &s0, sizeof(s0), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->icp_ticket, 0, 64, c->stream);
    if (e == hipSuccess) e = tfk_grid_clear(c);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)c->vba_guard, 0x7fff, TF_BLK3, c->stream);   // Voxel_s()
    if (e == hipSuccess) e = hipMemsetAsync(c->icp_tagged, 0, sizeof(unsigned long long) * TF_ICP_TAG_WORDS, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->integ_cnt, 0, sizeof(long long) * 2 * TF_INTEG_WG, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->visAgg, 0, sizeof(unsigned long long) * (size_t)c->vis_chunks, c->stream);   // no tag yet
    if (e == hipSuccess) e = hipMemsetAsync(c->allocType, 0, ntot_pad, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->winnerKey, 0xff, sizeof(int) * ntot_pad, c->stream);
    // the request pass counts into these; every frame's k_vis_count returns them to zero
    if (e == hipSuccess) e = hipMemsetAsync(c->allocCounts, 0, sizeof(int) * 2 * (size_t)c->alloc_chunks, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->visType, 0, ntot_pad, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->visibleIds, 0, sizeof(int) * (size_t)pin->vis_capacity, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->raycast, 0, sizeof(float) * 4 * npx, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->edBinCnt, 0, sizeof(int) * 2 * (size_t)ed_nrows(c->H), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->edDone, 0, 64, c->stream);
    if (e == hipSuccess) e = tfk_tile_order_init(c);
    if (e == hipSuccess) e = hipMemsetAsync(c->grey, 0, sizeof(uchar4) * npx, c->stream);
    for (int l = 0; l < TF_LEVELS && e == hipSuccess; ++l) {
        size_t n = (size_t)c->lw[l] * c->lh[l];
        e = hipMemsetAsync(c->prev_pts[l], 0, sizeof(float4) * n, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->prev_nrm[l], 0, sizeof(float4) * n, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->curr_pts[l], 0, sizeof(float4) * n, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->curr_nrm[l], 0, sizeof(float4) * n, c->stream);
    }
    if (e != hipSuccess) { ctx_free(c); return tf_from_hip(e); }
    {   // RenderState ctor: renderingRangeImage = (viewFrustum_min, viewFrustum_max) (RenderState.hpp:56-76)
        float2* tmp = (float2*)malloc(sizeof(float2) * npx);
        if (!tmp) { ctx_free(c); return TF_OOM; }
        for (size_t i = 0; i < npx; ++i) tmp[i] = make_float2(pin->viewFrustum_min, pin->viewFrustum_max);
        e = hipMemcpy(c->range, tmp, sizeof(float2) * npx, hipMemcpyHostToDevice);
        free(tmp);
        if (e == hipSuccess) e = ed_spill_all(c);       // the first CreateExpectedDepths clears the whole buffer
        if (e != hipSuccess) { ctx_free(c); return tf_from_hip(e); }
    }
    e = tfk_reset_scene(c);                              // topfu.cpp:75
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = tfk_check_div3(c, pin->mu, &c->mu_exact3);   // integrate: eta / mu
    if (e != hipSuccess) { ctx_free(c); return tf_from_hip(e); }
    // ICP: one persistent launch per frame when all its workgroups fit at once (and the switch allows it);
    // otherwise one k_icp_iter launch per iteration
    if (c->icp_persistent) c->icp_persistent = tfk_icp_persistent_ok(c);
    if (c->icp_persistent) {
        // ordering only (the contexts share no memory): no system-scope fence at the record --
        // with it, each record wrote back and invalidated the caches, a ~5 us dispatch gap after
        // every persistent ICP launch while two contexts exist
        e = hipEventCreateWithFlags(&c->icp_ev, hipEventDisableTiming | hipEventDisableSystemFence);
        if (e != hipSuccess) { c->icp_ev = nullptr; ctx_free(c); return tf_from_hip(e); }
        icp_order_register(c, +1);
    }
    *out = c;
    return TF_OK;
}

extern "C" void tf_destroy(tf_ctx* c)
{
    if (!c) return;
    (void)hipStreamSynchronize(c->stream);
    ctx_free(c);
}

extern "C" tf_status tf_reset(tf_ctx* c)
{
    TF_FLUSH(c);
    if (!c) return TF_INVALID_ARG;
    return ctx_reset(c);
}

extern "C" tf_status tf_get_pose(tf_ctx* c, float rt[12])
{
    TF_FLUSH(c);
    if (!c || !rt) return TF_INVALID_ARG;
    tf_status s = sync_state(c);
    if (s != TF_OK) return s;
    memcpy(rt, c->st_host->pose, sizeof(float) * 12);
    return TF_OK;
}

extern "C" tf_status tf_icp_get_result(tf_ctx* c, float affine_rt[12], float sums[27], int* ok, int* iterations)
{
    TF_FLUSH(c);
    if (!c) return TF_INVALID_ARG;
    tf_status s = sync_state(c);
    if (s != TF_OK) return s;
    if (affine_rt) memcpy(affine_rt, c->st_host->affine, sizeof(float) * 12);
    if (sums) memcpy(sums, c->st_host->sums, sizeof(float) * 27);
    if (ok) *ok = c->st_host->icp_ok;
    if (iterations) *iterations = c->st_host->icp_iters;
    return TF_OK;
}

extern "C" tf_status tf_get_stats(tf_ctx* c, tf_stats* stats)
{
    TF_FLUSH(c);
    if (!c || !stats) return TF_INVALID_ARG;
    tf_status s = sync_state(c);
    if (s != TF_OK) return s;
    fill_stats(c, stats);
    return TF_OK;
}

extern "C" tf_status tf_get_params(tf_ctx* c, tf_params* p)
{
    if (!c || !p) return TF_INVALID_ARG;
    *p = c->p;
    return TF_OK;
}

extern "C" void* tf_get_stream(tf_ctx* c)
{   // (a caller that synchronises the stream itself sees every frame complete)
    if (c) (void)flush_tail(c);
    return c ? (void*)c->stream : nullptr;
}

extern "C" tf_status tf_get_schedule(tf_ctx* c, int* icp_persistent)
{
    if (!c) return TF_INVALID_ARG;
    if (icp_persistent) *icp_persistent = c->icp_persistent;
    return TF_OK;
}

extern "C" tf_status tf_set_pose_algebra(tf_ctx* c, int algebra)
{
    if (!c) return TF_INVALID_ARG;
    if (algebra != TF_POSE_ALGEBRA_CANONICAL && algebra != TF_POSE_ALGEBRA_OPENCV2 && algebra != TF_POSE_ALGEBRA_OPENCV4)
        return TF_INVALID_ARG;
    TF_FLUSH(c);
    const int old = c->pose_alg;
    c->pose_alg = algebra;
    if (c->icp_persistent && !tfk_icp_persistent_ok(c)) {     // the schedule stays what tf_create chose
        c->pose_alg = old;
        return TF_INVALID_ARG;
    }
    return TF_OK;
}

extern "C" tf_status tf_get_pose_algebra(tf_ctx* c, int* algebra)
{
    if (!c || !algebra) return TF_INVALID_ARG;
    *algebra = c->pose_alg;
    return TF_OK;
}

// ---- state transfer -------------------------------------------------------------------
static void* buffer_ptr(tf_ctx* c, int which, int level, size_t* bytes)
{
    const size_t npx = (size_t)c->W * c->H;
    if (level < 0 || level >= TF_LEVELS) level = 0;
    const size_t nl = (size_t)c->lw[level] * c->lh[level];
    switch (which) {
    case TF_BUF_HASH: *bytes = sizeof(TfHashEntry) * (size_t)c->n_total; return c->hash;
    case TF_BUF_VBA: *bytes = sizeof(TfVoxel) * (size_t)c->p.n_blocks * TF_BLK3; return c->vba;
    case TF_BUF_VISIBLE_IDS: *bytes = sizeof(int) * (size_t)c->p.vis_capacity; return c->visibleIds;
    case TF_BUF_VISIBLE_TYPE: *bytes = (size_t)c->n_total; return c->visType;
    case TF_BUF_RANGE: *bytes = sizeof(float) * 2 * npx; return c->range;
    case TF_BUF_RAYCAST: *bytes = sizeof(float) * 4 * npx; return c->raycast;
    case TF_BUF_DISTS: *bytes = sizeof(float) * npx; return c->dists;
    case TF_BUF_DEPTH: *bytes = sizeof(uint16_t) * nl; return c->depth_pyr[level];
    case TF_BUF_CURR_POINTS: *bytes = sizeof(float4) * nl; return c->curr_pts[level];
    case TF_BUF_CURR_NORMALS: *bytes = sizeof(float4) * nl; return c->curr_nrm[level];
    case TF_BUF_PREV_POINTS: *bytes = sizeof(float4) * nl; return c->prev_pts[level];
    case TF_BUF_PREV_NORMALS: *bytes = sizeof(float4) * nl; return c->prev_nrm[level];
    case TF_BUF_GREY: *bytes = sizeof(uchar4) * npx; return c->grey;
    case TF_BUF_SWAP_STATE: *bytes = c->swapState ? (size_t)c->n_total : 0; return c->swapState;
    case TF_BUF_SWAP_STORED_FLAGS: *bytes = c->swapFlags ? (size_t)c->n_total : 0; return c->swapFlags;
    case TF_BUF_SWAP_STORED: *bytes = c->swapStore ? sizeof(TfVoxel) * (size_t)c->n_total * TF_BLK3 : 0; return c->swapStore;
    case TF_BUF_VBA_RGB: *bytes = c->vba_rgb ? sizeof(unsigned) * (size_t)c->p.n_blocks * TF_BLK3 : 0; return c->vba_rgb;
    case TF_BUF_ALLOC_LIST: *bytes = sizeof(int) * (size_t)c->p.n_blocks; return c->allocList;
    case TF_BUF_EXCESS_LIST: *bytes = sizeof(int) * (size_t)c->p.n_excess; return c->excessList;
    }
    *bytes = 0;
    return nullptr;
}

extern "C" tf_status tf_buffer_bytes(tf_ctx* c, int which, int level, size_t* bytes)
{
    TF_FLUSH(c);
    if (!c || !bytes) return TF_INVALID_ARG;
    return buffer_ptr(c, which, level, bytes) ? TF_OK : TF_INVALID_ARG;
}

extern "C" tf_status tf_download(tf_ctx* c, int which, int level, void* host, size_t bytes)
{
    TF_FLUSH(c);
    if (!c || !host) return TF_INVALID_ARG;
    size_t n;
    void* p = buffer_ptr(c, which, level, &n);
    if (!p || n != bytes) return TF_INVALID_ARG;
    TF_CHECK(hipMemcpyAsync(host, p, n, hipMemcpyDeviceToHost, c->stream));
    return sync_checked(c);
}

extern "C" tf_status tf_download_range(tf_ctx* c, int which, size_t offset, void* host, size_t bytes)
{
    TF_FLUSH(c);
    if (!c || !host) return TF_INVALID_ARG;
    size_t n;
    void* p = buffer_ptr(c, which, 0, &n);
    if (!p || offset > n || bytes > n - offset) return TF_INVALID_ARG;
    TF_CHECK(hipMemcpyAsync(host, (const char*)p + offset, bytes, hipMemcpyDeviceToHost, c->stream));
    return sync_checked(c);
}

extern "C" tf_status tf_upload(tf_ctx* c, int which, int level, const void* host, size_t bytes)
{
    TF_FLUSH(c);
    if (!c || !host) return TF_INVALID_ARG;
    size_t n;
    void* p = buffer_ptr(c, which, level, &n);
    if (!p || n != bytes) return TF_INVALID_ARG;
    TF_CHECK(hipMemcpyAsync(p, host, n, hipMemcpyHostToDevice, c->stream));
    if (which == TF_BUF_HASH) TF_CHECK(tfk_grid_rebuild(c));       // keep the block grid exact
    if (which == TF_BUF_RANGE) TF_CHECK(ed_spill_all(c));          // next CreateExpectedDepths: whole buffer
    static const int one = 1;
    if (which == TF_BUF_VISIBLE_TYPE || which == TF_BUF_VISIBLE_IDS)   // types 3 off the list (tf_vis.h)
        TF_CHECK(hipMemcpyAsync((char*)c->st + offsetof(TfDevState, vis_stale), &one, sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (which == TF_BUF_HASH || which == TF_BUF_VBA || which == TF_BUF_VBA_RGB || which == TF_BUF_ALLOC_LIST ||
        which == TF_BUF_EXCESS_LIST)                               // next reset (in-frame ones too): full clear
        TF_CHECK(hipMemcpyAsync((char*)c->st + offsetof(TfDevState, scene_external), &one, sizeof(int), hipMemcpyHostToDevice, c->stream));
    return sync_checked(c);
}

extern "C" tf_status tf_set_pose(tf_ctx* c, const float rt[12])
{
    TF_FLUSH(c);
    if (!c || !rt) return TF_INVALID_ARG;
    TF_CHECK(hipMemcpyAsync(c->st->pose, rt, sizeof(float) * 12, hipMemcpyHostToDevice, c->stream));
    return sync_checked(c);
}

extern "C" tf_status tf_set_counters(tf_ctx* c, int lastFreeBlockId, int lastFreeExcessListId, int noVisibleEntries)
{
    TF_FLUSH(c);
    if (!c) return TF_INVALID_ARG;
    tf_status s = sync_state(c);
    if (s != TF_OK) return s;
    c->st_host->lastFreeBlockId = lastFreeBlockId;
    c->st_host->lastFreeExcessListId = lastFreeExcessListId;
    c->st_host->noVisibleEntries = noVisibleEntries;
    c->st_host->vis_stale = 1;                                      // the list no longer vouches for every type 3
    c->st_host->scene_external = 1;                                 // next reset: full clear
    TF_CHECK(hipMemcpyAsync(c->st, c->st_host, sizeof(TfDevState), hipMemcpyHostToDevice, c->stream));
    return sync_checked(c);
}

extern "C" tf_status tf_get_totals(tf_ctx* c, tf_totals* t)
{
    TF_FLUSH(c);
    if (!c || !t) return TF_INVALID_ARG;
    tf_status s = sync_state(c);
    if (s != TF_OK) return s;
    const TfDevState* d = c->st_host;
    t->frames = d->tot_frames; t->frames_tracked = d->tot_tracked; t->resets = d->tot_resets;
    t->visible_sum = d->tot_visible; t->tiles_sum = d->tot_tiles;
    t->swapped_in = d->tot_swap_in; t->swapped_out = d->tot_swap_out;
    t->swapped_in_merged = d->tot_swap_merged;
    t->alloc_failed_type1 = d->tot_alloc_fail1; t->alloc_failed_type2 = d->tot_alloc_fail2;
    t->icp_fallbacks = c->icp_fallbacks;
    t->integrate_lanes_read = t->integrate_lanes_written = 0;
    std::vector<long long> h(2 * TF_INTEG_WG);
    TF_CHECK(hipMemcpyAsync(h.data(), c->integ_cnt, sizeof(long long) * h.size(), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < TF_INTEG_WG; ++i) { t->integrate_lanes_read += h[2 * i]; t->integrate_lanes_written += h[2 * i + 1]; }
    return TF_OK;
}

extern "C" tf_status tf_reset_totals(tf_ctx* c)
{
    TF_FLUSH(c);
    if (!c) return TF_INVALID_ARG;
    const size_t b = offsetof(TfDevState, tot_frames), e = offsetof(TfDevState, tot_alloc_fail2) + sizeof(long long);
    TF_CHECK(hipMemsetAsync((char*)c->st + b, 0, e - b, c->stream));
    TF_CHECK(hipMemsetAsync(c->integ_cnt, 0, sizeof(long long) * 2 * TF_INTEG_WG, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    c->icp_fallbacks = 0;
    return TF_OK;
}
