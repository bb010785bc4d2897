// tf_engines.hip -- the entry points beside the frame: the tracker's stages one at a time (tf_stage_*,
// tf_time_stage), tf_render_image*, and the engine entry points over caller buffers (tf_icp_*, tf_scene_*,
// tf_vis_*, tf_swap_*; include/tfusion/engines.hpp).  Every one is synchronous: flush, launches, sync_checked.
#include "tf_host.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

// stage entry points run the tracking-path kernels unconditionally
__global__ void k_stage_begin(TfDevState* st)
{
    st->abort = 0;
    st->mode = 1;
}

static hipError_t clear_abort(tf_ctx* c)
{
    hipLaunchKernelGGL(k_stage_begin, dim3(1), dim3(1), 0, c->stream, c->st);
    return hipGetLastError();
}

static void swap_pyramids(tf_ctx* c)
{
    for (int l = 0; l < TF_LEVELS; ++l) {
        float4* t = c->curr_pts[l]; c->curr_pts[l] = c->prev_pts[l]; c->prev_pts[l] = t;
        t = c->curr_nrm[l]; c->curr_nrm[l] = c->prev_nrm[l]; c->prev_nrm[l] = t;
    }
}

extern "C" tf_status tf_render_image(tf_ctx* c, uint8_t* dev_rgba, size_t pitch)
{   // TopFu::renderImage: raycast from poses_.back() with the current range image + grey
    TF_FLUSH(c);
    return tf_render_image_type(c, TF_RENDER_SHADED_GREYSCALE, dev_rgba, pitch);
}

extern "C" tf_status tf_render_image_type(tf_ctx* c, int type, uint8_t* dev_rgba, size_t pitch)
{   // VisualisationEngine_CUDA::RenderImage(..., type, RENDER_FROM_NEW_RAYCAST) from poses_.back()
    TF_FLUSH(c);
    if (!c || type < TF_RENDER_SHADED_GREYSCALE || type > TF_RENDER_COLOUR_FROM_CONFIDENCE) return TF_INVALID_ARG;
    TF_CHECK(clear_abort(c));
    TF_CHECK(hipMemcpyAsync(c->st->pose_in, c->st->pose, sizeof(float) * 12, hipMemcpyDeviceToDevice, c->stream));
    TF_CHECK(tfk_pose_from_input(c, 0));
    TF_CHECK(tfk_raycast(c, 0));
    TF_CHECK(tfk_render_type(c, type));
    if (dev_rgba) {
        if (pitch == 0) pitch = (size_t)c->W * 4;
        TF_CHECK(hipMemcpy2DAsync(dev_rgba, pitch, c->grey, (size_t)c->W * 4, (size_t)c->W * 4, c->H,
                                  hipMemcpyDeviceToDevice, c->stream));
    }
    return sync_checked(c);
}

// ---- stage entry points ---------------------------------------------------------------
// the call's pose into the device state; the tracking-path kernels run after it (clear_abort: st->mode = 1)
static tf_status set_pose_in(tf_ctx* c, const float* rt, int mode)
{
    TF_CHECK(clear_abort(c));
    TF_CHECK(hipMemcpyAsync(c->st->pose_in, rt, sizeof(float) * 12, hipMemcpyHostToDevice, c->stream));
    TF_CHECK(tfk_pose_from_input(c, mode));
    return TF_OK;
}

// what the pose-taking entry points share after their flush: argument check, the pose, the launches, the wait
template <class Launch>
static tf_status pose_stage(tf_ctx* c, const float* rt, int mode, Launch launch)
{
    if (!c || !rt) return TF_INVALID_ARG;
    const tf_status s = set_pose_in(c, rt, mode);
    if (s != TF_OK) return s;
    TF_CHECK(launch());
    return sync_checked(c);
}

extern "C" tf_status tf_stage_preprocess(tf_ctx* c, const uint16_t* dev_depth, size_t pitch)
{
    TF_FLUSH(c);
    if (!c || !dev_depth) return TF_INVALID_ARG;
    if (pitch == 0) pitch = (size_t)c->W * 2;
    TF_CHECK(clear_abort(c));
    TF_CHECK(tfk_preprocess(c, dev_depth, pitch, c->stream, c->d0_buf[0]));
    c->depth_pyr[0] = c->d0_buf[0];
    return sync_checked(c);
}

extern "C" tf_status tf_stage_preprocess_host(tf_ctx* c, const uint16_t* host_depth, size_t pitch)
{
    TF_FLUSH(c);
    if (!c || !host_depth) return TF_INVALID_ARG;
    if (pitch == 0) pitch = (size_t)c->W * 2;
    TF_CHECK(upload_depth(c, host_depth, pitch));
    return tf_stage_preprocess(c, c->depth_in, (size_t)c->W * 2);
}

extern "C" tf_status tf_stage_icp(tf_ctx* c, float affine_rt[12], int* ok, int* iterations)
{
    TF_FLUSH(c);
    if (!c) return TF_INVALID_ARG;
    TF_CHECK(clear_abort(c));                      // tracking-path kernels run (st->mode = 1)
    TF_CHECK(tfk_icp(c, 0));
    tf_status s = sync_state(c);
    if (s != TF_OK) return s;
    if (c->st_host->icp_ok < 0) return TF_HIP_ERROR;
    if (affine_rt) memcpy(affine_rt, c->st_host->affine, sizeof(float) * 12);
    if (ok) *ok = c->st_host->icp_ok;
    if (iterations) *iterations = c->st_host->icp_iters;
    TF_CHECK(clear_abort(c));
    return TF_OK;
}

extern "C" tf_status tf_stage_alloc(tf_ctx* c, const float pose_rt[12])
{
    TF_FLUSH(c);
    return pose_stage(c, pose_rt, TF_POSE_ALLOC_NOINV, [&] { return tfk_alloc(c); });
}

extern "C" tf_status tf_stage_integrate(tf_ctx* c, const float pose_rt[12])
{
    TF_FLUSH(c);
    return pose_stage(c, pose_rt, TF_POSE_ALLOC_NOINV, [&] { return tfk_integrate(c); });
}

extern "C" tf_status tf_stage_expected_depths(tf_ctx* c, const float pose_rt[12])
{
    TF_FLUSH(c);
    return pose_stage(c, pose_rt, TF_POSE_ALLOC_NOINV, [&] { return tfk_expected_depths(c); });
}

extern "C" tf_status tf_stage_raycast(tf_ctx* c, const float invM_rt[12], int update_visible)
{
    TF_FLUSH(c);
    return pose_stage(c, invM_rt, 0, [&] { return tfk_raycast(c, update_visible); });
}

extern "C" tf_status tf_stage_icp_maps(tf_ctx* c, const float invM_rt[12])
{
    TF_FLUSH(c);
    return pose_stage(c, invM_rt, 0, [&] { return tfk_icp_maps(c); });
}

extern "C" tf_status tf_stage_render_grey(tf_ctx* c, const float invM_rt[12])
{
    TF_FLUSH(c);
    return pose_stage(c, invM_rt, 0, [&] { return tfk_render_type(c, TF_RENDER_SHADED_GREYSCALE); });
}

extern "C" tf_status tf_time_stage(tf_ctx* c, int stage, const float pose_rt[12], int iters, float* ms_per_iter)
{
    TF_FLUSH(c);
    if (!c || !pose_rt || iters <= 0 || !ms_per_iter) return TF_INVALID_ARG;
    if (stage != TF_STAGE_INTEGRATE && stage != TF_STAGE_RAYCAST_ICP && stage != TF_STAGE_RAYCAST_RENDER &&
        stage != TF_STAGE_EXPECTED_DEPTHS)
        return TF_INVALID_ARG;
    tf_status s = set_pose_in(c, pose_rt, stage == TF_STAGE_INTEGRATE || stage == TF_STAGE_EXPECTED_DEPTHS ? TF_POSE_ALLOC_NOINV : 0);
    if (s != TF_OK) return s;
    if (stage == TF_STAGE_EXPECTED_DEPTHS) TF_CHECK(tfk_expected_depths(c, 0, 1));    // boxes of the current list
    // the pair's renderImage half reads the snapshot of the raycast matrix / range region
    if (stage == TF_STAGE_RAYCAST_RENDER) TF_CHECK(tfk_render_snapshot(c));
    hipEvent_t e0, e1;
    TF_CHECK(hipEventCreate(&e0));
    TF_CHECK(hipEventCreate(&e1));
    hipError_t e = hipEventRecord(e0, c->stream);
    for (int i = 0; i < iters && e == hipSuccess; ++i)
        e = stage == TF_STAGE_INTEGRATE ? tfk_integrate(c)
          : stage == TF_STAGE_EXPECTED_DEPTHS ? tfk_expected_depths(c, 1, 1)
          : stage == TF_STAGE_RAYCAST_ICP ? tfk_raycast(c, 1) : tfk_raycast_pair_ordered(c);
    if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    // the repeated fills kept the bins: empty them for the next projection pass
    if (e == hipSuccess && stage == TF_STAGE_EXPECTED_DEPTHS)
        e = hipMemsetAsync(c->edBinCnt, 0, sizeof(int) * 2 * (size_t)ed_nrows(c->H), c->stream);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (e != hipSuccess) return tf_from_hip(e);
    *ms_per_iter = ms / (float)iters;
    return TF_OK;
}

extern "C" tf_status tf_stage_reset_scene(tf_ctx* c)
{   // SceneReconstructionEngine::ResetScene: the GlobalCache stays (SceneReconstructionEngine_host.cu:51-73)
    TF_FLUSH(c);
    if (!c) return TF_INVALID_ARG;
    TF_CHECK(tfk_reset_scene(c, 0));
    return sync_checked(c);
}

extern "C" tf_status tf_stage_swap_pyramids(tf_ctx* c)
{
    TF_FLUSH(c);
    if (!c) return TF_INVALID_ARG;
    swap_pyramids(c);
    return TF_OK;
}

// ---- engine entry points over caller buffers (include/tfusion/engines.hpp) -------------
// the call's intrinsics (the reference engines take Intr per call) in place of the context's
// for as long as the scope lives; every launcher reads c->p when it builds its arguments
struct IntrScope {
    tf_ctx* c;
    float saved[4];
    IntrScope(tf_ctx* ctx, const float* intr) : c(ctx)
    {
        saved[0] = c->p.fx; saved[1] = c->p.fy; saved[2] = c->p.cx; saved[3] = c->p.cy;
        if (intr) { c->p.fx = intr[0]; c->p.fy = intr[1]; c->p.cx = intr[2]; c->p.cy = intr[3]; }
    }
    ~IntrScope() { c->p.fx = saved[0]; c->p.fy = saved[1]; c->p.cx = saved[2]; c->p.cy = saved[3]; }
};

extern "C" tf_status tf_icp_set_params(tf_ctx* c, float dist_thres, float angle_thres, const int iters[4])
{
    TF_FLUSH(c);
    if (!c || !iters || !(dist_thres >= 0) || !(angle_thres >= 0)) return TF_INVALID_ARG;
    if (iters[3] != 0) return TF_INVALID_ARG;            // three pyramid levels (TF_LEVELS)
    for (int l = 0; l < 4; ++l) if (iters[l] < 0) return TF_INVALID_ARG;
    c->p.icp_dist_thres = dist_thres;
    c->p.icp_angle_thres = angle_thres;
    for (int l = 0; l < 4; ++l) c->p.icp_iter_num[l] = iters[l];
    // ComputeIcpHelper ctor (projective_icp.cpp:11-15)
    c->min_cosine = cosf(angle_thres);
    c->dist2_thres = dist_thres * dist_thres;
    return TF_OK;
}

extern "C" tf_status tf_icp_get_params(tf_ctx* c, float* dist_thres, float* angle_thres, int iters[4])
{
    TF_FLUSH(c);
    if (!c) return TF_INVALID_ARG;
    if (dist_thres) *dist_thres = c->p.icp_dist_thres;
    if (angle_thres) *angle_thres = c->p.icp_angle_thres;
    if (iters) for (int l = 0; l < 4; ++l) iters[l] = c->p.icp_iter_num[l];
    return TF_OK;
}

// caller pitched float4 map -> the context's packed level buffer
static hipError_t copy_map_in(tf_ctx* c, float4* dst, int l, const void* src, size_t step)
{
    const size_t row = sizeof(float4) * (size_t)c->lw[l];
    return hipMemcpy2DAsync(dst, row, src, step ? step : row, row, c->lh[l], hipMemcpyDeviceToDevice, c->stream);
}

extern "C" tf_status tf_icp_estimate(tf_ctx* c, const float intr[4], const tf_map_level* curr, const tf_map_level* prev,
                                     int levels, float affine_rt[12], int* ok, int* iterations)
{
    TF_FLUSH(c);
    if (!c || !curr || !prev || levels < 1 || levels > TF_LEVELS) return TF_INVALID_ARG;
    int used = 4;                                         // getUsedLevelsNum (projective_icp.cpp:103-108)
    while (used > 0 && c->p.icp_iter_num[used - 1] == 0) --used;
    if (used > levels) return TF_INVALID_ARG;
    for (int l = 0; l < levels; ++l)
        if (!curr[l].points || !curr[l].normals || !prev[l].points || !prev[l].normals) return TF_INVALID_ARG;
    TF_CHECK(order_after_caller(c));
    for (int l = 0; l < levels; ++l) {
        TF_CHECK(copy_map_in(c, c->curr_pts[l], l, curr[l].points, curr[l].points_step));
        TF_CHECK(copy_map_in(c, c->curr_nrm[l], l, curr[l].normals, curr[l].normals_step));
        TF_CHECK(copy_map_in(c, c->prev_pts[l], l, prev[l].points, prev[l].points_step));
        TF_CHECK(copy_map_in(c, c->prev_nrm[l], l, prev[l].normals, prev[l].normals_step));
    }
    IntrScope is(c, intr);
    return tf_stage_icp(c, affine_rt, ok, iterations);
}

// caller dists (pitched) -> the context's dists buffer
static hipError_t copy_dists_in(tf_ctx* c, const float* dists, size_t step)
{
    const size_t row = sizeof(float) * (size_t)c->W;
    return hipMemcpy2DAsync(c->dists, row, dists, step ? step : row, row, c->H, hipMemcpyDeviceToDevice, c->stream);
}

extern "C" tf_status tf_scene_alloc(tf_ctx* c, const float intr[4], const float pose_rt[12], const float* dists,
                                   size_t dists_step, int only_update_visible_list, int reset_visible_list)
{
    TF_FLUSH(c);
    if (!c || !pose_rt || !dists) return TF_INVALID_ARG;
    TF_CHECK(order_after_caller(c));
    TF_CHECK(copy_dists_in(c, dists, dists_step));
    IntrScope is(c, intr);
    return pose_stage(c, pose_rt, TF_POSE_ALLOC_NOINV, [&] {
        hipError_t e = hipSuccess;
        if (reset_visible_list) {      // renderState_vh->noVisibleEntries = 0 (SceneReconstructionEngine_host.cu:88)
            static const int zero = 0, one = 1;
            e = hipMemcpyAsync((char*)c->st + offsetof(TfDevState, noVisibleEntries), &zero, sizeof(int), hipMemcpyHostToDevice,
                               c->stream);
            // the entries of the dropped list keep their types: those still of type 3 are tested all the same (tf_vis.h)
            if (e == hipSuccess)
                e = hipMemcpyAsync((char*)c->st + offsetof(TfDevState, vis_stale), &one, sizeof(int), hipMemcpyHostToDevice, c->stream);
        }
        return e == hipSuccess ? tfk_alloc(c, 0, TfAhead{}, 0, only_update_visible_list ? 1 : 0) : e;
    });
}

extern "C" tf_status tf_scene_integrate(tf_ctx* c, const float intr[4], const float pose_rt[12], const float* dists,
                                       size_t dists_step)
{
    TF_FLUSH(c);
    if (!c || !pose_rt || !dists) return TF_INVALID_ARG;
    TF_CHECK(order_after_caller(c));
    TF_CHECK(copy_dists_in(c, dists, dists_step));
    IntrScope is(c, intr);
    return pose_stage(c, pose_rt, TF_POSE_ALLOC_NOINV, [&] { return tfk_integrate(c); });
}

extern "C" tf_status tf_scene_integrate_rgb(tf_ctx* c, const float intr[4], const float pose_rt[12], const float* dists,
                                           size_t dists_step, const uint8_t* dev_rgb, size_t rgb_step)
{
    TF_FLUSH(c);
    if (!c || !pose_rt || !dists) return TF_INVALID_ARG;
    if (dev_rgb && !c->p.voxel_rgb) return TF_INVALID_ARG;
    RgbScope rs(c, dev_rgb, rgb_step);
    return tf_scene_integrate(c, intr, pose_rt, dists, dists_step);
}

static tf_status scene_swap(tf_ctx* c, int which)
{
    if (!c) return TF_INVALID_ARG;
    if (!c->p.use_swapping) return TF_INVALID_ARG;
    TF_CHECK(clear_abort(c));
    TF_CHECK(tfk_swap(c, which));
    return sync_checked(c);
}

extern "C" tf_status tf_scene_swap(tf_ctx* c) { TF_FLUSH(c); return scene_swap(c, 3); }
extern "C" tf_status tf_scene_swap_in(tf_ctx* c) { TF_FLUSH(c); return scene_swap(c, 1); }
extern "C" tf_status tf_scene_swap_out(tf_ctx* c) { TF_FLUSH(c); return scene_swap(c, 2); }

hipError_t tfk_fuse_frames(tf_ctx* c, const uint16_t* frames, size_t stride, size_t pitch, int n);   // tf_fuse.hip

extern "C" tf_status tf_scene_fuse_frames(tf_ctx* c, const float intr[4], const uint16_t* dev_frames, size_t stride,
                                         size_t pitch, const float* poses_rt, int n, tf_fuse_record* records)
{
    TF_FLUSH(c);
    if (!c || !dev_frames || !poses_rt || n < 0) return TF_INVALID_ARG;
    if (pitch == 0) pitch = (size_t)c->W * 2;
    if (pitch < (size_t)c->W * 2 || (n > 1 && stride < pitch * (size_t)c->H)) return TF_INVALID_ARG;
    if (c->st_host->sticky_error) return TF_HIP_ERROR;     // (in error since an earlier call: nothing runs)
    if (n == 0) return TF_OK;
    if (n > c->fuse_cap) {              // the pose / record lists grow to the largest batch seen
        TF_CHECK(hipStreamSynchronize(c->stream));
        c->fuse_cap = 0;
        TF_CHECK(tf_mem_hip(c->mem.release(c->fuse_pose)));
        TF_CHECK(tf_mem_hip(c->mem.release(c->fuse_rec)));
        TF_CHECK(tf_mem_hip(c->mem.alloc_group({ TfCtxMem::dev(&c->fuse_pose, sizeof(float) * 12 * (size_t)n),
                                                 TfCtxMem::dev(&c->fuse_rec, sizeof(tf_fuse_record) * (size_t)n) })));
        c->fuse_cap = n;
    }
    TF_CHECK(order_after_caller(c));
    TF_CHECK(hipMemcpyAsync(c->fuse_pose, poses_rt, sizeof(float) * 12 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    IntrScope is(c, intr);
    TF_CHECK(tfk_fuse_frames(c, dev_frames, stride, pitch, n));
    if (records)
        TF_CHECK(hipMemcpyAsync(records, c->fuse_rec, sizeof(tf_fuse_record) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    return sync_checked(c);
}

extern "C" tf_status tf_swap_counts(tf_ctx* c, int counts[3])
{
    TF_FLUSH(c);
    if (!c || !counts) return TF_INVALID_ARG;
    tf_status s = sync_state(c);
    if (s != TF_OK) return s;
    counts[0] = c->st_host->swap_in; counts[1] = c->st_host->swap_out; counts[2] = c->st_host->swap_realloc;
    return TF_OK;
}

// GlobalCache::SaveToFile / ReadFromFile (GlobalCache.hpp:79-110): hasStoredData (1 byte per
// entry), then 512 voxels of 4 bytes per entry
extern "C" tf_status tf_swap_save(tf_ctx* c, const char* path)
{
    TF_FLUSH(c);
    if (!c || !path || !c->p.use_swapping) return TF_INVALID_ARG;
    const size_t nf = (size_t)c->n_total, nv = sizeof(TfVoxel) * (size_t)c->n_total * TF_BLK3;
    void* host = malloc(nf + nv);
    if (!host) return TF_OOM;
    hipError_t e = hipMemcpyAsync(host, c->swapFlags, nf, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync((char*)host + nf, c->swapStore, nv, hipMemcpyDeviceToHost, c->stream);
    tf_status s = tf_from_hip(e);
    if (s == TF_OK) s = sync_checked(c);
    if (s == TF_OK) {
        FILE* f = fopen(path, "wb");
        if (!f || fwrite(host, 1, nf + nv, f) != nf + nv) s = TF_INVALID_ARG;
        if (f) fclose(f);
    }
    free(host);
    return s;
}

extern "C" tf_status tf_swap_load(tf_ctx* c, const char* path)
{
    TF_FLUSH(c);
    if (!c || !path || !c->p.use_swapping) return TF_INVALID_ARG;
    const size_t nf = (size_t)c->n_total, nv = sizeof(TfVoxel) * (size_t)c->n_total * TF_BLK3;
    FILE* f = fopen(path, "rb");
    if (!f) return TF_INVALID_ARG;
    void* host = malloc(nf + nv);
    if (!host) { fclose(f); return TF_OOM; }
    const size_t got = fread(host, 1, nf + nv, f);
    fclose(f);
    tf_status s = TF_OK;
    if (got == nf + nv) {       // the reference reads the blocks only when the flags are complete
        hipError_t e = hipMemcpyAsync(c->swapFlags, host, nf, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c->swapStore, (char*)host + nf, nv, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        s = tf_from_hip(e);
    } else s = TF_INVALID_ARG;
    free(host);
    return s;
}

extern "C" tf_status tf_vis_expected_depths(tf_ctx* c, const float intr[4], const float pose_rt[12])
{
    TF_FLUSH(c);
    if (!c || !pose_rt) return TF_INVALID_ARG;
    IntrScope is(c, intr);
    return tf_stage_expected_depths(c, pose_rt);
}

extern "C" tf_status tf_vis_render_image(tf_ctx* c, const float intr[4], const float pose_rt[12], int type, int new_raycast,
                                        uint8_t* dev_rgba, size_t step)
{
    TF_FLUSH(c);
    if (!c || !pose_rt || type < TF_RENDER_SHADED_GREYSCALE || type > TF_RENDER_COLOUR_FROM_CONFIDENCE) return TF_INVALID_ARG;
    IntrScope is(c, intr);
    tf_status s = set_pose_in(c, pose_rt, 0);
    if (s != TF_OK) return s;
    if (new_raycast) TF_CHECK(tfk_raycast(c, 0));        // RENDER_FROM_NEW_RAYCAST (VisualisationEngine_CUDA.cu:227-240)
    TF_CHECK(tfk_render_type(c, type));
    if (dev_rgba) {
        TF_CHECK(order_after_caller(c));                  // the caller may still read the image on stream 0
        const size_t row = (size_t)c->W * 4;
        TF_CHECK(hipMemcpy2DAsync(dev_rgba, step ? step : row, c->grey, row, row, c->H, hipMemcpyDeviceToDevice, c->stream));
    }
    return sync_checked(c);
}

extern "C" tf_status tf_vis_icp_maps(tf_ctx* c, const float intr[4], const float pose_rt[12], void* points,
                                    size_t points_step, void* normals, size_t normals_step)
{
    TF_FLUSH(c);
    if (!c || !pose_rt) return TF_INVALID_ARG;
    IntrScope is(c, intr);
    tf_status s = set_pose_in(c, pose_rt, 0);
    if (s != TF_OK) return s;
    TF_CHECK(tfk_raycast(c, 1));                          // castRay<true> (VisualisationEngine_CUDA.cu:340-345)
    TF_CHECK(tfk_icp_maps(c));                            // renderICP (:347-359) + the context's resized levels
    const size_t row = sizeof(float4) * (size_t)c->W;
    if (points || normals) TF_CHECK(order_after_caller(c));
    if (points)
        TF_CHECK(hipMemcpy2DAsync(points, points_step ? points_step : row, c->prev_pts[0], row, row, c->H,
                                  hipMemcpyDeviceToDevice, c->stream));
    if (normals)
        TF_CHECK(hipMemcpy2DAsync(normals, normals_step ? normals_step : row, c->prev_nrm[0], row, row, c->H,
                                  hipMemcpyDeviceToDevice, c->stream));
    return sync_checked(c);
}
