// tf_host.h -- what the host layer's translation units share (tf_capi.hip: the context; tf_frame.hip:
// TopFu::operator(); tf_engines.hip: the stage and engine entry points; the mesh and checkpoint entry points
// below their launchers in tf_mesh.hip and tf_scene_ckpt.hip).  Host only; nothing here is exported.
#pragma once
#include "tf_internal.h"

#include <string.h>

#pragma GCC visibility push(hidden)

static inline tf_status tf_from_hip(hipError_t e)
{
    if (e == hipSuccess) return TF_OK;
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return TF_OOM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return TF_NO_DEVICE;
    return TF_HIP_ERROR;
}

#define TF_CHECK(expr)                                   \
    do {                                                 \
        hipError_t e_ = (expr);                          \
        if (e_ != hipSuccess) return tf_from_hip(e_);    \
    } while (0)

// A deferred per-call frame's last two launches (tf_frame.hip); every entry point but the per-call frame
// itself first completes them
tf_status flush_tail(tf_ctx* c, TfAhead nxt = TfAhead{}, size_t pitch = 0);
#define TF_FLUSH(c) do { if (c) { const tf_status fs_ = flush_tail(c); if (fs_ != TF_OK) return fs_; } } while (0)

// the ends of a synchronous entry point (tf_capi.hip): the whole device state to st_host, or the error flag alone
tf_status sync_state(tf_ctx* c);
tf_status sync_checked(tf_ctx* c);

// The context stream is non-blocking, so it does not wait for the legacy default stream on
// which the reference-shaped callers produce their inputs (cuda:: imgproc wrappers with
// stream 0, asynchronous uploads): in the reference everything runs on the default stream and
// that order is implicit.  Entry points that read caller device buffers therefore make the
// context stream wait for all work already enqueued on stream 0 before their first read.
static inline hipError_t order_after_caller(tf_ctx* c)
{
    hipError_t e = hipEventRecord(c->caller_ev, nullptr);
    return e == hipSuccess ? hipStreamWaitEvent(c->stream, c->caller_ev, 0) : e;
}

// the view's RGB image for the integrations enqueued while in scope (voxel_rgb)
struct RgbScope {
    tf_ctx* c;
    RgbScope(tf_ctx* ctx, const uint8_t* rgb, size_t pitch) : c(ctx)
    {
        c->rgb_cur = (const uchar4*)rgb;
        c->rgb_pitch = pitch ? pitch : (size_t)c->W * 4;
    }
    ~RgbScope() { c->rgb_cur = nullptr; }
};

// a host depth / RGB image (rows `pitch` bytes apart) into the context's packed staging buffer
static inline hipError_t upload_depth(tf_ctx* c, const uint16_t* host_depth, size_t pitch)
{
    return hipMemcpy2DAsync(c->depth_in, (size_t)c->W * 2, host_depth, pitch, (size_t)c->W * 2, c->H, hipMemcpyHostToDevice,
                            c->stream);
}
static inline hipError_t upload_rgb(tf_ctx* c, const uint8_t* host_rgb, size_t pitch)
{
    return hipMemcpy2DAsync(c->rgb_in, (size_t)c->W * 4, host_rgb, pitch, (size_t)c->W * 4, c->H, hipMemcpyHostToDevice,
                            c->stream);
}

// tf_stats from the state of the last sync
static inline void fill_stats(tf_ctx* c, tf_stats* st)
{
    if (!st) return;
    const TfDevState* d = c->st_host;
    st->lastFreeBlockId = d->lastFreeBlockId;
    st->lastFreeExcessListId = d->lastFreeExcessListId;
    st->noVisibleEntries = d->noVisibleEntries;
    st->noTotalBlocks = d->noTotalBlocks;
    st->frame_counter = c->frame_counter;   // mirrors of the device counters (last sync)
    st->icp_iterations = d->icp_iters;
    st->icp_ok = d->icp_ok;
    st->n_resets = c->n_resets;
}

#pragma GCC visibility pop
