// tf_frame.hip -- TopFu::operator(): the frame plan and its enqueue, stage profiling (tf_profile_*), the
// verdict wait of per-call frames, the fallback of a persistent ICP that lost a peer, and the batch.
//
// TopFu::operator() (tfusion/src/topfu.cpp:161-330) becomes a fixed sequence of kernels on
// the context's stream with ONE host synchronisation at the end of the frame (the
// reference has ~27).  ICP, pose algebra and every counter live on the device
// (TfDevState); the host only reads the frame's bool + counters back.
#include "tf_host.h"

// A deferred per-call frame's last two launches (TfFramePlan::defer_tail): CreateICPMaps' raycast
// + renderImage (+ CreateExpectedDepths' fill), then CreateICPMaps + the frame end.  nxt: the next
// frame, whose bilateral pass joins the first grid and whose dists / pyramid / normals pass the
// second (the batch's lookahead, enqueue_frame); none when flushed for another entry point.
tf_status flush_tail(tf_ctx* c, TfAhead nxt, size_t pitch)
{
    if (!c->tail_pending) return TF_OK;
    c->tail_pending = 0;
    TF_CHECK(tfk_raycast_pair(c, TfAhead{}, nxt, pitch, c->tail_fuse_ed, 1));
    TF_CHECK(tfk_icp_maps_end(c, 0, nxt, pitch));
    return TF_OK;
}

// ---- per-stage event timing -----------------------------------------------------------
// Events ring: TF_PROF_RING frames x (start, end) per stage.  Frames are attributed after a
// sync, once their mode / ok flags are known, and only for the stages that did work.
// A single-kernel stage (stage_single) is timed by its dispatch's own timestamps (tf_launch,
// hipExtLaunchKernelGGL); the others by event records around their launches.
#define STAGE_ON(strm, id, expr)                                                              \
    do {                                                                                      \
        const bool timed_ = c->prof_slot_on[slot] && ((c->prof_mask >> (id)) & 1u);          \
        const bool ext_ = timed_ && stage_single(c, id);                                      \
        if (timed_) c->prof_slot_stages[slot] |= 1u << (id);                                  \
        if (ext_) { c->ev_start = prof_event(c, slot, 2 * (id)); c->ev_stop = prof_event(c, slot, 2 * (id) + 1); } \
        else if (timed_) TF_CHECK(hipEventRecord(prof_event(c, slot, 2 * (id)), (strm)));     \
        const hipError_t se_ = (expr);                                                        \
        /* the launcher consumes the events in tf_launch; on every other exit they are dropped */ \
        const bool unused_ = ext_ && c->ev_start;                                             \
        c->ev_start = c->ev_stop = nullptr;                                                   \
        TF_CHECK(se_);                                                                        \
        if (unused_) return TF_HIP_ERROR;                                                     \
        if (timed_ && !ext_) TF_CHECK(hipEventRecord(prof_event(c, slot, 2 * (id) + 1), (strm))); \
    } while (0)
#define STAGE(id, expr) STAGE_ON(c->stream, id, expr)

// stages whose frame-path launcher issues exactly one kernel (through tf_launch)
static bool stage_single(const tf_ctx* c, int id)
{
    return (id == TF_STAGE_ICP && c->icp_persistent) || id == TF_STAGE_INTEGRATE || id == TF_STAGE_EXPECTED_DEPTHS ||
           id == TF_STAGE_RAYCAST_ICP || id == TF_STAGE_ICP_MAPS;
}

static hipEvent_t prof_event(tf_ctx* c, int slot, int k)
{
    return c->prof_ev[(slot % TF_PROF_RING) * 2 * TF_NUM_STAGES + k];
}

static bool stage_ran(int stage, int mode, int ok)
{
    if (stage == TF_STAGE_PREPROCESS) return true;
    // ICP: only frames whose estimateTransform ran all its iterations (a failed det check ends
    // it early, and its launch would understate the per-launch time of the full 19 iterations)
    if (stage == TF_STAGE_ICP) return mode == 1 && ok == 1;
    if (stage == TF_STAGE_ALLOC || stage == TF_STAGE_INTEGRATE) return mode == 0 || ok == 1;
    if (stage == TF_STAGE_GREY) return false;                      // fused into RAYCAST_RENDER
    return mode == 1 && ok == 1;
}

// attribute the timed stages of batch slots [first, first+n) (their events must be complete)
static tf_status prof_collect(tf_ctx* c, int first, int n, const int* ok, const int* mode)
{
    if (!c->prof_enabled) return TF_OK;
    for (int f = 0; f < n; ++f)
        for (int i = 0; i < TF_NUM_STAGES; ++i) {
            if (!c->prof_slot_on[first + f] || !((c->prof_mask >> i) & 1u) || !stage_ran(i, mode[f], ok[f])) continue;
            if (!((c->prof_slot_stages[first + f] >> i) & 1u)) continue;      // not enqueued as its own stage
            if (i == TF_STAGE_PREPROCESS && !c->prof_slot_pre[first + f]) continue;   // done by the previous frame
            if (i == TF_STAGE_RAYCAST_RENDER) continue;                       // fused into RAYCAST_ICP
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, prof_event(c, first + f, 2 * i), prof_event(c, first + f, 2 * i + 1)) == hipSuccess) {
                c->prof_ms[i] += ms;
                c->prof_count[i] += 1;
            }
        }
    return TF_OK;
}

// enqueue one TopFu::operator() frame into batch slot `slot` (no host synchronisation).
// The frame's branches (frame 0 / tracking / ICP failure -> reset, topfu.cpp:161-330) are
// decided on the device: the ICP launch starts the frame (tf_frame_begin sets st->mode), every
// later kernel checks st->mode / st->abort, and the frame end in k_icp_maps_end's tail (frame
// counters, per-slot ok flag, ResetScene on ICP failure) closes it.  A batch is therefore
// enqueued back to back.  Per frame: k_icp_frame (+ setToType3 and the renderImage snapshot in
// its tail) -> k_alloc_requests -> k_alloc_apply -> k_vis_count -> k_vis_apply -> k_integrate
// (+ CreateExpectedDepths' projection) -> k_ed_fill -> k_raycast_pair (CreateICPMaps' castRay
// and renderImage's castRay + grey in one grid) -> k_icp_maps_end.
//
// Lookahead (batches): later frames' preprocessing runs in this frame's grid tails and their
// enqueues skip it.  k_raycast_pair of frame j runs frame j+1's computeDists + pyramids +
// normals and frame j+2's bilateral pass, whose level-0 depth goes to the buffer of j's parity
// (d0_buf, ping-pong); the batch's first frame also runs frame 1's bilateral pass in
// k_alloc_requests.  Preprocessing is a pure function of the raw frame; what it writes is past
// its last reader of this frame by then (level-0 depth: this frame's pyramid pass; dists and
// the current maps: this frame's allocation, integration and ICP).
struct TfFramePlan {
    int pre_done;            // this frame's preprocessing ran in earlier launches
    uint16_t* d0;            // this frame's level-0 depth buffer
    TfAhead alloc_bil, pair_pyr, pair_bil;
    int defer_tail;          // leave k_raycast_pair + k_icp_maps_end to the next call (flush_tail)
};

#ifdef TF_DIAG_NOP_AFTER_ICP
__global__ void k_diag_nop() {}
#endif

static tf_status enqueue_frame(tf_ctx* c, const uint16_t* depth, size_t pitch, int slot,
                               const TfFramePlan* plan = nullptr)
{
    static const TfFramePlan none = { 0, nullptr, {}, {}, {}, 0 };
    if (!plan) plan = &none;
    uint16_t* d0 = plan->d0 ? plan->d0 : c->d0_buf[0];
    c->prof_slot_on[slot] = c->prof_enabled && (c->prof_seq++ % c->prof_period) == 0;
    c->prof_slot_pre[slot] = !plan->pre_done;
    c->prof_slot_stages[slot] = 0;
    // preprocessing (topfu.cpp:166-197)
    if (!plan->pre_done) STAGE(TF_STAGE_PREPROCESS, tfk_preprocess(c, depth, pitch, c->stream, d0));
    c->depth_pyr[0] = d0;
    // frame begin + estimateTransform + poses_.push_back (topfu.cpp:200, 242-243); with the
    // persistent ICP, setToType3 / the renderImage snapshot run in its tail
    const bool t3_fold = c->icp_persistent != 0;
    STAGE(TF_STAGE_ICP, tfk_icp(c, 1, 1, t3_fold));
#ifdef TF_DIAG_NOP_AFTER_ICP
    // diagnostic builds only: an empty launch between the ICP and the allocation, to tell in a
    // kernel trace which side of that boundary its dispatch gap belongs to
    hipLaunchKernelGGL(k_diag_nop, dim3(1), dim3(64), 0, c->stream);
#endif
    STAGE(TF_STAGE_ALLOC, tfk_alloc(c, t3_fold ? 2 : 1, plan->alloc_bil, pitch));   // topfu.cpp:202 / 281
    // (+ CreateExpectedDepths' projection pass in the same grid)
    STAGE(TF_STAGE_INTEGRATE, tfk_integrate(c, 1, 1));              // topfu.cpp:203 / 282 (+ frame-0 prev_ = curr_)
    if (c->p.use_swapping) TF_CHECK(tfk_swap(c));                   // swap in / out after integration
    // CreateExpectedDepths (topfu.cpp:306): its projection ran in k_integrate's grid; its fill runs
    // in k_raycast_pair's grid when the frame is narrow enough (tfk_ed_fused), else on its own
    const int fuse_ed = tfk_ed_fused(c);
    if (!fuse_ed) STAGE(TF_STAGE_EXPECTED_DEPTHS, tfk_expected_depths(c, 1));
    if (plan->defer_tail) {                   // per-call frame: the last two launches wait for the next call
        c->tail_pending = 1;
        c->tail_fuse_ed = fuse_ed;
        return TF_OK;
    }
    // CreateICPMaps' raycast + renderImage (topfu.cpp:284-285 + 307) in one launch (snapshot range)
    STAGE(TF_STAGE_RAYCAST_ICP, tfk_raycast_pair(c, plan->pair_pyr, plan->pair_bil, pitch, fuse_ed, 1));
    // renderICP + resizePointsNormals (topfu.cpp:308-309) + the frame end (topfu.cpp:263-264)
    STAGE(TF_STAGE_ICP_MAPS, tfk_icp_maps_end(c, slot));
    return TF_OK;
}


// sync, read back slots [first, first+n) and the state; ok_out gets 1/0 per frame.  *lost: the
// slot whose persistent ICP lost a peer (frame_ok -1: nothing of it ran past the ICP, and the
// later slots were skipped, -2), for the caller to re-run from there; -1 if none.  A frame that
// failed past its ICP (-3) is TF_HIP_ERROR.
static tf_status finish_frames(tf_ctx* c, int first, int n, int* ok_out, int* lost = nullptr)
{
    if (lost) *lost = -1;
    // one device-to-host copy into the pinned mirror: the state and the slots' ok / mode
    TF_CHECK(hipMemcpyAsync(c->st_host, c->st, TF_ST_BYTES, hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipStreamSynchronize(c->stream));
    const int* okb = (const int*)(c->st_host + 1) + first;
    const int* modeb = (const int*)(c->st_host + 1) + TF_PROF_RING + first;
    c->frame_counter = c->st_host->frame_counter;
    c->n_resets = c->st_host->n_resets;
    prof_collect(c, first, n, okb, modeb);
    if (c->st_host->sticky_error) return TF_HIP_ERROR;
    tf_status r = TF_OK;
    for (int i = 0; i < n; ++i) {
        if (okb[i] == -1 && lost) { *lost = i; break; }
        if (okb[i] < 0) return TF_HIP_ERROR;
        if (ok_out) ok_out[i] = okb[i];
        if (okb[i] == 0) r = TF_ICP_FAIL;
    }
    return r;
}

// Run-time fallback of the persistent ICP: a frame whose persistent launch lost a peer (some of
// its 256 workgroups could not be co-resident -- another process or kernel on the device; the
// bounded spins ended it: frame_ok -1, the frame end halted the batch) is enqueued again, whole,
// on the per-iteration schedule (k_icp_iter: one launch per iteration, no co-residency needed).
// Nothing of the failed attempt changed the scene (every stage after the ICP no-oped on abort),
// so the re-run is the frame as it would have run.  Synchronous; *ok = its frame_ok.
static tf_status rerun_frame_fallback(tf_ctx* c, const uint16_t* depth, size_t pitch, int* ok)
{
    TF_CHECK(hipMemsetAsync((char*)c->st + offsetof(TfDevState, halt), 0, sizeof(int), c->stream));
    const int saved = c->icp_persistent;
    c->icp_persistent = 0;
    c->icp_fallbacks++;
    tf_status s = enqueue_frame(c, depth, pitch, 0);
    c->icp_persistent = saved;
    if (s != TF_OK) return s;
    int okv = 0;
    s = finish_frames(c, 0, 1, &okv);
    if (s != TF_OK && s != TF_ICP_FAIL) return s;
    if (ok) *ok = okv;
    return s;
}

extern "C" tf_status tf_profile_enable(tf_ctx* c, int enable)
{
    if (!c) return TF_INVALID_ARG;
    if (enable && !c->prof_ev[0]) {
        // timing only (read after the stream is synchronised): no system-scope fence at the record,
        // whose cache writeback and invalidate were a dispatch gap after every timed stage
        for (int i = 0; i < 2 * TF_NUM_STAGES * TF_PROF_RING; ++i)
            TF_CHECK(hipEventCreateWithFlags(&c->prof_ev[i], hipEventDisableSystemFence));
    }
    c->prof_enabled = enable ? 1 : 0;
    c->count_lanes = enable ? 1 : 0;
    c->prof_mask = (1u << TF_NUM_STAGES) - 1;
    c->prof_period = 1;
    c->prof_seq = 0;
    return TF_OK;
}

extern "C" tf_status tf_profile_stages(tf_ctx* c, unsigned mask)
{
    if (!c) return TF_INVALID_ARG;
    tf_status s = tf_profile_enable(c, mask != 0);
    if (s != TF_OK) return s;
    c->prof_mask = mask;
    c->count_lanes = 0;          // (selected stages: a timed run, no counting atomics in it)
    return TF_OK;
}

extern "C" tf_status tf_profile_sample(tf_ctx* c, int period)
{
    if (!c || period < 1) return TF_INVALID_ARG;
    c->prof_period = period;
    c->prof_seq = 0;
    return TF_OK;
}

extern "C" tf_status tf_profile_reset(tf_ctx* c)
{
    if (!c) return TF_INVALID_ARG;
    for (int i = 0; i < TF_NUM_STAGES; ++i) { c->prof_ms[i] = 0; c->prof_count[i] = 0; }
    return TF_OK;
}

extern "C" tf_status tf_profile_read(tf_ctx* c, double* ms, long long* counts, int n)
{
    if (!c || n < 0 || n > TF_NUM_STAGES) return TF_INVALID_ARG;
    for (int i = 0; i < n; ++i) {
        if (ms) ms[i] = c->prof_ms[i];
        if (counts) counts[i] = c->prof_count[i];
    }
    return TF_OK;
}

// A per-call frame returns on its verdict (early) when nothing the caller asked for needs the
// whole frame: no stats, no stage timing, no RGB image (k_integrate reads the caller's image
// directly, so the call must not return before the integration has run), and the persistent
// ICP (the per-iteration fallback writes no verdict).
static bool percall_early(const tf_ctx* c, const tf_stats* stats)
{
    return c->percall_early && c->icp_persistent && !c->prof_enabled && !stats && !c->rgb_cur;
}

// TopFu::operator() returning on its verdict.  Enqueues the whole frame, then waits only until
// the persistent ICP launch has written the frame's verdict (topfu.cpp:209 / 263-264 / 329:
// frame-0 path, reset + false, true; and poses_.back()) into host memory.  The allocation,
// integration, raycasts and frame end are still running on the context stream when it returns;
// everything that reads their results later (tf_download, tf_render_image, tf_get_*) is ordered
// after them on that stream, and the next frame's launches queue behind them, so the device does
// not wait for the host between frames.  The frame's preprocessing has read the depth by then.
// host_depth: the tf_process_frame_host form.
static tf_status process_frame_early(tf_ctx* c, const uint16_t* depth, size_t pitch, const uint16_t* host_depth,
                                     float pose_out[12])
{
    if (host_depth) {
        TF_CHECK(upload_depth(c, host_depth, pitch));
        depth = c->depth_in;
        pitch = (size_t)c->W * 2;
    }
    // the previous frame's deferred launches carry this frame's preprocessing in their grid tails
    TfFramePlan plan = { 0, nullptr, {}, {}, {}, c->percall_defer };
    if (c->tail_pending) {
        const TfAhead nxt = { depth, c->d0_buf[0] };
        tf_status fs = flush_tail(c, nxt, pitch);
        if (fs != TF_OK) return fs;
        plan.pre_done = 1;
        plan.d0 = c->d0_buf[0];
    }
    if (++c->verdict_gen == 0) c->verdict_gen = 1;
    const unsigned gen = c->verdict_gen;
    c->verdict_arm = 1;
    tf_status s = enqueue_frame(c, depth, pitch, 0, &plan);
    c->verdict_arm = 0;
    if (s != TF_OK) return s;
    // wait for the verdict: every word tagged with this generation
    volatile unsigned long long* v = c->verdict_host;
    unsigned long long w[13];
    bool drained = false;
    for (unsigned spins = 0;; ++spins) {
        int k = 0;
        for (; k < 13; ++k) {
            w[k] = v[k];
            if ((unsigned)(w[k] >> 32) != gen) break;
        }
        if (k == 13) break;
        if (drained) return TF_HIP_ERROR;        // the stream finished without writing it
        if ((spins & 1023u) == 1023u) {
            const hipError_t q = hipStreamQuery(c->stream);
            if (q == hipSuccess) drained = true;   // read the record once more, then give up
            else if (q != hipErrorNotReady) return tf_from_hip(q);
        }
        __builtin_ia32_pause();
    }
    const int mode = (int)(w[0] & 15u), ok = (int)((w[0] >> 4) & 15u) - 1;
    if (ok < 0) {
        // the frame's launches end on the device (the halted / failed frame no-ops); its deferred
        // tail holds the frame end, enqueued now without a lookahead
        const tf_status fs = flush_tail(c);
        if (fs != TF_OK) return fs;
        TF_CHECK(hipStreamSynchronize(c->stream));
        if ((w[0] >> 16) & 1u) return TF_HIP_ERROR;           // halted: an earlier frame failed past its ICP
        // a lost peer in the persistent ICP: the frame again, on the per-iteration schedule
        int okv = 0;
        const tf_status s2 = rerun_frame_fallback(c, depth, pitch, &okv);
        if (s2 != TF_OK && s2 != TF_ICP_FAIL) return s2;
        if (pose_out) memcpy(pose_out, c->st_host->pose, sizeof(float) * 12);
        return s2;
    }
    // host mirrors of the counters the frame end writes (tf_reset.h)
    if (mode == 0) c->frame_counter = 1;
    else if (ok) c->frame_counter++;
    else { c->frame_counter = 0; c->n_resets++; }
    if (pose_out)
        for (int i = 0; i < 12; ++i) {
            const unsigned bits = (unsigned)w[1 + i];
            memcpy(&pose_out[i], &bits, sizeof(float));
        }
    return ok ? TF_OK : TF_ICP_FAIL;
}

extern "C" tf_status tf_process_frame(tf_ctx* c, const uint16_t* dev_depth, size_t pitch, float pose_out[12],
                                      tf_stats* stats)
{
    if (!c || !dev_depth) return TF_INVALID_ARG;
    if (pitch == 0) pitch = (size_t)c->W * 2;
    if (percall_early(c, stats)) return process_frame_early(c, dev_depth, pitch, nullptr, pose_out);
    TF_FLUSH(c);
    tf_status s = enqueue_frame(c, dev_depth, pitch, 0);
    if (s != TF_OK) return s;
    int lost = -1;
    s = finish_frames(c, 0, 1, nullptr, &lost);
    if (lost == 0) s = rerun_frame_fallback(c, dev_depth, pitch, nullptr);   // the persistent ICP lost a peer
    if (s != TF_OK && s != TF_ICP_FAIL) return s;
    if (pose_out) memcpy(pose_out, c->st_host->pose, sizeof(float) * 12);
    fill_stats(c, stats);
    return s;
}

extern "C" tf_status tf_process_frame_rgb(tf_ctx* c, const uint16_t* dev_depth, size_t pitch, const uint8_t* dev_rgb,
                                          size_t rgb_pitch, float pose_out[12], tf_stats* stats)
{
    TF_FLUSH(c);
    if (!c) return TF_INVALID_ARG;
    if (dev_rgb && !c->p.voxel_rgb) return TF_INVALID_ARG;
    RgbScope rs(c, dev_rgb, rgb_pitch);
    return tf_process_frame(c, dev_depth, pitch, pose_out, stats);
}

extern "C" tf_status tf_process_frame_rgb_host(tf_ctx* c, const uint16_t* host_depth, size_t pitch, const uint8_t* host_rgb,
                                               size_t rgb_pitch, float pose_out[12], tf_stats* stats)
{
    TF_FLUSH(c);
    if (!c || !host_depth) return TF_INVALID_ARG;
    if (host_rgb && !c->p.voxel_rgb) return TF_INVALID_ARG;
    if (!host_rgb) return tf_process_frame_host(c, host_depth, pitch, pose_out, stats);
    if (rgb_pitch == 0) rgb_pitch = (size_t)c->W * 4;
    TF_CHECK(upload_rgb(c, host_rgb, rgb_pitch));
    if (pitch == 0) pitch = (size_t)c->W * 2;
    TF_CHECK(upload_depth(c, host_depth, pitch));
    return tf_process_frame_rgb(c, c->depth_in, (size_t)c->W * 2, (const uint8_t*)c->rgb_in, (size_t)c->W * 4, pose_out,
                                stats);
}

extern "C" tf_status tf_process_frame_host(tf_ctx* c, const uint16_t* host_depth, size_t pitch, float pose_out[12],
                                           tf_stats* stats)
{
    if (!c || !host_depth) return TF_INVALID_ARG;
    if (pitch == 0) pitch = (size_t)c->W * 2;
    if (percall_early(c, stats)) return process_frame_early(c, nullptr, pitch, host_depth, pose_out);
    TF_FLUSH(c);
    TF_CHECK(upload_depth(c, host_depth, pitch));
    return tf_process_frame(c, c->depth_in, (size_t)c->W * 2, pose_out, stats);
}

// a batch of device-resident frames: enqueued TF_PROF_RING at a time with no host round trip
// inside a group (the frame's branches are decided on the device)
static tf_status process_frames(tf_ctx* c, const uint16_t* dev_frames, size_t stride, const uint8_t* rgb_frames,
                                size_t rgb_stride, int n, int* ok_out);

extern "C" tf_status tf_process_frames(tf_ctx* c, const uint16_t* dev_frames, size_t stride, int n, int* ok_out)
{
    TF_FLUSH(c);
    return process_frames(c, dev_frames, stride, nullptr, 0, n, ok_out);
}

extern "C" tf_status tf_process_frames_rgb(tf_ctx* c, const uint16_t* dev_frames, size_t stride, const uint8_t* rgb_frames,
                                          size_t rgb_stride, int n, int* ok_out)
{
    TF_FLUSH(c);
    if (c && rgb_frames && !c->p.voxel_rgb) return TF_INVALID_ARG;
    return process_frames(c, dev_frames, stride, rgb_frames, rgb_stride, n, ok_out);
}

static tf_status process_frames(tf_ctx* c, const uint16_t* dev_frames, size_t stride, const uint8_t* rgb_frames,
                                size_t rgb_stride, int n, int* ok_out)
{
    if (!c || !dev_frames || n < 0) return TF_INVALID_ARG;
    if (rgb_frames && rgb_stride == 0) rgb_stride = (size_t)c->W * c->H * 4;
    auto frame = [&](int j) { return (const uint16_t*)((const char*)dev_frames + (size_t)j * stride); };
    int s0 = 0;                 // the frame the lookahead chain starts at (0, or after a fallback re-run)
    for (int first = 0; first < n;) {
        const int m = n - first < TF_PROF_RING ? n - first : TF_PROF_RING;
        for (int i = 0; i < m; ++i) {
            const int j = first + i;
            // two-frame lookahead (enqueue_frame): frame j+1's pyramid pass and frame j+2's
            // bilateral pass run in frame j's grid tails
            TfFramePlan p = { j > s0, c->d0_buf[j & 1], {}, {}, {}, 0 };
            if (j + 1 < n) {
                TfAhead next = { frame(j + 1), c->d0_buf[(j + 1) & 1] };
                p.pair_pyr = next;
                if (j == s0) p.alloc_bil = next;
                if (j + 2 < n) p.pair_bil = TfAhead{ frame(j + 2), c->d0_buf[j & 1] };
            }
            RgbScope rs(c, rgb_frames ? rgb_frames + (size_t)j * rgb_stride : nullptr, (size_t)c->W * 4);
            tf_status s = enqueue_frame(c, frame(j), (size_t)c->W * 2, i, &p);
            if (s != TF_OK) return s;
        }
        int lost = -1;
        tf_status s = finish_frames(c, 0, m, ok_out ? ok_out + first : nullptr, &lost);
        if (s != TF_OK && s != TF_ICP_FAIL) return s;
        if (lost < 0) { first += m; continue; }
        // frame first+lost lost an ICP peer, the rest of the group was skipped: re-run it on the
        // per-iteration schedule (its own preprocessing: its maps were overwritten by the lookahead
        // of the skipped frames), then continue the batch after it with a fresh lookahead chain
        const int j = first + lost;
        RgbScope rs(c, rgb_frames ? rgb_frames + (size_t)j * rgb_stride : nullptr, (size_t)c->W * 4);
        int okv = 0;
        s = rerun_frame_fallback(c, frame(j), (size_t)c->W * 2, &okv);
        if (s != TF_OK && s != TF_ICP_FAIL) return s;
        if (ok_out) ok_out[j] = okv;
        first = s0 = j + 1;
    }
    return TF_OK;
}
