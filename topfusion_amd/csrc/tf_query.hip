// tf_query.hip -- scene queries (DESIGN.md §5 Scene queries): the TSDF at any point and on any plane, both readings.
// Host layer only: the argument rules of tf_scene_query / tf_scene_slice (include/tfusion_hip.h) and the calls'
// place on the context stream.  The kernels stand in tf_render.hip beside the reads they are made of
// (k_scene_query, tfk_scene_query).
//
// Neither call writes anything of the context's: no TF_BUF_* buffer, no counter, no visType, no device state
// field, no tile order.  Both flush a pending per-call frame first, run on the context stream after the caller's
// work on the default stream, and return when done, as the view calls do.
#include "tf_host.h"

static bool query_args_ok(const tf_ctx* c, int units, int reading, const tf_query_out* out)
{
    if (!c || !out) return false;
    if (units != TF_QUERY_VOXELS && units != TF_QUERY_METRES) return false;
    if (reading != TF_VIEW_RESIDENT && reading != TF_VIEW_WHOLE) return false;
    if (!out->sdf_nearest && !out->entry && !out->sdf && !out->confidence && !out->normal && !out->colour) return false;
    // the colour plane exists on voxel_rgb contexts alone, and the whole reading has none (tf_create refuses colour
    // with swapping)
    if (out->colour && (!c->p.voxel_rgb || reading == TF_VIEW_WHOLE)) return false;
    return true;
}

static tf_status query_run(tf_ctx* c, const float* pts, const TfQuerySlice* slice, long long n, int units, int reading,
                           const tf_query_out* out)
{
    TF_CHECK(order_after_caller(c));
    const float scale = units == TF_QUERY_METRES ? 1.0f / c->p.voxelSize : 1.0f;     // the raycast's oneOverVoxelSize
    TF_CHECK(tfk_scene_query(c, pts, slice, n, scale, reading == TF_VIEW_WHOLE, *out));
    return sync_checked(c);
}

extern "C" tf_status tf_scene_query(tf_ctx* c, const float* dev_points, long long n, int units, int reading,
                                    const tf_query_out* out)
{
    TF_FLUSH(c);
    if (!query_args_ok(c, units, reading, out) || n < 0 || (n > 0 && !dev_points)) return TF_INVALID_ARG;
    if (n > 0x7fffffffLL * 256) return TF_INVALID_ARG;      // one workgroup per 256 points
    return query_run(c, dev_points, nullptr, n, units, reading, out);
}

extern "C" tf_status tf_scene_slice(tf_ctx* c, const float origin[3], const float u[3], const float v[3], int cols, int rows,
                                    int units, int reading, const tf_query_out* out)
{
    TF_FLUSH(c);
    if (!query_args_ok(c, units, reading, out) || !origin || !u || !v || cols <= 0 || rows <= 0) return TF_INVALID_ARG;
    TfQuerySlice s;
    for (int k = 0; k < 3; ++k) { s.o[k] = origin[k]; s.u[k] = u[k]; s.v[k] = v[k]; }
    s.cols = cols;
    return query_run(c, nullptr, &s, (long long)cols * rows, units, reading, out);
}
