/*
 * tfusion_hip.h -- C-ABI of libtfusion_hip.so, the MI355X (gfx950) implementation
 * of the topfusion hot path: depth preprocessing, projective point-to-plane ICP,
 * voxel-block-hash allocation, TSDF integration and raycasting.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; device pointers
 * are HIP device pointers on the context's device.  Every entry point replaces a
 * reference interface, cited as file:line relative to the 3d-scan/topfusion root.
 * The C++ mirror of the reference API (include/tfusion/topfu.hpp etc.) is a thin layer over
 * these functions; see INTEGRATION.md for the bindings.
 *
 * Error convention: every function returns a tf_status (0 = TF_OK).  The reference
 * prints and exit()s on CUDA errors (tfusion/src/device_memory.cpp:7-11,
 * tfusion/include/tfusion/cuda/CUDADefines.hpp:26-33); here the caller decides.
 * ICP degeneracy is TF_ICP_FAIL and triggers the same reset as the reference
 * (tfusion/src/topfu.cpp:263-264).
 *
 * Device-side failures.  The frame's stages wait on each other inside grids with bounded spins.
 * (1) The persistent ICP launch needs its 256 workgroups resident at once; if another process or
 * kernel holds part of the device, the launch ends with a lost peer.  Nothing past the ICP has
 * run then, and the frame is run again on the per-iteration ICP schedule (tf_totals::icp_fallbacks
 * counts it): the caller sees the frame's normal result.  (2) A bounded spin past the ICP that
 * times out leaves the frame half done: the context is in error from then on -- that frame's
 * call, or the next call that synchronises with the device if the frame's call had already
 * returned (per-call frames return on their ICP verdict), and every later call that
 * synchronises with the device (downloads, uploads, stage / engine / visualisation calls,
 * tf_scene_fuse_frames, stats and pose queries) returns TF_HIP_ERROR until tf_reset.  The same
 * holds for an engine-level call whose visible-list build loses a wait (k_vis_build), which has
 * no frame end to report it.  An engine batch on a context halted by a failed frame no-ops.
 */
#ifndef TFUSION_HIP_H
#define TFUSION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum tf_status {
    TF_OK = 0,
    TF_ICP_FAIL = 1,        /* estimateTransform returned false; scene was reset */
    TF_INVALID_ARG = 2,
    TF_OOM = 3,
    TF_HIP_ERROR = 4,
    TF_NO_DEVICE = 5,
    TF_INDEX_RANGE = 6,     /* tf_mesh_extract_indexed: the mesh has more than 2^32 - 1 vertices, nothing written */
    TF_CAPACITY = 7         /* tf_map_load_resized: the file's live content does not fit the context's tables; context untouched.
                               tf_view_find_visible / tf_view_render: more visible entries than the view's vis_capacity;
                               the view's buffers untouched, the number needed reported */
} tf_status;

/* TopFuParams (tfusion/include/tfusion/topfu.hpp:28-60) restricted to the fields the
 * hot path reads, plus SceneParams (tfusion/include/tfusion/SceneParams.hpp:8-66)
 * and the reference's compile-time capacities made run-time. */
typedef struct tf_params {
    int   cols, rows;
    float fx, fy, cx, cy;               /* Intr */
    float bilateral_sigma_depth;        /* m */
    float bilateral_sigma_spatial;      /* px */
    int   bilateral_kernel_size;        /* px (7) */
    float icp_truncate_depth_dist;      /* m; <= 0 disables */
    float icp_dist_thres;               /* m */
    float icp_angle_thres;              /* rad */
    int   icp_iter_num[4];              /* per level 0..3; none negative, [3] == 0 (three pyramid levels) */
    float mu;                           /* TSDF truncation band (SceneParams::mu) */
    int   maxW;
    float voxelSize;                    /* m */
    float viewFrustum_min, viewFrustum_max;
    int   n_buckets;                    /* SDF_BUCKET_NUM, power of two (VoxelBlockHash.hpp:16) */
    int   n_excess;                     /* SDF_EXCESS_LIST_SIZE (VoxelBlockHash.hpp:18) */
    int   n_blocks;                     /* SDF_LOCAL_BLOCK_NUM (VoxelBlockHash.hpp:14) */
    int   vis_capacity;                 /* visibleEntryIDs capacity (RenderState_VH.hpp:42) */
    int   max_render_blocks;            /* MAX_RENDERING_BLOCKS (VisualisationEngine_Shared.hpp:5) */
    /* swapping: Scene(params, useSwapping) (scene.hpp:29-33) with its GlobalCache
       (GlobalCache.hpp:11-134), kept in HBM; TopFu itself runs without (topfu.cpp:67) */
    int   use_swapping;
    int   swap_transfer_blocks;         /* SDF_TRANSFER_BLOCK_NUM (VoxelBlockHash.hpp:27): blocks per swap */
    /* colour: Voxel_s_rgb voxels (VoxelTypes.hpp:39-67) integrated from the RGB image */
    int   voxel_rgb;                    /* 1: Voxel_s_rgb (colour integrated by the *_rgb entry points) */
    float rgb_intr[4];                  /* projParams_rgb (fx, fy, cx, cy); all 0: the depth intrinsics */
    float depth_to_rgb[12];             /* calib_inv of trafo_rgb_to_depth, row-major [R|t]: M_rgb = it * M_d */
} tf_params;

/* integer counters the reference keeps host-side (LocalVBA.hpp:26, VoxelBlockHash.hpp:69,
 * RenderState_VH.hpp:33, VisualisationEngine_CUDA.cu:160) plus ICP bookkeeping */
typedef struct tf_stats {
    int lastFreeBlockId;
    int lastFreeExcessListId;
    int noVisibleEntries;
    int noTotalBlocks;
    int frame_counter;
    int icp_iterations;                 /* iterations executed by the last estimateTransform */
    int icp_ok;
    int n_resets;
} tf_stats;

typedef struct tf_ctx tf_ctx;

/* buffer ids for tf_download / tf_upload (state inspection for parity tests) */
typedef enum tf_buffer {
    TF_BUF_HASH = 0,          /* HashEntry[n_buckets+n_excess], 16 B each (VoxelBlockHash.hpp:32-44) */
    TF_BUF_VBA = 1,           /* Voxel_s[n_blocks*512], 4 B each (VoxelTypes.hpp:69-92) */
    TF_BUF_VISIBLE_IDS = 2,   /* int[vis_capacity] */
    TF_BUF_VISIBLE_TYPE = 3,  /* uchar[n_buckets+n_excess] */
    TF_BUF_RANGE = 4,         /* float2[rows*cols]  renderingRangeImage */
    TF_BUF_RAYCAST = 5,       /* float4[rows*cols]  raycastResult */
    TF_BUF_DISTS = 6,         /* float[rows*cols] */
    TF_BUF_DEPTH = 7,         /* ushort[level]  filtered depth pyramid */
    TF_BUF_CURR_POINTS = 8,   /* float4[level] */
    TF_BUF_CURR_NORMALS = 9,
    TF_BUF_PREV_POINTS = 10,
    TF_BUF_PREV_NORMALS = 11,
    TF_BUF_GREY = 12,         /* uchar4[rows*cols] last renderImage output */
    TF_BUF_SWAP_STATE = 13,   /* uchar[n_buckets+n_excess] HashSwapState::state (GlobalCache.hpp:11-20) */
    TF_BUF_SWAP_STORED_FLAGS = 14,  /* uchar[n_buckets+n_excess] GlobalCache hasStoredData */
    TF_BUF_SWAP_STORED = 15,  /* Voxel_s[(n_buckets+n_excess)*512] GlobalCache storedVoxelBlocks */
    TF_BUF_VBA_RGB = 16,      /* voxel_rgb: uint32[n_blocks*512] Voxel_s_rgb clr + w_color (VoxelTypes.hpp:39-67),
                                 r | g << 8 | b << 16 | w_color << 24 -- the colour half of each voxel */
    TF_BUF_ALLOC_LIST = 17,   /* int[n_blocks] LocalVBA::allocationList, the free-block stack (LocalVBA.hpp:19, 35) */
    TF_BUF_EXCESS_LIST = 18   /* int[n_excess] VoxelBlockHash::excessAllocationList (VoxelBlockHash.hpp:81, 88) */
} tf_buffer;

/* ---- device ---------------------------------------------------------------- */
/* cuda::getCudaEnabledDeviceCount / setDevice (tfusion/include/tfusion/topfu.hpp:20-21) */
tf_status tf_device_count(int* count);
tf_status tf_set_device(int device);
const char* tf_status_string(tf_status s);

/* ---- context (TopFu) -------------------------------------------------------- */
/* TopFuParams::default_params (tfusion/src/topfu.cpp:12-53) */
tf_status tf_default_params(tf_params* p);
/* TopFu::TopFu (tfusion/src/topfu.cpp:55-84): allocates the scene, render state and
 * ICP buffers on the current device and creates one HIP stream. */
tf_status tf_create(const tf_params* p, tf_ctx** out);
void      tf_destroy(tf_ctx* ctx);
/* TopFu::reset (tfusion/src/topfu.cpp:141-152) */
tf_status tf_reset(tf_ctx* ctx);
/* TopFu::operator()(const cuda::Depth&) (tfusion/src/topfu.cpp:161-330).
 * dev_depth: uint16 millimetres, rows x cols, row pitch in bytes.
 * Returns TF_OK (true) or TF_ICP_FAIL (false, scene reset).  pose_out (optional):
 * getCameraPose() as a row-major 3x4 [R|t].  Returns as soon as the frame's result is known
 * (after its ICP), with its allocation, integration and raycasts still running on the context
 * stream -- the reference likewise returns with its last kernels in flight (topfu.cpp:307-329);
 * every later call that reads the state is ordered after them.  dev_depth has been consumed by
 * then.  stats (optional) waits for the whole frame; so do RGB frames and profiled contexts.
 * Deferred tail: the frame's last two launches (CreateICPMaps' raycast + renderImage, and
 * CreateICPMaps + the frame end) are not enqueued by this call but by the next tf_* call on the
 * context (the next frame's call carries that frame's preprocessing in them).  A caller that
 * synchronises the device or a stream itself must first call tf_get_stream(), which enqueues
 * them; every other entry point does it before its own work. */
tf_status tf_process_frame(tf_ctx* ctx, const uint16_t* dev_depth, size_t pitch_bytes,
                           float pose_out[12], tf_stats* stats);
/* same, host depth (cuda::Depth::upload, device_array.hpp; demo.cpp:100) */
tf_status tf_process_frame_host(tf_ctx* ctx, const uint16_t* host_depth, size_t pitch_bytes,
                                float pose_out[12], tf_stats* stats);
/* Runs n frames (frame i at dev_frames + i*frame_stride_bytes, pitch cols*2) with the
 * exact per-frame semantics of tf_process_frame, but without a host round trip per
 * frame.  ok_out (optional, n ints) receives each frame's bool. */
tf_status tf_process_frames(tf_ctx* ctx, const uint16_t* dev_frames, size_t frame_stride_bytes, int n,
                            int* ok_out);
/* TopFu::operator()(depth, image) (topfu.hpp:80) with the image integrated: with voxel_rgb set,
 * each frame's uchar4 RGB image (rows x cols, pitch bytes; registered to the depth through
 * rgb_intr / depth_to_rgb) updates the Voxel_s_rgb colour of the voxels near the surface
 * (computeUpdatedVoxelColorInfo, SceneReconstructionEngine.hpp:116-148, where the lineage's
 * ComputeUpdatedVoxelInfo<true, ...> calls it, :163-176).  dev_rgb null: as the depth-only call. */
tf_status tf_process_frame_rgb(tf_ctx* ctx, const uint16_t* dev_depth, size_t pitch_bytes, const uint8_t* dev_rgb,
                               size_t rgb_pitch_bytes, float pose_out[12], tf_stats* stats);
/* same, host depth and host RGB (uploaded through the context's staging buffers) */
tf_status tf_process_frame_rgb_host(tf_ctx* ctx, const uint16_t* host_depth, size_t pitch_bytes, const uint8_t* host_rgb,
                                    size_t rgb_pitch_bytes, float pose_out[12], tf_stats* stats);
/* the batch form: frame i's RGB image at dev_rgb_frames + i*rgb_stride_bytes (pitch cols*4) */
tf_status tf_process_frames_rgb(tf_ctx* ctx, const uint16_t* dev_frames, size_t frame_stride_bytes,
                                const uint8_t* dev_rgb_frames, size_t rgb_stride_bytes, int n, int* ok_out);
/* TopFu::renderImage (tfusion/src/topfu.cpp:332-377): raycast + grey shading of the
 * current pose into dev_rgba (uchar4, rows x cols, pitch bytes). */
tf_status tf_render_image(tf_ctx* ctx, uint8_t* dev_rgba, size_t pitch_bytes);
/* IVisualisationEngine::RenderImageType (tfusion/include/tfusion/VisualisationEngine.hpp:15-22) */
typedef enum tf_render_type {
    TF_RENDER_SHADED_GREYSCALE = 0,              /* renderGrey_device (SDF-gradient normals) */
    TF_RENDER_SHADED_GREYSCALE_IMAGENORMALS = 1, /* renderGrey_ImageNormals_device<false> (raycast-image normals) */
    TF_RENDER_COLOUR_FROM_VOLUME = 2,            /* renderColour_device with voxel_rgb; Voxel_s has no colour: greyscale
                                                    (VisualisationEngine_CUDA.cu:251-256) */
    TF_RENDER_COLOUR_FROM_NORMAL = 3,            /* renderColourFromNormal_device (alpha left as it was) */
    TF_RENDER_COLOUR_FROM_CONFIDENCE = 4         /* renderColourFromConfidence_device */
} tf_render_type;
/* VisualisationEngine_CUDA::RenderImage(scene, pose, intr, renderState, image, type,
 * RENDER_FROM_NEW_RAYCAST) (VisualisationEngine_CUDA.cu:220-291, 423-429) from poses_.back():
 * raycast with the current range image, then the type's pixel stage into the context's
 * image buffer (TF_BUF_GREY) and, when dev_rgba is non-null, a copy there. */
tf_status tf_render_image_type(tf_ctx* ctx, int type, uint8_t* dev_rgba, size_t pitch_bytes);
/* TopFu::getCameraPose (tfusion/src/topfu.cpp:154-159), time = -1 only */
tf_status tf_get_pose(tf_ctx* ctx, float rt[12]);
tf_status tf_get_stats(tf_ctx* ctx, tf_stats* stats);
tf_status tf_get_params(tf_ctx* ctx, tf_params* p);
/* HIP stream owned by the context (hipStream_t), for interop */
void*     tf_get_stream(tf_ctx* ctx);
/* execution schedule chosen at tf_create (no reference counterpart): 1 when ICP runs as one
 * persistent launch per frame (k_icp_frame), 0 for one launch per iteration; the environment
 * variable TFUSION_ICP_PERSISTENT=0 forces the latter */
tf_status tf_get_schedule(tf_ctx* ctx, int* icp_persistent);
/* The ICP iterations' pose algebra: estimateTransform's cv::determinant(A), cv::solve(A, b, r,
 * cv::DECOMP_SVD) and Affine3f Tinc(r) (tfusion/src/projective_icp.cpp:197-209).
 *   TF_POSE_ALGEBRA_CANONICAL: the pivoting LU determinant, a 2 x 2 block Schur solve in double
 *     (closed-form 3 x 3 adjugates) and Rodrigues in sinc form -- a short serial tail per iteration;
 *   TF_POSE_ALGEBRA_OPENCV4 / _OPENCV2: OpenCV's published algorithms as the oracle restates them
 *     for OpenCV 3.x-4.x / 2.4.9 (Matx_DetOp's LU, JacobiSVD + SVBkSb in float, Affine3::rotation
 *     with float rounding of every Matx operation; not checked against an OpenCV build, none is
 *     available) -- the reference's algebra (see DESIGN.md §2 for what the two algebras do to a
 *     sequence).
 * Default: TF_POSE_ALGEBRA_OPENCV4 (the reference's algebra; the persistent ICP runs its Jacobi SVD
 * lane-parallel).  The environment variable TFUSION_ICP_SOLVE=opencv4|opencv2|canonical sets it
 * at tf_create.
 * TF_INVALID_ARG if the algebra's persistent ICP kernel would not fit the schedule chosen. */
enum { TF_POSE_ALGEBRA_CANONICAL = 0, TF_POSE_ALGEBRA_OPENCV2 = 2, TF_POSE_ALGEBRA_OPENCV4 = 4 };
tf_status tf_set_pose_algebra(tf_ctx* ctx, int algebra);
tf_status tf_get_pose_algebra(tf_ctx* ctx, int* algebra);
/* One ICP iteration's algebra on caller systems (no context): for each of n systems given as
 * the 27 sums of estimateTransform's reduction (StreamHelper layout, projective_icp.cpp:51-61),
 * det[q] = cv::determinant(A) and x[q] = cv::solve(A, b, DECOMP_SVD) (:197-206) under the
 * algebra TF_POSE_ALGEBRA_* -- the same device code the persistent ICP runs (OpenCV algebras:
 * the lane-parallel Jacobi SVD).  Device buffers: sums 27 n floats, x 6 n floats, det n doubles
 * (may be NULL); asynchronous on `stream` (NULL: the null stream). */
tf_status tf_icp_solve_systems(int algebra, const float* dev_sums, int n, float* dev_x, double* dev_det, void* stream);
/* The record of the context's last estimateTransform (a frame's or a stage call's), as the device
 * left it: the working affine (row-major 3x4; on a failed det check the last composition taken),
 * the 27 sums of the last iteration run (the failing one's on failure), ok (1, 0 = det check
 * failed, -1 = the launch reported a lost peer) and the iterations run.  Any pointer may be NULL.
 * Synchronous. */
tf_status tf_icp_get_result(tf_ctx* ctx, float affine_rt[12], float sums[27], int* ok, int* iterations);

/* ---- stage entry points (operate on context state; parity tests) ------------- */
/* computeDists + depthBilateralFilter + depthTruncation + depthBuildPyramid +
 * computePointNormals (topfu.cpp:166-197; imgproc.cpp:3-48) into the curr pyramid */
tf_status tf_stage_preprocess(tf_ctx* ctx, const uint16_t* dev_depth, size_t pitch_bytes);
/* same, host depth */
tf_status tf_stage_preprocess_host(tf_ctx* ctx, const uint16_t* host_depth, size_t pitch_bytes);
/* ProjectiveICP::estimateTransform(points overload) (projective_icp.cpp:169-213) on
 * the context's curr/prev pyramids; affine_rt (out) row-major 3x4. */
tf_status tf_stage_icp(tf_ctx* ctx, float affine_rt[12], int* ok, int* iterations);
/* SceneReconstructionEngine_CUDA::AllocateSceneFromDepth
 * (SceneReconstructionEngine_host.cu:75-195) with the context's dists */
tf_status tf_stage_alloc(tf_ctx* ctx, const float pose_rt[12]);
/* ::IntegrateIntoScene (SceneReconstructionEngine_host.cu:197-251) */
tf_status tf_stage_integrate(tf_ctx* ctx, const float pose_rt[12]);
/* VisualisationEngine_CUDA::CreateExpectedDepths (VisualisationEngine_CUDA.cu:119-173) */
tf_status tf_stage_expected_depths(tf_ctx* ctx, const float pose_rt[12]);
/* GenericRaycast (VisualisationEngine_CUDA.cu:175-218) into raycastResult */
tf_status tf_stage_raycast(tf_ctx* ctx, const float invM_rt[12], int update_visible);
/* renderICP_device + resizePointsNormals (VisualisationEngine_CUDA.cu:323-360,
 * topfu.cpp:308-309): raycastResult -> prev points/normals pyramid */
tf_status tf_stage_icp_maps(tf_ctx* ctx, const float invM_rt[12]);
/* renderGrey_device (VisualisationHelper.hpp:105-118) from raycastResult */
tf_status tf_stage_render_grey(tf_ctx* ctx, const float invM_rt[12]);
/* ResetScene (SceneReconstructionEngine_host.cu:51-73) only */
tf_status tf_stage_reset_scene(tf_ctx* ctx);
/* swap curr <-> prev points/normals pyramids (topfu.cpp:205-207) */
tf_status tf_stage_swap_pyramids(tf_ctx* ctx);

/* ---- engine entry points over caller buffers (the L4 C++ API, include/tfusion/engines.hpp) --
 * Poses are row-major 3x4 [R|t]; intr = {fx, fy, cx, cy} (Intr, types.hpp:20-26) and overrides the
 * context's intrinsics for the call; dists / maps are caller device buffers with a row step in
 * bytes, rows x cols of the context's image size.  All synchronous. */
/* cuda::ProjectiveICP::setDistThreshold / setAngleThreshold / setIterationsNum
 * (projective_icp.cpp:81-101): the tracker parameters the context's frames use from now on */
tf_status tf_icp_set_params(tf_ctx* ctx, float dist_thres, float angle_thres, const int iters[4]);
tf_status tf_icp_get_params(tf_ctx* ctx, float* dist_thres, float* angle_thres, int iters[4]);
/* one level of a point/normal pyramid: float4 maps, row steps in bytes */
typedef struct tf_map_level {
    const void* points; size_t points_step;
    const void* normals; size_t normals_step;
} tf_map_level;
/* cuda::ProjectiveICP::estimateTransform(affine, intr, vcurr, ncurr, vprev, nprev)
 * (projective_icp.cpp:169-213) on caller pyramids (level l is (cols >> l) x (rows >> l)); the
 * maps are copied into the context's current/previous pyramids first.  affine_rt receives the
 * estimate (the last successful composition when *ok == 0, as the reference leaves it). */
tf_status tf_icp_estimate(tf_ctx* ctx, const float intr[4], const tf_map_level* curr, const tf_map_level* prev,
                          int levels, float affine_rt[12], int* ok, int* iterations);
/* SceneReconstructionEngine_CUDA::AllocateSceneFromDepth(scene, intr, pose, dists, renderState,
 * onlyUpdateVisibleList, resetVisibleList) (SceneReconstructionEngine_host.cu:75-195); pose is
 * world -> camera (TopFu passes poses_.back().inv(), topfu.cpp:281) */
tf_status tf_scene_alloc(tf_ctx* ctx, const float intr[4], const float pose_rt[12], const float* dists,
                         size_t dists_step, int only_update_visible_list, int reset_visible_list);
/* ::IntegrateIntoScene(scene, intr, pose, dists, renderState) (SceneReconstructionEngine_host.cu:197-251) */
tf_status tf_scene_integrate(tf_ctx* ctx, const float intr[4], const float pose_rt[12], const float* dists,
                             size_t dists_step);
/* ::IntegrateIntoScene with the view's RGB image (voxel_rgb: the Voxel_s_rgb colour update;
 * SceneReconstructionEngine_host.cu:217 M_rgb = calib_inv * M_d, :245-247 the rgb arguments) */
tf_status tf_scene_integrate_rgb(tf_ctx* ctx, const float intr[4], const float pose_rt[12], const float* dists,
                                 size_t dists_step, const uint8_t* dev_rgb, size_t rgb_step);
/* The swapping engine of the GlobalCache's lineage, run after integration when use_swapping is
 * set (every frame of tf_process_frame(s) does it): IntegrateGlobalIntoLocal + SaveToGlobalMemory
 * (InfiniTAM ITMSwappingEngine_CUDA, whose instantiation the reference comments out,
 * CUDAInstantiations.cu:8); its semantics are written out in DESIGN.md §Swapping. */
tf_status tf_scene_swap(tf_ctx* ctx);
/* the two halves on their own: SwappingEngine::IntegrateGlobalIntoLocal(scene, renderState) and
 * ::SaveToGlobalMemory(scene, renderState); tf_scene_swap == swap_in then swap_out */
tf_status tf_scene_swap_in(tf_ctx* ctx);
tf_status tf_scene_swap_out(tf_ctx* ctx);
/* blocks swapped in / out and reallocated by the last frame (or tf_scene_* call) */
tf_status tf_swap_counts(tf_ctx* ctx, int counts[3]);
/* The state after each frame of tf_scene_fuse_frames (no reference counterpart: the reference keeps
 * these counters host-side, LocalVBA.hpp:26, VoxelBlockHash.hpp:69, RenderState_VH.hpp:33, and its
 * allocation failures are silent, SceneReconstructionEngine_host.cu:374-381, 398-401). */
typedef struct tf_fuse_record {
    int lastFreeBlockId;
    int lastFreeExcessListId;
    int noVisibleEntries;
    int alloc_failed_type1;             /* this frame's requests refused for want of a free block */
    int alloc_failed_type2;             /* ... excess-list requests refused (no block or no excess slot) */
    int swapped_in;                     /* use_swapping: IntegrateGlobalIntoLocal's state 1 -> 2 entries */
    int swapped_out;                    /* SaveToGlobalMemory's blocks moved to the GlobalCache and freed */
    int swap_realloc;                   /* reAllocateSwappedOutVoxelBlocks' blocks */
    int swapped_in_merged;              /* stored blocks merged back into the VBA */
    int pad;
} tf_fuse_record;
/* Engine-level fusion of n device-resident frames at given poses with no host round trip inside,
 * TopFu's call order without the tracker: for frame k, cuda::computeDists(depth_k) (imgproc.cu:
 * 263-290, topfu.cpp:166), SceneReconstructionEngine_CUDA::AllocateSceneFromDepth(scene, intr,
 * poses[k], dists, renderState) and ::IntegrateIntoScene(...) (SceneReconstructionEngine_host.cu:
 * 75-251, topfu.cpp:202-203), then with use_swapping the swapping engine (tf_scene_swap).  The
 * results equal tf_imgproc_compute_dists + tf_scene_alloc + tf_scene_integrate (+ tf_scene_swap)
 * called per frame.  dev_frames: uint16 depth, frame k at dev_frames + k * frame_stride_bytes, rows
 * pitch_bytes apart (0: cols * 2); poses_rt: n world -> camera poses (host, row-major [R|t], as
 * tf_scene_alloc takes them); intr: NULL = the context's; records: NULL or n host records.
 * Returns when the batch is done. */
tf_status tf_scene_fuse_frames(tf_ctx* ctx, const float intr[4], const uint16_t* dev_frames, size_t frame_stride_bytes,
                               size_t pitch_bytes, const float* poses_rt, int n, tf_fuse_record* records);
/* GlobalCache::SaveToFile / ReadFromFile (GlobalCache.hpp:79-110): hasStoredData as one byte per
 * entry, then every entry's 512 voxels (4 B each), n_buckets + n_excess entries */
tf_status tf_swap_save(tf_ctx* ctx, const char* path);
tf_status tf_swap_load(tf_ctx* ctx, const char* path);
/* VisualisationEngine_CUDA::CreateExpectedDepths(scene, pose, intr, renderState)
 * (VisualisationEngine_CUDA.cu:119-173); pose is world -> camera */
tf_status tf_vis_expected_depths(tf_ctx* ctx, const float intr[4], const float pose_rt[12]);
/* ::RenderImage(scene, pose, intr, renderState, image, type, raycastType)
 * (VisualisationEngine_CUDA.cu:220-291, 423-429); pose is camera -> world (Matrix4f(poses_.back()),
 * topfu.cpp:346-352); new_raycast = 1: RENDER_FROM_NEW_RAYCAST, 0: RENDER_FROM_OLD_RAYCAST (the
 * pixel stage on the current raycast result) */
tf_status tf_vis_render_image(tf_ctx* ctx, const float intr[4], const float pose_rt[12], int type, int new_raycast,
                              uint8_t* dev_rgba, size_t step);
/* ::CreateICPMaps(scene, pose, intr, points, normals, renderState) (VisualisationEngine_CUDA.cu:
 * 323-360, 473-493): castRay<true> + renderICP into the caller's level-0 maps; pose is camera -> world */
tf_status tf_vis_icp_maps(tf_ctx* ctx, const float intr[4], const float pose_rt[12], void* points, size_t points_step,
                          void* normals, size_t normals_step);

/* ---- cuda:: image processing over caller buffers (imgproc.hpp:9-31, imgproc.cu) --------
 * Stateless; stream = hipStream_t (NULL: the legacy default stream); all asynchronous on it.
 * Depth is uint16 millimetres, dists float, points / normals float4; steps in bytes. */
/* cuda::computeDists (imgproc.cu:263-290) */
tf_status tf_imgproc_compute_dists(const uint16_t* depth, size_t depth_step, float* dists, size_t dists_step,
                                   int cols, int rows, void* stream);
/* cuda::depthBilateralFilter (imgproc.cu:10-61); sigma_depth in metres as the reference takes it */
tf_status tf_imgproc_bilateral(const uint16_t* in, size_t in_step, uint16_t* out, size_t out_step, int cols, int rows,
                               int ksz, float sigma_spatial, float sigma_depth, void* stream);
/* cuda::depthTruncation (imgproc.cu:70-89), in place; threshold in metres */
tf_status tf_imgproc_truncate(uint16_t* depth, size_t step, int cols, int rows, float threshold, void* stream);
/* cuda::depthBuildPyramid (imgproc.cu:98-140): out is (cols/2) x (rows/2) */
tf_status tf_imgproc_pyr_down(const uint16_t* in, size_t in_step, int cols, int rows, uint16_t* out, size_t out_step,
                              float sigma_depth, void* stream);
/* cuda::computePointNormals (imgproc.cu:214-254) with intr = {fx, fy, cx, cy} of this level */
tf_status tf_imgproc_point_normals(const float intr[4], const uint16_t* depth, size_t depth_step, int cols, int rows,
                                   void* points, size_t points_step, void* normals, size_t normals_step, void* stream);
/* cuda::resizePointsNormals (imgproc.cu:355-401): outputs are (cols/2) x (rows/2) */
tf_status tf_imgproc_resize_points_normals(const void* points, size_t points_step, const void* normals,
                                           size_t normals_step, int cols, int rows, void* points_out,
                                           size_t points_out_step, void* normals_out, size_t normals_out_step,
                                           void* stream);
/* cuda::waitAllDefaultStream (imgproc.cpp:18-19) */
tf_status tf_imgproc_sync(void* stream);

/* ---- state transfer --------------------------------------------------------- */
/* host <-> context buffer copies; level selects the pyramid level for TF_BUF_DEPTH..
 * TF_BUF_PREV_NORMALS.  bytes must equal the buffer size (tf_buffer_bytes). */
tf_status tf_buffer_bytes(tf_ctx* ctx, int which, int level, size_t* bytes);
tf_status tf_download(tf_ctx* ctx, int which, int level, void* host, size_t bytes);
/* bytes [offset, offset + bytes) of a level-0 buffer (one entry of a large table) */
tf_status tf_download_range(tf_ctx* ctx, int which, size_t offset, void* host, size_t bytes);
tf_status tf_upload(tf_ctx* ctx, int which, int level, const void* host, size_t bytes);
tf_status tf_set_pose(tf_ctx* ctx, const float rt[12]);

/* ---- per-stage timing (SampledScopeTime, tfusion/include/tfusion/types.hpp:91-104) --
 * When enabled, every frame records HIP events around each stage on the context stream;
 * durations accumulate until tf_profile_reset.  Stage ids: */
typedef enum tf_stage_id {
    TF_STAGE_PREPROCESS = 0,      /* dists + bilateral + pyramid + vertex/normal maps */
    TF_STAGE_ICP = 1,             /* estimateTransform, all iterations */
    TF_STAGE_ALLOC = 2,           /* AllocateSceneFromDepth */
    TF_STAGE_INTEGRATE = 3,       /* IntegrateIntoScene (k_integrate only) */
    TF_STAGE_RAYCAST_RENDER = 4,  /* renderImage raycast (fused into TF_STAGE_RAYCAST_ICP in the frame) */
    TF_STAGE_GREY = 5,            /* renderGrey (fused likewise) */
    TF_STAGE_EXPECTED_DEPTHS = 6, /* CreateExpectedDepths */
    TF_STAGE_RAYCAST_ICP = 7,     /* CreateICPMaps raycast<true> + renderImage (k_raycast_pair) */
    TF_STAGE_ICP_MAPS = 8         /* renderICP + resizePointsNormals */
} tf_stage_id;
tf_status tf_profile_enable(tf_ctx* ctx, int enable);
/* time only the stages whose bit (1 << tf_stage_id) is set; 0 disables.  Each timed stage
 * adds two event records per frame to the stream, which cost GPU time of their own, so a
 * throughput measurement times only the stage it needs. */
tf_status tf_profile_stages(tf_ctx* ctx, unsigned mask);
/* time only every `period`-th frame enqueued from now on (1 = every frame, the default after
 * tf_profile_enable / tf_profile_stages): a throughput run keeps its stage timing live while
 * all but 1/period of its frames carry no events */
tf_status tf_profile_sample(tf_ctx* ctx, int period);
tf_status tf_profile_reset(tf_ctx* ctx);
/* ms[i] = accumulated milliseconds, counts[i] = frames measured, for i < n (n <= 9) */
tf_status tf_profile_read(tf_ctx* ctx, double* ms, long long* counts, int n);
tf_status tf_set_counters(tf_ctx* ctx, int lastFreeBlockId, int lastFreeExcessListId, int noVisibleEntries);
/* Frame totals accumulated on the device by every frame's end since tf_create or the last
 * tf_reset_totals (measurement; no reference counterpart -- the reference's only metric is the
 * SampledScopeTime average, tfusion/src/core.cpp:202-216). */
typedef struct tf_totals {
    long long frames;               /* TopFu::operator() calls completed */
    long long frames_tracked;       /* tracking path with ICP ok (alloc + integrate + both raycasts) */
    long long resets;               /* ICP failures -> reset (topfu.cpp:263-264) */
    long long visible_sum;          /* noVisibleEntries summed over the frames that integrated */
    long long tiles_sum;            /* noTotalBlocks summed over the tracked frames */
    long long swapped_in;           /* swap-ins (use_swapping): state-1 entries with a block set to state 2,
                                       whether or not the GlobalCache held data for them */
    long long swapped_out;          /* blocks swapped out: each one copied VBA -> GlobalCache and freed */
    long long integrate_lanes_read;     /* 16-B voxel lanes (4 voxels) integration read: those with an update */
    long long integrate_lanes_written;  /* ... and wrote back: those whose value changed */
    long long swapped_in_merged;    /* the swap-ins whose entry held stored data: GlobalCache -> VBA transfers */
    long long alloc_failed_type1;   /* allocation requests that failed silently for want of a free voxel block
                                       (allocateVoxelBlocksList, SceneReconstructionEngine_host.cu:374-381) */
    long long alloc_failed_type2;   /* ... excess-list requests that failed for want of a block or an excess
                                       slot (:386-411) */
    long long icp_fallbacks;        /* frames re-run on the per-iteration ICP schedule because the persistent
                                       launch lost a peer (not all of its workgroups were co-resident) */
} tf_totals;
tf_status tf_get_totals(tf_ctx* ctx, tf_totals* totals);
tf_status tf_reset_totals(tf_ctx* ctx);
/* Measurement: `iters` back-to-back launches of one stage's kernels on the context stream
 * with the pose/matrices of tf_stage_* (stage = TF_STAGE_INTEGRATE: k_integrate;
 * TF_STAGE_EXPECTED_DEPTHS: k_ed_fill over the boxes one projection pass of the current list
 * made first;
 * TF_STAGE_RAYCAST_ICP: castRay<true> into raycastResult; TF_STAGE_RAYCAST_RENDER: the frame's
 * k_raycast_pair -- castRay<true> + renderImage's castRay and grey, over the current range
 * image), timed by HIP events on that stream; *ms_per_iter = elapsed / iters.  The scene is
 * updated by every launch exactly as by tf_stage_integrate / tf_stage_raycast. */
tf_status tf_time_stage(tf_ctx* ctx, int stage, const float pose_rt[12], int iters, float* ms_per_iter);

/* ---- mesh extraction (additions: the reference has no mesher, nothing here replaces a reference
 * interface) ------------------------------------------------------------------------------------
 * Marching tetrahedra on the Kuhn split of every voxel cube of every allocated block (hash entries
 * with ptr >= 0), specified to the bit in DESIGN.md (Mesh extraction): a cube is meshed when all
 * eight corner voxels exist with w > 0, a corner is inside when its sdf short is < 0, vertices are
 * world positions (voxel coordinate * voxelSize, as integration and raycast place them).  The scene
 * is only read.
 * Two readings of a swapping scene.  The resident one (every entry point without TF_MESH_WHOLE): blocks
 * swapped out to the GlobalCache (ptr == -1) are not meshed and count as missing for their neighbours'
 * cubes, and a block is read as it lies in the VBA.  The whole one (tf_mesh_extract_whole, TF_MESH_WHOLE in
 * tf_mesh_save_ply_attr's attrs): every hash entry that holds voxel data in either tier is meshed, and every
 * block -- own, cube neighbour, gradient neighbour -- is resolved the same way: the active block; the stored
 * block as it is where the entry is swapped out; CombineVoxelInformation(stored, active, maxW) per voxel
 * where a stored block still awaits its merge, i.e. what the engine's next IntegrateGlobalIntoLocal would
 * write (Mesh extraction, the whole map).  The GlobalCache is read where it lies; nothing is
 * swapped in and neither tier is written.  On a context with no stored data -- any context without
 * use_swapping, a swapping one before its first eviction -- the whole mesh is byte-identical to the
 * resident one.  The indexed form exists in both readings: tf_mesh_extract_indexed and tf_mesh_save_ply_indexed
 * are resident-only (their edge bits are keyed by VBA block, which a stored block does not have);
 * tf_mesh_extract_indexed_whole and tf_mesh_save_ply_indexed_whole give the whole reading's triangles as a vertex
 * table and indices, their edge bits keyed by a compact numbering of the entries that resolve. */
/* addition (no reference counterpart): triangles in a fixed order (ascending hash entry, voxel
 * x + 8y + 64z, tetrahedron, triangle of the case) as float[n][9] -- three xyz vertices, right-hand
 * normal towards sdf >= 0 -- into the device buffer: the first min(n, capacity) of them;
 * *n_triangles = the full count n.  capacity 0 (dev_triangles may be NULL) only counts.  Two
 * extractions of one scene are byte-identical.  Synchronous. */
tf_status tf_mesh_extract(tf_ctx* ctx, float* dev_triangles, long long capacity, long long* n_triangles);
/* addition (no reference counterpart): host only, no context -- n triangles (float[n][9]) as a binary
 * little-endian PLY: vertices welded by exact bit equality of their three floats (in unspecified
 * order), faces of three int indices in the input order */
tf_status tf_mesh_write_ply(const char* path, const float* host_triangles, long long n);
/* addition (no reference counterpart): count, extract into a temporary device buffer, download,
 * tf_mesh_write_ply; TF_OOM when the buffers cannot be had */
tf_status tf_mesh_save_ply(tf_ctx* ctx, const char* path);

/* Per-vertex attributes (Mesh extraction, attributes).  Every vertex lies on a cube edge
 * between two voxels; its normal is the TSDF's integer gradient at the two (central differences, one-sided
 * next to a missing or unobserved voxel) interpolated like the position and normalised -- it points
 * towards free space, as the triangles' right-hand normal does -- and its colour the colour plane's
 * words at the two, interpolated where both have w_color > 0.  Both are functions of the edge alone. */
#define TF_MESH_NORMALS 1
#define TF_MESH_COLOURS 2
/* addition (no reference counterpart): tf_mesh_extract with up to three outputs for the same triangles in
 * the same order, each skipped when its pointer is NULL: positions float[n][9] (byte-identical to
 * tf_mesh_extract's), unit normals float[n][9] (three xyz per triangle; (0, 0, 0) where the gradient
 * vanishes), colours uint8[n][12] (RGBA per vertex, alpha 255, or 0 0 0 0 where neither end of the edge
 * has colour; the buffer 4-byte aligned).  All are clipped at the same capacity; with all three NULL
 * capacity must be 0 (count only).  dev_colours on a context without voxel_rgb is TF_INVALID_ARG.
 * *n_triangles = the full count.  Synchronous; the scene is only read. */
tf_status tf_mesh_extract_attr(tf_ctx* ctx, float* dev_triangles, float* dev_normals, uint8_t* dev_colours,
                               long long capacity, long long* n_triangles);
/* addition (no reference counterpart): host only, no context -- tf_mesh_write_ply with vertex properties
 * x y z, then nx ny nz when host_normals is given, then red green blue alpha (uchar) when host_colours
 * is; vertices welded by exact bit equality of the whole record (position and attributes), faces in the
 * input order.  With both attribute pointers NULL the file is tf_mesh_write_ply's, byte for byte. */
tf_status tf_mesh_write_ply_attr(const char* path, const float* host_triangles, const float* host_normals,
                                 const uint8_t* host_colours, long long n);
/* addition (no reference counterpart): count, extract into temporary device buffers, download,
 * tf_mesh_write_ply_attr; attrs = TF_MESH_NORMALS | TF_MESH_COLOURS or either or 0; TF_OOM when the
 * buffers cannot be had, TF_INVALID_ARG for TF_MESH_COLOURS without voxel_rgb.  With TF_MESH_WHOLE the file
 * holds the whole reading's mesh (normals too when asked for; TF_MESH_COLOURS with it is TF_INVALID_ARG: a
 * swapping scene has no colour plane).  The writer is the same: one device buffer, one host copy, one weld,
 * so the caller's memory bounds the mesh that can be saved in one piece. */
tf_status tf_mesh_save_ply_attr(tf_ctx* ctx, const char* path, int attrs);

#define TF_MESH_WHOLE 8
/* addition (no reference counterpart): tf_mesh_extract_attr's positions and normals in the whole reading
 * (above): the same order (ascending hash entry over the entries that resolve, then voxel, tetrahedron,
 * triangle), the same capacity, count-only and NULL rules (either pointer may be NULL; with both NULL
 * capacity must be 0), *n_triangles = the full count.  A normal's "usable voxel" is one whose block resolves
 * and whose resolved w > 0.  Synchronous; the scene and the GlobalCache are only read. */
tf_status tf_mesh_extract_whole(tf_ctx* ctx, float* dev_triangles, float* dev_normals, long long capacity,
                                long long* n_triangles);

/* The indexed form (Mesh extraction, indexed): the same triangles with shared vertices.  A vertex
 * is the cube edge it lies on -- (p, d), p the edge's lower voxel, d in {0,1}^3 \ {0} -- and exists when a
 * triangle of tf_mesh_extract has a vertex there; two edges are never merged, even where their positions
 * are equal bit for bit, and no vertex is unreferenced.  Vertices are numbered by ascending hash entry of
 * p's block, then p's voxel index x + 8y + 64z in it, then dx | dy << 1 | dz << 2. */
#define TF_MESH_INDEXED 4
/* addition (no reference counterpart): the vertex table -- positions float[nv][3], unit normals float[nv][3],
 * colours uint8[nv][4] RGBA (voxel_rgb contexts only), each skipped when its pointer is NULL and clipped at
 * vertex_capacity -- and indices uint32[nt][3], clipped at triangle_capacity, for tf_mesh_extract's triangles
 * in its order: vertices[indices] is tf_mesh_extract's float[nt][9] bit for bit, and normals / colours
 * [indices] are tf_mesh_extract_attr's.  An index keeps its true value even when it points past
 * vertex_capacity.  *n_vertices and *n_triangles are always the full counts.  A capacity of 0 (its buffers may
 * be NULL) writes nothing of that part; both 0 only counts.  TF_INVALID_ARG: a negative capacity, a non-zero
 * capacity with its buffers NULL, a NULL count pointer or ctx, dev_colours without voxel_rgb.
 * TF_INDEX_RANGE: more than 2^32 - 1 vertices -- the counts are returned, nothing is written.  TF_OOM when the
 * scratch (448 B of edge bits and as much of prefixes per VBA block, allocated by the first call and kept
 * by the context) cannot be had.  Two extractions of one scene are byte-identical.  Synchronous; the scene
 * is only read. */
tf_status tf_mesh_extract_indexed(tf_ctx* ctx, float* dev_vertices, float* dev_normals, uint8_t* dev_colours,
                                  long long vertex_capacity, uint32_t* dev_indices, long long triangle_capacity,
                                  long long* n_vertices, long long* n_triangles);
/* addition (no reference counterpart): host only, no context -- the vertex table as given (no welding, order
 * and duplicate positions kept) and nt faces as a binary little-endian PLY with tf_mesh_write_ply_attr's
 * property layout and face format.  TF_INVALID_ARG also for nv > 2^31 - 1 or an index >= nv. */
tf_status tf_mesh_write_ply_indexed(const char* path, const float* host_vertices, const float* host_normals,
                                    const uint8_t* host_colours, long long nv, const uint32_t* host_indices, long long nt);
/* addition (no reference counterpart): count, extract the indexed buffers into a temporary device buffer,
 * download them (and nothing else), tf_mesh_write_ply_indexed; attrs as tf_mesh_save_ply_attr's
 * (TF_MESH_INDEXED may be set and changes nothing); TF_INDEX_RANGE beyond 2^31 - 1 vertices.  Resident
 * only: TF_MESH_WHOLE in attrs is TF_INVALID_ARG (see DESIGN.md §10 for what rekeying the edge bits by hash
 * entry would take) */
tf_status tf_mesh_save_ply_indexed(tf_ctx* ctx, const char* path, int attrs);

/* addition (no reference counterpart): tf_mesh_extract_indexed in the whole reading -- tf_mesh_extract_whole's
 * triangles in its order as a vertex table (positions float[nv][3], normals float[nv][3]; no colours: a swapping
 * scene has no colour plane) and indices uint32[nt][3]: vertices[indices] is tf_mesh_extract_whole's float[nt][9]
 * bit for bit, normals[indices] its normals.  A vertex is its Kuhn edge (p, d), as above; the edge's owner is the
 * first entry on the hash walk of block floor(p / 8) that resolves (ptr >= 0, or ptr == -1 with stored data), and
 * vertices are numbered by ascending owner hash entry, then p's voxel index in the owner block, then
 * dx | dy << 1 | dz << 2.  The capacity, NULL, count-only, full-count and TF_INDEX_RANGE rules are
 * tf_mesh_extract_indexed's, without the colour column.  On a context with no stored data the result is
 * tf_mesh_extract_indexed's byte for byte (the same kernels).  TF_OOM when the scratch cannot be had -- one int
 * per hash entry, and 448 B of edge bits and as much of prefixes per entry that RESOLVES (not per hash entry, not
 * per VBA block), kept by the context and grown geometrically when a later extraction finds more entries; the
 * context stays usable.  The resident form's scratch is separate: the two may alternate on one context.  Two
 * extractions of one scene are byte-identical.  Synchronous; the scene and the GlobalCache are only read. */
tf_status tf_mesh_extract_indexed_whole(tf_ctx* ctx, float* dev_vertices, float* dev_normals, long long vertex_capacity,
                                        uint32_t* dev_indices, long long triangle_capacity, long long* n_vertices,
                                        long long* n_triangles);
/* addition (no reference counterpart): the whole map as an indexed PLY, written in bounded pieces.  attrs: 0 or
 * TF_MESH_NORMALS (any other bit is TF_INVALID_ARG).  The columns of tf_mesh_extract_indexed_whole stay in a
 * temporary device buffer and come to the host a chunk at a time through a pinned staging buffer kept by the
 * context (TFUSION_MESH_CHUNK_BYTES bytes, read at tf_create; default 8388608 = 8 MiB; values outside
 * [24, 2^30] read as the default); the streaming writer below interleaves each chunk into vertex records and then
 * face records, so host memory is bounded by the chunk, never by the mesh.  The file is tf_mesh_write_ply_indexed's
 * for the extracted arrays, byte for byte, whatever the chunk size.  TF_INDEX_RANGE beyond 2^31 - 1 vertices;
 * TF_OOM when a buffer cannot be had; every index is checked against nv, chunk by chunk (TF_INVALID_ARG).  On
 * any failure no file is left. */
tf_status tf_mesh_save_ply_indexed_whole(tf_ctx* ctx, const char* path, int attrs);

/* addition (no reference counterpart): the streaming form of tf_mesh_write_ply_indexed -- host only, no context.
 * begin writes the header for nv vertices and nt faces with the columns attrs names (TF_MESH_NORMALS,
 * TF_MESH_COLOURS); then the vertices in any number of pieces (normals / colours as attrs declared them, NULL
 * otherwise), then the faces in any number of pieces (all vertices first; an index >= nv fails); end closes the
 * file.  The writer's memory is a fixed record buffer.  After a failed call every further append fails, and end
 * -- which must be called exactly once after a successful begin, and frees the stream -- removes the file and
 * returns TF_INVALID_ARG, as it does when fewer records were appended than begin declared.  commit == 0: the
 * caller gives up; the file is removed and end returns TF_OK. */
typedef struct tf_ply_stream tf_ply_stream;
tf_status tf_mesh_ply_begin(const char* path, long long nv, long long nt, int attrs, tf_ply_stream** out);
tf_status tf_mesh_ply_vertices(tf_ply_stream* s, const float* host_vertices, const float* host_normals,
                               const uint8_t* host_colours, long long n);
tf_status tf_mesh_ply_faces(tf_ply_stream* s, const uint32_t* host_indices, long long n);
tf_status tf_mesh_ply_end(tf_ply_stream* s, int commit);

/* ---- scene checkpoints (additions: the reference cannot save its map; DESIGN.md §5 Scene checkpoints) --
 * A checkpoint is the state a sequence resumes from, sized by what is live: the hash entries that differ
 * from ResetScene's, their voxel (and colour) blocks, visType where non-zero, visibleIds[0, noVisibleEntries),
 * the live parts of the two free lists, the counters, frame_counter, the pose and the previous points /
 * normals pyramid.  A context that loads a checkpoint is indistinguishable, bit for bit, from the one that
 * saved it, now and after any further frames.  Contexts with use_swapping are refused (TF_INVALID_ARG) by
 * these two calls: their checkpoint, GlobalCache included, is tf_map_save / tf_map_load's (below). */
/* addition (no reference counterpart): writes the checkpoint of the current state to path.  Synchronous, the
 * scene is only read; two saves of one state are byte-identical, and a save straight after tf_scene_load of
 * file F is byte-identical to F.  TF_INVALID_ARG: NULL arguments, use_swapping, a path that cannot be
 * written, and a state that tf_scene_load would refuse -- tables or counters that came through tf_upload /
 * tf_set_counters with a ptr outside the VBA or named twice, a chain offset past the excess list, a counter
 * or a live list / visible-list value outside its table (checked by load's own rule; no file is left);
 * TF_HIP_ERROR on a context in error; TF_OOM.  The blocks travel through a bounded staging buffer
 * (TFUSION_CKPT_CHUNK_BLOCKS blocks, read at tf_create; default 4096), kept by the context after the first call. */
tf_status tf_scene_save(tf_ctx* ctx, const char* path);
/* addition (no reference counterpart): replaces the context's scene, pose, frame counter and tracker maps by
 * the file's.  The context must agree with the file in cols, rows, n_buckets, n_excess, n_blocks, voxel_rgb,
 * use_swapping == 0 and the bits of voxelSize, mu, maxW; its tracker parameters, pose algebra and intrinsics
 * stay its own.  The whole file is read and validated on the host first: TF_INVALID_ARG (a missing, truncated,
 * corrupt or mismatched file, use_swapping) leaves the context exactly as it was.  Synchronous. */
tf_status tf_scene_load(tf_ctx* ctx, const char* path);
/* what a checkpoint file holds, from its header */
struct tf_scene_file_info {
    tf_params params;               /* the saving context's tf_get_params */
    int pose_algebra, frame_counter;
    int lastFreeBlockId, lastFreeExcessListId, noVisibleEntries;
    long long n_records, n_blocks_stored, file_bytes;
    float pose[12];
};
/* addition (no reference counterpart): host only, no context, no GPU call -- the header of the file at path,
 * checked against its checksum and the file's length.  (The struct is named by its tag: C has one name
 * space for typedefs and functions.) */
tf_status tf_scene_file_info(const char* path, struct tf_scene_file_info* info);
/* addition (measurement; no reference counterpart): what the context's last tf_scene_save / tf_scene_load
 * spent, in milliseconds, by the host clock: ms[2] the D2H / H2D copies, ms[3] the file reads / writes, ms[6]
 * the record check and checksum (load: the whole validation), ms[4] the whole call.  On a context created
 * with the environment variable TFUSION_CKPT_TIMING=1 the kernels are also timed, by HIP events on the context
 * stream and a wait after each group (0 otherwise): ms[0] the index kernels (save: count + prefix + records;
 * load: records -> hash, visType, block grid), ms[1] the block kernels (gather / scatter, summed over the
 * chunks).  ms[5] is not a time: the bytes the block kernels read + wrote.  ms[7] is 0. */
tf_status tf_scene_ckpt_times(tf_ctx* ctx, double ms[8]);

/* ---- map checkpoints (additions; DESIGN.md §5 Map checkpoints) ------------------------------------------
 * The checkpoint of a context with or without use_swapping.  A swapping context's state is the scene
 * checkpoint's state plus the GlobalCache: swapState and hasStoredData per entry and the stored block of
 * every entry whose flag is 1 (a stored block whose flag is 0 is read by nobody and is not state).  It is
 * written as version 2 of the checkpoint file: the records carry the two bytes, and the stored blocks follow
 * the active ones as a second payload in record order.  A swapping context that loads a map checkpoint is
 * indistinguishable, bit for bit, from the one that saved it, now and after any further frames or engine
 * calls.  Not stored: the last call's tf_swap_counts (zero after a load) and the totals. */
/* addition (no reference counterpart): on a context without use_swapping tf_scene_save's file, byte for byte
 * (version 1); on a swapping context the version-2 file.  tf_scene_save's guarantees: synchronous, the scene
 * and the cache are only read; two saves of one state are byte-identical, a save straight after tf_map_load
 * of file F is byte-identical to F; a state that tf_map_load would refuse (also: a swap state > 2, a stored
 * flag > 1) is TF_INVALID_ARG with no file left; every block travels through the same bounded staging buffer
 * (TFUSION_CKPT_CHUNK_BLOCKS). */
tf_status tf_map_save(tf_ctx* ctx, const char* path);
/* addition (no reference counterpart): a version-1 file into a context without use_swapping (exactly
 * tf_scene_load), a version-2 file into a swapping context: the file's use_swapping must equal the context's,
 * the other agreement rules are tf_scene_load's (swap_transfer_blocks stays the context's own, as the tracker
 * parameters do).  The whole file is validated on the host before the context is touched: TF_INVALID_ARG
 * leaves it exactly as it was, the three GlobalCache buffers included.  Stored blocks of entries the file does
 * not flag are left as they are (no clear of the store); states and flags are the file's over the whole table. */
tf_status tf_map_load(tf_ctx* ctx, const char* path);
/* what a map checkpoint file holds, from its header: version 1 or 2; n_cache_blocks is 0 for version 1 */
struct tf_map_file_info {
    struct tf_scene_file_info scene;
    int version;
    long long n_cache_blocks;
};
/* addition (no reference counterpart): host only, no context, no GPU call -- the header of a version-1 or
 * version-2 file, checked against its checksum and the file's length.  (tf_scene_file_info and tf_scene_load
 * refuse a version-2 file, as any unknown version.) */
tf_status tf_map_file_info(const char* path, struct tf_map_file_info* info);
/* tf_scene_ckpt_times reports the last tf_map_save / tf_map_load too: the cache blocks' kernel time is part
 * of ms[1], their bytes of ms[5]. */

/* ---- resized load (addition; DESIGN.md §5 Resized load) --------------------------------------------------
 * A map checkpoint into a context whose n_buckets, n_excess or n_blocks are not the file's: the records are
 * re-hashed on the way in.  The result is the state a freshly reset context of the target's capacities reaches
 * when the file's records with a block position (entry.ptr >= -1), in file order, are inserted one at a time by
 * the reference's allocation rule: the bucket entry, or the end of the bucket's chain linked to
 * excessList[lastFreeExcessListId--]; a block from allocList[lastFreeBlockId--] where the record has one.  Both
 * free lists are the identity afterwards.  Records with ptr < -1 (a reset entry that only kept a visType, a swap
 * state or a stored flag) have no position and are dropped, a stored block of theirs with them.  visibleIds is
 * rebuilt: the ascending entries with visType > 0, the first vis_capacity of them.  Pose, frame counter and
 * previous maps are the file's.  Two loads of one file give byte-identical contexts. */
struct tf_resize_report {
    long long records_carried;   /* records with a block position (ptr >= -1) placed in the new table */
    long long records_dropped;   /* records with ptr < -1: no position, cannot be re-hashed */
    long long blocks;            /* VBA blocks placed (records with ptr >= 0) */
    long long cache_blocks;      /* GlobalCache blocks placed (carried records with hasStoredData) */
    long long excess_used;       /* excess-list slots taken */
    int longest_chain;           /* entries on the longest bucket chain, bucket entry included */
    int pad;
};
/* addition (no reference counterpart): a version-1 file into a context without use_swapping, a version-2 file
 * into a swapping one.  File and context must agree in cols, rows, voxel_rgb, use_swapping as a boolean, the
 * bits of voxelSize and mu, and maxW (else TF_INVALID_ARG, as for a file tf_map_load would refuse as invalid);
 * n_buckets, n_excess, n_blocks, vis_capacity, max_render_blocks and swap_transfer_blocks are the context's own.
 * TF_CAPACITY: more records with a block than n_blocks, or more chained records than n_excess.  Every refusal
 * leaves the context exactly as it was, the three GlobalCache buffers included.  report may be NULL; it is
 * filled on TF_OK and on TF_CAPACITY (what would have been needed), zeroed otherwise.  tf_scene_ckpt_times
 * reports the call as tf_map_load's, the placement kernels in ms[0].  Continuing a sequence after a resized load
 * reproduces the saving context's frames when n_buckets is the file's. */
tf_status tf_map_load_resized(tf_ctx* ctx, const char* path, struct tf_resize_report* report);

/* ---- map merge (addition; DESIGN.md §5 Map merge) ---------------------------------------------------------
 * A version-1 checkpoint fused into the live scene, block by block.  The file's records with a block (ptr >= 0,
 * the carried records), in file order and with block_offset added to their block position, are applied one at a
 * time: the reference's allocation walk looks the position up in the live table.  Found with a block: every voxel
 * of it becomes CombineVoxelInformation(file voxel, context voxel, maxW) -- a file voxel of weight 0 leaves the
 * context's as it is.  Found with ptr == -1: the entry takes allocList[lastFreeBlockId--] and the file's block is
 * copied.  Not found: inserted by the reference's allocation rule -- the free bucket entry, or
 * excessList[lastFreeExcessListId--] linked to the end of the bucket's chain -- with a block from the alloc list,
 * the file's block copied, visType 0.  The visible list, the pose, the frame counter, the tracker's maps, the
 * range image, the raycast result and every view stay as they are; the block grid gets the new blocks; the
 * context counts as after a hash upload.  Two merges of one file into byte-identical contexts give byte-identical
 * contexts. */
struct tf_merge_report {
    long long records_combined;  /* position already held a block: combined voxel by voxel */
    long long records_inserted;  /* position new to the table: entry and block added */
    long long records_revived;   /* position found with ptr == -1: given a block, the file's copied */
    long long records_skipped;   /* file records with ptr < 0: no voxels to give */
    long long blocks_used;       /* VBA blocks taken from the free list (inserted + revived) */
    long long excess_used;       /* excess-list slots taken */
};
/* addition (no reference counterpart).  block_offset: NULL or three ints added to every record's block position
 * (whole blocks).  The context must have use_swapping == 0 and voxel_rgb == 0 and so must the file, a version-1
 * one; both agree in the bits of voxelSize and mu and in maxW; cols, rows, the capacities and the intrinsics
 * need not agree.  The file's pose, frame counter, previous maps, visible list, free lists and visType bytes are
 * ignored.  TF_INVALID_ARG otherwise, for a file tf_map_load would refuse as invalid, for an offset that takes a
 * carried position outside the int16 range, and for two carried records of one position.  TF_CAPACITY: more
 * blocks needed than lastFreeBlockId + 1, or more excess slots than lastFreeExcessListId + 1.  Every refusal is
 * decided before the first write and leaves the context exactly as it was.  report may be NULL; it is filled on
 * TF_OK and on TF_CAPACITY (what would have been needed), zeroed otherwise.  Synchronous.  tf_scene_ckpt_times
 * reports the call as a load: the placement kernels in ms[0], the block kernel in ms[1], its bytes in ms[5]. */
tf_status tf_map_merge(tf_ctx* ctx, const char* path, const int block_offset[3], struct tf_merge_report* report);

/* ---- free views (addition; DESIGN.md §5 Free views) -------------------------------------------------------
 * A tf_view is a second render state bound to a context: its own image size, visible list, range image, raycast
 * result, output image, expected-depth scratch and device state block.  It owns no scene data: it reads the
 * context's hash, VBA and colour plane where they lie.  With it the map is rendered from any pose at any size
 * (a thumbnail, a 1280x960 still from a 640x480 tracker) and the tracker does not notice: no view call changes a
 * TF_BUF_* buffer of the context, its counters, its pose, its device state or the raycast pair's tile order, so
 * a context with view calls between its frames produces, bit for bit, the frames of one without.
 *
 * tf_view_find_visible is VisualisationEngine::FindVisibleBlocks (buildCompleteVisibleList_device,
 * VisualisationHelper.cu:17-50): the list holds every entry index i in [0, n_buckets + n_excess) with
 * hash[i].ptr >= 0 and checkBlockVisibility<false> true for the view's cols, rows, the call's intrinsics and the
 * context's voxelSize -- the plain frustum, never the enlarged one, also on a swapping context -- in ascending i
 * (the reference's order is an atomic race; with a binding max_render_blocks the order decides which blocks
 * CreateExpectedDepths drops).  If more entries qualify than vis_capacity the call returns TF_CAPACITY, *n_visible
 * holds the number needed and the view's buffers stay as they were.
 *
 * A view has a reading of the scene (tf_set_view_reading).  TF_VIEW_RESIDENT, the default: the blocks in the VBA
 * (ptr >= 0), as the tracker sees them; on a swapping context the blocks held in the GlobalCache are not raycast.
 * TF_VIEW_WHOLE: both tiers of a swapping context -- every stage behaves as the resident stage would on the scene
 * resolved by the table above (the mesher's, TF_MESH_WHOLE): an entry holds its active block, per voxel
 * CombineVoxelInformation(stored, active, maxW) while a merge is pending, or its stored block, and the block at a
 * position is the first entry of its chain that resolves.  tf_view_find_visible then lists the entries that resolve
 * (ptr >= 0, or ptr == -1 with stored data), CreateExpectedDepths projects each of them, and every voxel read of the
 * raycast and of the pixel stages (the uninterpolated read, the interpolation corners, the confidence, the SDF
 * gradient) goes through the resolution.  Nothing but the view's own buffers is written: hash, VBA, swap state, flags,
 * stored blocks and counters stay bit-identical.  Without stored data -- a context without swapping, where the
 * reading is accepted and runs the resident kernels, or a swapping one before its first eviction -- the whole
 * reading equals the resident one byte for byte in every view buffer.
 *
 * Every call flushes a pending per-call frame, runs on the context stream after the caller's work on the
 * default stream, and returns when done.  View memory is the context's: tf_destroy releases the views still alive
 * (their handles are dead afterwards), tf_view_destroy releases one early.  tf_reset, the scene / map loads and
 * tf_map_load_resized leave a view valid: it keeps nothing of the map between calls but what its last
 * tf_view_find_visible wrote, and tf_view_render rebuilds that every time. */
typedef struct tf_view tf_view;
typedef struct tf_view_params {
    int cols, rows;             /* positive multiples of 4 as tf_create demands, independent of the context's */
    int vis_capacity;           /* 0: n_buckets + n_excess */
    int max_render_blocks;      /* 0: the context's */
} tf_view_params;
tf_status tf_view_create(tf_ctx* ctx, const tf_view_params* params, tf_view** out);
void      tf_view_destroy(tf_view* view);
tf_status tf_view_get_params(tf_view* view, tf_view_params* params);    /* with the zeros resolved */
typedef enum tf_view_reading {
    TF_VIEW_RESIDENT = 0,       /* the VBA's blocks (the default) */
    TF_VIEW_WHOLE = 1           /* the VBA's and the GlobalCache's */
} tf_view_reading;
/* the reading of every later call on the view; any other value: TF_INVALID_ARG.  tf_view_params keeps its layout.
 * (Named beside the tf_view_* family, not in it: that family is the eleven calls above, and its list is pinned by
 * tests/test_view_host.py.) */
tf_status tf_set_view_reading(tf_view* view, int reading);
tf_status tf_get_view_reading(tf_view* view, int* reading);
/* FindVisibleBlocks; pose world -> camera; intr NULL: the context's.  *n_visible = entries found (may be NULL) */
tf_status tf_view_find_visible(tf_view* view, const float intr[4], const float pose_rt[12], int* n_visible);
/* CreateExpectedDepths over the view's list into the view's range image; pose world -> camera */
tf_status tf_view_expected_depths(tf_view* view, const float intr[4], const float pose_rt[12]);
/* castRay<false> over the view's range image into its raycast result; pose camera -> world */
tf_status tf_view_raycast(tf_view* view, const float intr[4], const float invM_rt[12]);
/* RenderImage's pixel stage (tf_render_type) on the view's raycast result into its image, and into dev_rgba
 * (device, rows step bytes apart, 0: cols * 4; may be NULL); pose camera -> world */
tf_status tf_view_shade(tf_view* view, const float intr[4], const float invM_rt[12], int type, uint8_t* dev_rgba, size_t step);
/* renderICP on the view's raycast result (no new raycast, no visibility marks) into the caller's level-0 maps
 * (device float4, steps in bytes, 0: cols * 16; either may be NULL); pose camera -> world */
tf_status tf_view_icp_maps(tf_view* view, const float intr[4], const float invM_rt[12], void* points, size_t points_step,
                           void* normals, size_t normals_step);
/* find_visible, expected_depths, raycast and shade in one call from a camera -> world pose; world -> camera is
 * the rigid inverse of it as the frame path inverts poses_.back() (topfu.cpp:281, 306).  TF_CAPACITY as above. */
tf_status tf_view_render(tf_view* view, const float intr[4], const float c2w_rt[12], int type, uint8_t* dev_rgba, size_t step);
typedef enum tf_view_buffer {
    TF_VIEW_VISIBLE_IDS = 0,  /* int[vis_capacity]; the first n_visible are the list */
    TF_VIEW_RANGE = 1,        /* float2[rows*cols] */
    TF_VIEW_RAYCAST = 2,      /* float4[rows*cols] */
    TF_VIEW_IMAGE = 3         /* uchar4[rows*cols] */
} tf_view_buffer;
tf_status tf_view_download(tf_view* view, int which, void* host, size_t bytes);
/* the last find_visible's count and the last expected_depths' tile total (noTotalBlocks) */
tf_status tf_view_stats(tf_view* view, int* n_visible, int* n_render_blocks);

/* ---- scene queries (addition; DESIGN.md §5 Scene queries) --------------------------------------------------
 * The TSDF at any point and on any plane, without a camera: per point the reference's three SDF reads
 * (RepresentationAccess.hpp: readFromSDF_float_uninterpolated, readFromSDF_float_interpolated,
 * readWithConfidenceFromSDF_float_interpolated), computeSingleNormalFromSDF and drawPixelColour, each with a fresh
 * IndexCache -- a query has no cache to carry, so a point has one value whatever stands before it in the batch.
 *
 * Coordinates.  A point is three floats in voxel units (TF_QUERY_VOXELS), as the reference's functions take them.
 * With TF_QUERY_METRES each component is first multiplied by the float32 1.0f / voxelSize (one rounding: the
 * raycast's oneOverVoxelSize).
 * Range guard.  Decided per point before any memory read, on the voxel-unit coordinates: a point is in range iff
 * all three satisfy -262136.0f <= c && c <= 262136.0f (+-32767 * 8: every voxel from -1 to +2 around it then has
 * an int16 block coordinate).  NaN fails the comparison.  An out-of-range point reads as nothing: sdf_nearest 1,
 * entry -1, sdf 1, confidence 0, normal (0, 0, 0), colour 0 0 0 0.  An in-range point gets what the reference's
 * functions compute, whatever that is in empty space.
 * Slices.  Pixel (x, y) of tf_scene_slice is the point (o_k + (float)x * u_k) + (float)y * v_k per component,
 * every operation rounded to float32 and none contracted; units and guard then apply as above.  A slice is
 * tf_scene_query on those points, byte for byte, without the points ever existing in memory.
 * Reading.  TF_VIEW_RESIDENT or TF_VIEW_WHOLE with the meaning they have for a view.  Under the whole reading
 * every voxel read goes through the resolution of its block over the VBA and the GlobalCache, and entry is the
 * first entry of the chain that resolves; colour is refused (a swapping scene has no colour plane).  On a context
 * without stored data the whole reading is byte-identical to the resident one; without use_swapping it runs the
 * resident kernels.
 * Status.  n == 0 is TF_OK with nothing written; outputs past n are never touched.  TF_INVALID_ARG: a NULL ctx,
 * NULL points with n > 0, n < 0, cols or rows <= 0, an unknown units or reading, out NULL or every output NULL,
 * colour without voxel_rgb or with TF_VIEW_WHOLE.  A context in error returns TF_HIP_ERROR.
 * Ordering.  The call flushes a pending per-call frame, runs on the context stream after the caller's work on the
 * default stream, and returns when done.  Nothing of the context is written -- no TF_BUF_* buffer, counter,
 * visType, device state field or tile order -- so a context with queries between its frames produces the frames
 * of one without, bit for bit. */
typedef enum tf_query_units { TF_QUERY_VOXELS = 0, TF_QUERY_METRES = 1 } tf_query_units;
typedef struct tf_query_out {        /* device pointers; each skipped when NULL; at least one non-NULL */
    float*   sdf_nearest;  /* [n]    readFromSDF_float_uninterpolated */
    int*     entry;        /* [n]    hash entry whose block holds the nearest voxel, -1: none (the fresh-cache vmIndex - 1) */
    float*   sdf;          /* [n]    readFromSDF_float_interpolated (== readWithConfidence...'s value) */
    float*   confidence;   /* [n]    readWithConfidenceFromSDF_float_interpolated's confidence */
    float*   normal;       /* [n][3] computeSingleNormalFromSDF, as the reference leaves it (not normalised) */
    uint8_t* colour;       /* [n][4] drawPixelColour; voxel_rgb contexts only; 4-byte aligned (stored as one word) */
} tf_query_out;
tf_status tf_scene_query(tf_ctx* ctx, const float* dev_points /* [n][3] */, long long n, int units, int reading,
                         const tf_query_out* out);
/* n = cols * rows, row-major */
tf_status tf_scene_slice(tf_ctx* ctx, const float origin[3], const float u[3], const float v[3], int cols, int rows,
                         int units, int reading, const tf_query_out* out);

#ifdef __cplusplus
}
#endif
#endif
