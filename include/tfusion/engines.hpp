// tfusion/engines.hpp -- the L4 engine API of the reference (scene, render state, reconstruction
// and visualisation engines, cuda:: image processing) for MI355X, header-only over the C-ABI of
// libtfusion_hip.so.  Mirrors:
//   Scene<TVoxel, TIndex>                   tfusion/include/tfusion/scene.hpp:13-44
//   RenderState / RenderState_VH            tfusion/include/tfusion/RenderState.hpp:12-88, RenderState_VH.hpp:15-61
//   SceneReconstructionEngine_CUDA          tfusion/include/tfusion/cuda/SceneReconstructionEngine_host.hpp:42-74
//   VisualisationEngine_CUDA                tfusion/include/tfusion/cuda/VisualisationEngine_CUDA.hpp:12-47
//   IVisualisationEngine enums              tfusion/include/tfusion/VisualisationEngine.hpp:12-40
//   cuda::{computeDists, depthBilateralFilter, depthTruncation, depthBuildPyramid,
//          computePointNormals, resizePointsNormals, waitAllDefaultStream}
//                                           tfusion/include/tfusion/cuda/imgproc.hpp:9-31
//
// One difference of structure: a Scene owns one libtfusion_hip context, which holds the scene
// (hash, voxel blocks, block grid) AND the render state the tracker works with (visible list and
// types, range image, raycast result), sized at construction: the image size and the capacities
// come from the TopFuParams the Scene is given (defaults: the reference's default_params,
// VoxelBlockHash.hpp:10-27).  The engines take that state when they are given no RenderState
// (nullptr) or one that was never bound.
//
// A RenderState / RenderState_VH passed to VisualisationEngine_CUDA::FindVisibleBlocks becomes a
// render state of its own: on first use it binds a free view (tf_view, include/tfusion_hip.h) of
// its imgSize on that scene's context -- its own visible list, range image, raycast result and
// image -- and releases it in its destructor.  CreateExpectedDepths, RenderImage and CreateICPMaps
// given a bound render state work on that view and size their outputs by it, and leave the
// scene's own render state (the tracker's) untouched.  A bound render state is destroyed before
// its scene (the scene's destructor releases the views still bound to it).
#pragma once
#include "../tfusion_hip.h"
#include "topfu.hpp"
#include "types.hpp"

#include <stdexcept>
#include <string>

namespace tfusion
{
    inline void tf_engine_check(tf_status s, const char* what)
    {
        if (s != TF_OK) throw std::runtime_error(std::string(what) + ": " + tf_status_string(s));
    }

    // voxel / index type tags (VoxelTypes.hpp:69-92, VoxelBlockHash.hpp:53-122)
    struct Voxel_s {
        short sdf;
        unsigned char w_depth;
        unsigned char pad;
        static short SDF_initialValue() { return 32767; }
        static float valueToFloat(float x) { return x / 32767.0f; }
        static short floatToValue(float x) { return (short)(x * 32767.0f); }
        static const bool hasColorInformation = false;
    };
    // Voxel_s_rgb (VoxelTypes.hpp:39-67): the context keeps its colour half (clr, w_color) as a
    // second plane (TF_BUF_VBA_RGB); this struct is the combined view a caller assembles
    struct Voxel_s_rgb {
        short sdf;
        unsigned char w_depth;
        Vector3u clr;
        unsigned char w_color;
        static short SDF_initialValue() { return 32767; }
        static float valueToFloat(float x) { return x / 32767.0f; }
        static short floatToValue(float x) { return (short)(x * 32767.0f); }
        static const bool hasColorInformation = true;
    };
    struct VoxelBlockHash {
        enum { noTotalEntries = 0x100000 + 0x20000 };   // SDF_BUCKET_NUM + SDF_EXCESS_LIST_SIZE (defaults)
    };

    // IVisualisationEngine::RenderImageType / RenderRaycastSelection (VisualisationEngine.hpp:15-27)
    struct IVisualisationEngine {
        enum RenderImageType {
            RENDER_SHADED_GREYSCALE = TF_RENDER_SHADED_GREYSCALE,
            RENDER_SHADED_GREYSCALE_IMAGENORMALS = TF_RENDER_SHADED_GREYSCALE_IMAGENORMALS,
            RENDER_COLOUR_FROM_VOLUME = TF_RENDER_COLOUR_FROM_VOLUME,
            RENDER_COLOUR_FROM_NORMAL = TF_RENDER_COLOUR_FROM_NORMAL,
            RENDER_COLOUR_FROM_CONFIDENCE = TF_RENDER_COLOUR_FROM_CONFIDENCE
        };
        enum RenderRaycastSelection { RENDER_FROM_NEW_RAYCAST, RENDER_FROM_OLD_RAYCAST, RENDER_FROM_OLD_FORWARDPROJ };
    };

    // HashSwapState (GlobalCache.hpp:11-20): 0 data on the host side only, 1 in both (not yet
    // combined), 2 most recent in active memory
    struct HashSwapState { unsigned char state; };

    // GlobalCache<TVoxel> (GlobalCache.hpp:22-134): a view of the scene context's cache, which
    // lives in HBM next to the active voxel blocks, not in host memory;
    // the accessors copy out.  The transfer buffers of the reference (synced blocks, needed ids)
    // have no counterpart: a transfer is a device-side copy.
    template <class TVoxel>
    class GlobalCache
    {
    public:
        int noTotalEntries;

        explicit GlobalCache(tf_ctx* ctx) : noTotalEntries(0), ctx_(ctx)
        {
            tf_params p;
            tf_engine_check(tf_get_params(ctx, &p), "GlobalCache: tf_get_params");
            noTotalEntries = p.n_buckets + p.n_excess;
        }
        bool HasStoredData(int address) const { return byte_at(TF_BUF_SWAP_STORED_FLAGS, address) != 0; }
        // the stored block of an entry (SDF_BLOCK_SIZE3 voxels) copied into `out`
        void GetStoredVoxelBlock(int address, TVoxel* out) const
        {
            size_t n = 0;
            tf_engine_check(tf_buffer_bytes(ctx_, TF_BUF_SWAP_STORED, 0, &n), "tf_buffer_bytes");
            const size_t blk = sizeof(TVoxel) * 512;
            if (address < 0 || address >= noTotalEntries) throw std::out_of_range("GetStoredVoxelBlock");
            tf_engine_check(tf_download_range(ctx_, TF_BUF_SWAP_STORED, (size_t)address * blk, out, blk),
                            "GetStoredVoxelBlock");
        }
        HashSwapState GetSwapState(int address) const { return HashSwapState{ byte_at(TF_BUF_SWAP_STATE, address) }; }
        void SaveToFile(const char* fileName) const { tf_engine_check(tf_swap_save(ctx_, fileName), "SaveToFile"); }
        void ReadFromFile(const char* fileName) { tf_engine_check(tf_swap_load(ctx_, fileName), "ReadFromFile"); }

    private:
        unsigned char byte_at(int which, int address) const
        {
            if (address < 0 || address >= noTotalEntries) throw std::out_of_range("GlobalCache entry");
            unsigned char b = 0;
            tf_engine_check(tf_download_range(ctx_, which, (size_t)address, &b, 1), "GlobalCache");
            return b;
        }
        tf_ctx* ctx_;
    };

    // Scene<TVoxel, TIndex> (scene.hpp:13-44): owns the context
    template <class TVoxel, class TIndex>
    class Scene
    {
    public:
        const SceneParams* sceneParams;
        GlobalCache<TVoxel>* globalCache = nullptr;     // scene.hpp:27, set when useSwapping

        // scene.hpp:29-34; `frame` (an addition, defaulted) gives the image size, intrinsics and
        // capacities the context is created with; useSwapping sets tf_params::use_swapping
        Scene(const SceneParams* params, bool useSwapping, const TopFuParams& frame = TopFuParams::default_params())
            : sceneParams(params)
        {
            TopFuParams tp = frame;
            tf_params c = tp.to_c();
            if (params) {
                c.mu = params->mu; c.maxW = params->maxW; c.voxelSize = params->voxelSize;
                c.viewFrustum_min = params->viewFrustum_min; c.viewFrustum_max = params->viewFrustum_max;
            }
            c.use_swapping = useSwapping ? 1 : 0;
            c.voxel_rgb = TVoxel::hasColorInformation ? 1 : 0;    // Scene<Voxel_s_rgb, ...>
            tf_engine_check(tf_create(&c, &ctx_), "Scene: tf_create");
            intr_ = tp.intr;
            if (useSwapping) globalCache = new GlobalCache<TVoxel>(ctx_);
        }
        ~Scene()
        {
            delete globalCache;
            tf_destroy(ctx_);
        }
        Scene(const Scene&) = delete;
        Scene& operator=(const Scene&) = delete;

        tf_ctx* context() const { return ctx_; }
        const Intr& intr() const { return intr_; }
        // LocalVBA::lastFreeBlockId, VoxelBlockHash::lastFreeExcessListId, RenderState_VH::noVisibleEntries
        tf_stats counters() const
        {
            tf_stats s;
            tf_engine_check(tf_get_stats(ctx_, &s), "tf_get_stats");
            return s;
        }

        // Mesh extraction over the scene's context (additions, as TopFu::extractMesh / saveMesh; the class a
        // swapping caller holds, so this is where the whole map leaves the device).  flags: 0 = the resident
        // blocks, TF_MESH_WHOLE = every block of either tier (tf_mesh_extract_whole).  Triangles as 9 floats
        // each, resized to fit, normals (9 floats per triangle) beside them when the pointer is not null;
        // returns the triangle count.
        long long extractMesh(cuda::DeviceArray<float>& triangles, cuda::DeviceArray<float>* normals = nullptr, int flags = 0)
        {
            if (flags & ~TF_MESH_WHOLE) tf_engine_check(TF_INVALID_ARG, "Scene::extractMesh");
            const bool whole = (flags & TF_MESH_WHOLE) != 0;
            auto call = [&](float* t, float* n, long long cap, long long* count) {
                return whole ? tf_mesh_extract_whole(ctx_, t, n, cap, count) : tf_mesh_extract_attr(ctx_, t, n, nullptr, cap, count);
            };
            long long n = 0, m = 0;
            tf_engine_check(call(nullptr, nullptr, 0, &n), "Scene::extractMesh");
            triangles.create((size_t)n * 9);
            if (normals) normals->create((size_t)n * 9);
            if (n > 0) tf_engine_check(call(triangles.ptr(), normals ? normals->ptr() : nullptr, n, &m), "Scene::extractMesh");
            return n;
        }
        // the mesh as a binary PLY with welded vertices; attrs = TF_MESH_NORMALS and / or TF_MESH_WHOLE (the
        // whole mesh is downloaded and welded in one piece: the host's memory bounds it), TF_MESH_COLOURS on a
        // Voxel_s_rgb scene, TF_MESH_INDEXED for the resident vertex table as it leaves the GPU
        void saveMesh(const std::string& path, int attrs = 0)
        {
            if (attrs & TF_MESH_INDEXED) tf_engine_check(tf_mesh_save_ply_indexed(ctx_, path.c_str(), attrs), "tf_mesh_save_ply_indexed");
            else tf_engine_check(tf_mesh_save_ply_attr(ctx_, path.c_str(), attrs), "tf_mesh_save_ply_attr");
        }
        // The mesh with shared vertices: 3 floats per vertex, 3 vertex numbers per triangle (extractMesh's
        // triangles in its order), 3 normal floats per vertex when the pointer is not null; all resized to fit.
        // flags: 0 = the resident blocks (tf_mesh_extract_indexed), TF_MESH_WHOLE = every block of either tier
        // (tf_mesh_extract_indexed_whole).  Returns the triangle count; vertices.size() / 3 is the vertex count.
        long long extractMeshIndexed(cuda::DeviceArray<float>& vertices, cuda::DeviceArray<unsigned>& indices,
                                     cuda::DeviceArray<float>* normals = nullptr, int flags = 0)
        {
            if (flags & ~TF_MESH_WHOLE) tf_engine_check(TF_INVALID_ARG, "Scene::extractMeshIndexed");
            const bool whole = (flags & TF_MESH_WHOLE) != 0;
            auto call = [&](float* v, float* n, long long vcap, unsigned* i, long long tcap, long long* nv, long long* nt) {
                return whole ? tf_mesh_extract_indexed_whole(ctx_, v, n, vcap, i, tcap, nv, nt)
                             : tf_mesh_extract_indexed(ctx_, v, n, nullptr, vcap, i, tcap, nv, nt);
            };
            long long nv = 0, nt = 0, mv = 0, mt = 0;
            tf_engine_check(call(nullptr, nullptr, 0, nullptr, 0, &nv, &nt), "Scene::extractMeshIndexed");
            vertices.create((size_t)nv * 3);
            indices.create((size_t)nt * 3);
            if (normals) normals->create((size_t)nv * 3);
            if (nt > 0)
                tf_engine_check(call(vertices.ptr(), normals ? normals->ptr() : nullptr, nv, indices.ptr(), nt, &mv, &mt), "Scene::extractMeshIndexed");
            return nt;
        }
        // the whole map's indexed mesh as a binary PLY, written in bounded pieces (tf_mesh_save_ply_indexed_whole):
        // attrs = 0 or TF_MESH_NORMALS; the host holds one chunk, whatever the map
        void saveMeshIndexedWhole(const std::string& path, int attrs = 0)
        {
            tf_engine_check(tf_mesh_save_ply_indexed_whole(ctx_, path.c_str(), attrs), "tf_mesh_save_ply_indexed_whole");
        }

        // Scene queries (additions: tf_scene_query / tf_scene_slice): the TSDF at n device points (3 floats each,
        // in voxel units or metres) or on the cols x rows pixels of the plane origin + x * u + y * v -- per point
        // the nearest and the interpolated SDF, the confidence, the entry of the nearest voxel's block, the SDF
        // gradient and (Voxel_s_rgb scenes, never with whole) the colour, each into the device array of `out` that
        // is not null.  whole: both tiers of a swapping scene.  Nothing of the scene is written.
        void query(const float* points, long long n, tf_query_units units, bool whole, const tf_query_out& out)
        {
            tf_engine_check(tf_scene_query(ctx_, points, n, (int)units, whole ? TF_VIEW_WHOLE : TF_VIEW_RESIDENT, &out), "tf_scene_query");
        }
        void slice(const float origin[3], const float u[3], const float v[3], int cols, int rows, tf_query_units units, bool whole,
                   const tf_query_out& out)
        {
            tf_engine_check(tf_scene_slice(ctx_, origin, u, v, cols, rows, (int)units, whole ? TF_VIEW_WHOLE : TF_VIEW_RESIDENT, &out),
                            "tf_scene_slice");
        }

        // Map checkpoints (additions: tf_map_save / tf_map_load).  saveMap writes the state the scene resumes
        // from, sized by what is live: of a swapping scene both tiers -- the hash, the active blocks, the
        // GlobalCache's swap states, stored flags and stored blocks, the lists and counters (version 2 of the
        // checkpoint file); of a scene without swapping the scene checkpoint (version 1).  loadMap replaces this
        // scene's state by the file's: a scene with the file's capacities, image size, scene parameters and
        // useSwapping is from then on the one that saved, bit for bit, through any further engine calls.
        void saveMap(const std::string& path) { tf_engine_check(tf_map_save(ctx_, path.c_str()), "tf_map_save"); }
        void loadMap(const std::string& path) { tf_engine_check(tf_map_load(ctx_, path.c_str()), "tf_map_load"); }
        // Resized load (addition: tf_map_load_resized): a file saved with other table sizes into this scene -- the
        // records with a block position are re-hashed as if inserted one by one into a reset table, the others
        // dropped.  Throws with TF_CAPACITY when the map does not fit (report, when given, says what it needs);
        // the scene is then as it was.
        void loadMapResized(const std::string& path, struct tf_resize_report* report = nullptr)
        {
            tf_engine_check(tf_map_load_resized(ctx_, path.c_str(), report), "tf_map_load_resized");
        }
        // Map merge (addition: tf_map_merge): a version-1 checkpoint fused into this scene, which must be one
        // without swapping; its block positions are moved by `offset` whole blocks.  A position the scene holds
        // with a block is combined voxel by voxel (CombineVoxelInformation), a new one is inserted by the
        // allocation rule.  Throws with TF_CAPACITY when the free lists are too short (report, when given, says
        // what is needed); the scene is then as it was.
        void mergeMap(const std::string& path, const std::array<int, 3>& offset = { 0, 0, 0 }, struct tf_merge_report* report = nullptr)
        {
            tf_engine_check(tf_map_merge(ctx_, path.c_str(), offset.data(), report), "tf_map_merge");
        }

    private:
        tf_ctx* ctx_ = nullptr;
        Intr intr_;
    };

    // RenderState (RenderState.hpp:12-88) / RenderState_VH (RenderState_VH.hpp:15-61): unbound, a handle
    // for the scene's own render state; bound by FindVisibleBlocks, a free view of imgSize (see the
    // header comment)
    class RenderState
    {
    public:
        RenderState(const Vector2i& imgSize, float vf_min, float vf_max) : imgSize_(imgSize), vf_min_(vf_min), vf_max_(vf_max) {}
        virtual ~RenderState() { tf_view_destroy(view_); }
        RenderState(const RenderState&) = delete;
        RenderState& operator=(const RenderState&) = delete;
        const Vector2i& imgSize() const { return imgSize_; }
        // the free view this state is bound to (nullptr: never bound)
        tf_view* view() const { return view_; }
        // the reading of a bound state (an addition: tf_set_view_reading): on a swapping scene FindVisibleBlocks,
        // CreateExpectedDepths, RenderImage and CreateICPMaps given this state then see the blocks held in the
        // GlobalCache as well as the resident ones.  Kept across a re-binding; no effect on an unbound state.
        void setWhole(bool whole)
        {
            whole_ = whole;
            if (view_) tf_engine_check(tf_set_view_reading(view_, whole_ ? TF_VIEW_WHOLE : TF_VIEW_RESIDENT), "RenderState: tf_set_view_reading");
        }
        bool whole() const { return whole_; }
        // binds a view of imgSize on `ctx` (the first use; again when given another scene's context)
        tf_view* bind(tf_ctx* ctx)
        {
            if (view_ && ctx_ == ctx) return view_;
            tf_view_destroy(view_);
            view_ = nullptr;
            const tf_view_params vp = { imgSize_.x, imgSize_.y, 0, 0 };
            tf_engine_check(tf_view_create(ctx, &vp, &view_), "RenderState: tf_view_create");
            tf_engine_check(tf_set_view_reading(view_, whole_ ? TF_VIEW_WHOLE : TF_VIEW_RESIDENT), "RenderState: tf_set_view_reading");
            ctx_ = ctx;
            return view_;
        }
    private:
        Vector2i imgSize_;
        float vf_min_, vf_max_;
        tf_view* view_ = nullptr;
        tf_ctx* ctx_ = nullptr;
        bool whole_ = false;
    };
    class RenderState_VH : public RenderState
    {
    public:
        RenderState_VH(int noTotalEntries, const Vector2i& imgSize, float vf_min, float vf_max)
            : RenderState(imgSize, vf_min, vf_max), noTotalEntries_(noTotalEntries) {}
    private:
        int noTotalEntries_;
    };

    namespace detail
    {
        inline void intr4(const Intr& i, float out[4]) { out[0] = i.fx; out[1] = i.fy; out[2] = i.cx; out[3] = i.cy; }
        inline void rt_of(const Affine3f& a, float rt[12]) { affine_to_rt(a, rt); }
        inline void rt_of(const Matrix4f& m, float rt[12]) { m.toRt(rt); }
    }

    // SceneReconstructionEngine_CUDA<TVoxel, TIndex> (SceneReconstructionEngine_host.hpp:42-74)
    template <class TVoxel, class TIndex>
    class SceneReconstructionEngine_CUDA
    {
    public:
        // ResetScene (SceneReconstructionEngine_host.cu:51-73)
        void ResetScene(Scene<TVoxel, TIndex>* scene)
        {
            tf_engine_check(tf_stage_reset_scene(scene->context()), "ResetScene");
        }
        // AllocateSceneFromDepth (:75-195); pose is world -> camera, as TopFu passes it
        void AllocateSceneFromDepth(Scene<TVoxel, TIndex>* scene, const Intr intr, const Affine3f pose, cuda::Dists& dist,
                                    const RenderState* = nullptr, bool onlyUpdateVisibleList = false,
                                    bool resetVisibleList = false)
        {
            float in[4], rt[12];
            detail::intr4(intr, in);
            detail::rt_of(pose, rt);
            tf_engine_check(tf_scene_alloc(scene->context(), in, rt, dist.ptr(), dist.step(), onlyUpdateVisibleList ? 1 : 0,
                                           resetVisibleList ? 1 : 0), "AllocateSceneFromDepth");
        }
        // IntegrateIntoScene (:197-251)
        void IntegrateIntoScene(Scene<TVoxel, TIndex>* scene, const Intr intr, const Affine3f pose, cuda::Dists& dist,
                                const RenderState* = nullptr)
        {
            float in[4], rt[12];
            detail::intr4(intr, in);
            detail::rt_of(pose, rt);
            tf_engine_check(tf_scene_integrate(scene->context(), in, rt, dist.ptr(), dist.step()), "IntegrateIntoScene");
        }
        // with the view's RGBA image (view->rgb, :225): the colour update of a Voxel_s_rgb scene
        void IntegrateIntoScene(Scene<TVoxel, TIndex>* scene, const Intr intr, const Affine3f pose, cuda::Dists& dist,
                                const cuda::image4u& rgb, const RenderState* = nullptr)
        {
            float in[4], rt[12];
            detail::intr4(intr, in);
            detail::rt_of(pose, rt);
            tf_engine_check(tf_scene_integrate_rgb(scene->context(), in, rt, dist.ptr(), dist.step(),
                                                   reinterpret_cast<const uint8_t*>(rgb.ptr()), rgb.step()),
                            "IntegrateIntoScene(rgb)");
        }
    };

    // SwappingEngine_CUDA<TVoxel, TIndex>: the engine of the GlobalCache's lineage (InfiniTAM
    // ITMSwappingEngine_CUDA; its instantiation is commented out in the reference,
    // CUDAInstantiations.cu:8), called after IntegrateIntoScene on a swapping scene
    template <class TVoxel, class TIndex>
    class SwappingEngine_CUDA
    {
    public:
        // stored blocks of the entries marked "needed" (state 1) merged into their active blocks
        void IntegrateGlobalIntoLocal(Scene<TVoxel, TIndex>* scene, RenderState* = nullptr)
        {
            tf_engine_check(tf_scene_swap_in(scene->context()), "IntegrateGlobalIntoLocal");
        }
        // active blocks not visible this frame moved to the cache, their VBA blocks freed
        void SaveToGlobalMemory(Scene<TVoxel, TIndex>* scene, RenderState* = nullptr)
        {
            tf_engine_check(tf_scene_swap_out(scene->context()), "SaveToGlobalMemory");
        }
    };

    // VisualisationEngine_CUDA<TVoxel, TIndex> (VisualisationEngine_CUDA.hpp:12-47)
    template <class TVoxel, class TIndex>
    class VisualisationEngine_CUDA
    {
    public:
        // FindVisibleBlocks (the reference's declaration is commented out, VisualisationEngine_CUDA.cu:43-73; its
        // kernel buildCompleteVisibleList_device is live): every allocated block of the scene that projects into
        // renderState's image from `pose` (world -> camera), in ascending entry order, into renderState's own
        // visible list.  Binds renderState to a free view of its imgSize on first use.  Returns the count; throws
        // with TF_CAPACITY's text when the list is too short.  On a swapping scene: the resident blocks only.
        int FindVisibleBlocks(const Scene<TVoxel, TIndex>* scene, const Matrix4f pose, const Vector4f intrinsics,
                              RenderState* renderState) const
        {
            if (!renderState) throw std::invalid_argument("FindVisibleBlocks: a RenderState is needed");
            const float in[4] = { intrinsics.x, intrinsics.y, intrinsics.z, intrinsics.w };
            float rt[12];
            detail::rt_of(pose, rt);
            int n = 0;
            tf_engine_check(tf_view_find_visible(renderState->bind(scene->context()), in, rt, &n), "FindVisibleBlocks");
            return n;
        }
        // CreateExpectedDepths (VisualisationEngine_CUDA.cu:119-173); pose is world -> camera
        void CreateExpectedDepths(const Scene<TVoxel, TIndex>* scene, const Affine3f pose, const Intr intrinsics,
                                  RenderState* renderState = nullptr) const
        {
            float in[4], rt[12];
            detail::intr4(intrinsics, in);
            detail::rt_of(pose, rt);
            if (renderState && renderState->view())
                tf_engine_check(tf_view_expected_depths(renderState->view(), in, rt), "CreateExpectedDepths (view)");
            else
                tf_engine_check(tf_vis_expected_depths(scene->context(), in, rt), "CreateExpectedDepths");
        }
        // RenderImage (:220-291, 423-429); pose is camera -> world (TopFu's Matrix4f(poses_.back()))
        void RenderImage(const Scene<TVoxel, TIndex>* scene, Matrix4f pose, const Vector4f intrinsics, RenderState* renderState,
                         cuda::image4u& outputImage,
                         IVisualisationEngine::RenderImageType type = IVisualisationEngine::RENDER_SHADED_GREYSCALE,
                         IVisualisationEngine::RenderRaycastSelection raycastType =
                             IVisualisationEngine::RENDER_FROM_NEW_RAYCAST) const
        {
            if (raycastType == IVisualisationEngine::RENDER_FROM_OLD_FORWARDPROJ)
                throw std::invalid_argument("RenderImage: RENDER_FROM_OLD_FORWARDPROJ is not on this path");
            float in[4] = { intrinsics.x, intrinsics.y, intrinsics.z, intrinsics.w }, rt[12];
            detail::rt_of(pose, rt);
            if (renderState && renderState->view()) {      // a bound render state: its own raycast result and size
                tf_view* v = renderState->view();
                outputImage.create(renderState->imgSize().y, renderState->imgSize().x);
                if (raycastType == IVisualisationEngine::RENDER_FROM_NEW_RAYCAST)
                    tf_engine_check(tf_view_raycast(v, in, rt), "RenderImage (view raycast)");
                tf_engine_check(tf_view_shade(v, in, rt, (int)type, reinterpret_cast<uint8_t*>(outputImage.ptr()),
                                              outputImage.step()), "RenderImage (view)");
                return;
            }
            tf_params p;
            tf_engine_check(tf_get_params(scene->context(), &p), "tf_get_params");
            outputImage.create(p.rows, p.cols);
            tf_engine_check(tf_vis_render_image(scene->context(), in, rt, (int)type,
                                                raycastType == IVisualisationEngine::RENDER_FROM_NEW_RAYCAST ? 1 : 0,
                                                reinterpret_cast<uint8_t*>(outputImage.ptr()), outputImage.step()),
                            "RenderImage");
        }
        // CreateICPMaps (:473-493 -> 323-360); pose is camera -> world
        // (a bound render state has no visibility types to mark: its raycast is castRay<false>)
        void CreateICPMaps(const Scene<TVoxel, TIndex>* scene, const Matrix4f pose, const Intr intr, cuda::Cloud& points,
                           cuda::Normals& normals, RenderState* renderState = nullptr) const
        {
            float in[4], rt[12];
            detail::intr4(intr, in);
            detail::rt_of(pose, rt);
            if (renderState && renderState->view()) {
                tf_view* v = renderState->view();
                points.create(renderState->imgSize().y, renderState->imgSize().x);
                normals.create(renderState->imgSize().y, renderState->imgSize().x);
                tf_engine_check(tf_view_raycast(v, in, rt), "CreateICPMaps (view raycast)");
                tf_engine_check(tf_view_icp_maps(v, in, rt, points.ptr(), points.step(), normals.ptr(), normals.step()),
                                "CreateICPMaps (view)");
                return;
            }
            tf_params p;
            tf_engine_check(tf_get_params(scene->context(), &p), "tf_get_params");
            points.create(p.rows, p.cols);
            normals.create(p.rows, p.cols);
            tf_engine_check(tf_vis_icp_maps(scene->context(), in, rt, points.ptr(), points.step(), normals.ptr(),
                                            normals.step()), "CreateICPMaps");
        }
    };

    // cuda:: image processing (imgproc.hpp:9-31) on the legacy default stream
    namespace cuda
    {
        // computeDists (imgproc.cpp:44-48): mm -> m, >= 2047 mm or 0 -> -1
        inline void computeDists(const Depth& depth, Dists& dists, const Intr&)
        {
            dists.create(depth.rows(), depth.cols());
            tf_engine_check(tf_imgproc_compute_dists(depth.ptr(), depth.step(), dists.ptr(), dists.step(), depth.cols(),
                                                     depth.rows(), nullptr), "computeDists");
        }
        // depthBilateralFilter (imgproc.cpp:3-7); sigma_depth in metres
        inline void depthBilateralFilter(const Depth& in, Depth& out, int ksz, float sigma_spatial, float sigma_depth)
        {
            out.create(in.rows(), in.cols());
            tf_engine_check(tf_imgproc_bilateral(in.ptr(), in.step(), out.ptr(), out.step(), in.cols(), in.rows(), ksz,
                                                 sigma_spatial, sigma_depth, nullptr), "depthBilateralFilter");
        }
        // depthTruncation (imgproc.cpp:9-10); threshold in metres
        inline void depthTruncation(Depth& depth, float threshold)
        {
            tf_engine_check(tf_imgproc_truncate(depth.ptr(), depth.step(), depth.cols(), depth.rows(), threshold, nullptr),
                            "depthTruncation");
        }
        // depthBuildPyramid (imgproc.cpp:12-16)
        inline void depthBuildPyramid(const Depth& depth, Depth& pyramid, float sigma_depth)
        {
            pyramid.create(depth.rows() / 2, depth.cols() / 2);
            tf_engine_check(tf_imgproc_pyr_down(depth.ptr(), depth.step(), depth.cols(), depth.rows(), pyramid.ptr(),
                                                pyramid.step(), sigma_depth, nullptr), "depthBuildPyramid");
        }
        // computePointNormals (imgproc.cpp:31-41)
        inline void computePointNormals(const Intr& intr, const Depth& depth, Cloud& points, Normals& normals)
        {
            points.create(depth.rows(), depth.cols());
            normals.create(depth.rows(), depth.cols());
            const float in[4] = { intr.fx, intr.fy, intr.cx, intr.cy };
            tf_engine_check(tf_imgproc_point_normals(in, depth.ptr(), depth.step(), depth.cols(), depth.rows(), points.ptr(),
                                                     points.step(), normals.ptr(), normals.step(), nullptr),
                            "computePointNormals");
        }
        // resizePointsNormals (imgproc.cpp:64-73)
        inline void resizePointsNormals(const Cloud& points, const Normals& normals, Cloud& points_out, Normals& normals_out)
        {
            points_out.create(points.rows() / 2, points.cols() / 2);
            normals_out.create(normals.rows() / 2, normals.cols() / 2);
            tf_engine_check(tf_imgproc_resize_points_normals(points.ptr(), points.step(), normals.ptr(), normals.step(),
                                                             points.cols(), points.rows(), points_out.ptr(),
                                                             points_out.step(), normals_out.ptr(), normals_out.step(),
                                                             nullptr), "resizePointsNormals");
        }
        // waitAllDefaultStream (imgproc.cpp:18-19)
        inline void waitAllDefaultStream() { tf_engine_check(tf_imgproc_sync(nullptr), "waitAllDefaultStream"); }
    }
}
