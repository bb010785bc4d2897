// tfusion/topfu.hpp -- the tfusion pipeline API (TopFuParams, TopFu) for MI355X, header-only
// over the C-ABI of libtfusion_hip.so (include/tfusion_hip.h).
//
// Drop-in for tfusion/include/tfusion/topfu.hpp:17-110 as used by apps/demo.cpp:27-38,100-115,
// 141-168: TopFuParams::default_params, TopFu(params), operator()(Depth), renderImage(image4u&),
// getCameraPose(time), reset(), params(), icp(); cuda::{setDevice, getCudaEnabledDeviceCount,
// getDeviceName, checkIfPreFermiGPU, printShortCudaDeviceInfo, printCudaDeviceInfo}.
// Behaviour mirrored from topfu.cpp: frame 0 integrates only; later frames track and return
// false after an ICP failure, which resets the pipeline (poses_ back to {Identity},
// topfu.cpp:141-152, 263-264); getCameraPose(time) indexes the pose history (:154-159).
// Errors: a HIP failure throws std::runtime_error (the reference exits, device_memory.cpp:7-11).
#pragma once
#include "../tfusion_hip.h"
#include "types.hpp"
#include "cuda/projective_icp.hpp"

#include <array>
#include <memory>

namespace tfusion
{
    namespace cuda
    {
        inline int getCudaEnabledDeviceCount()
        {
            int n = 0;
            return tf_device_count(&n) == TF_OK ? n : 0;
        }
        inline void setDevice(int device)
        {
            if (tf_set_device(device) != TF_OK) throw std::runtime_error("tfusion::cuda::setDevice failed");
        }
        inline std::string getDeviceName(int device)
        {
            hipDeviceProp_t p;
            hip_check(hipGetDeviceProperties(&p, device), "hipGetDeviceProperties");
            return p.name;
        }
        inline bool checkIfPreFermiGPU(int) { return false; }   // no such GPUs on this path
        inline void printShortCudaDeviceInfo(int device)
        {
            hipDeviceProp_t p;
            hip_check(hipGetDeviceProperties(&p, device), "hipGetDeviceProperties");
            std::printf("Device %d: \"%s\" %s, %d CUs, %.0f GB\n", device, p.name, p.gcnArchName, p.multiProcessorCount,
                        p.totalGlobalMem / 1e9);
        }
        inline void printCudaDeviceInfo(int device) { printShortCudaDeviceInfo(device); }
    }

    // SceneParams (SceneParams.hpp:9-63)
    struct SceneParams {
        float voxelSize, viewFrustum_min, viewFrustum_max, mu;
        int maxW;
        bool stopIntegratingAtMaxW;
        SceneParams() : voxelSize(0.005f), viewFrustum_min(0.2f), viewFrustum_max(3.0f), mu(0.02f), maxW(100),
                        stopIntegratingAtMaxW(false) {}
        SceneParams(float mu_, int maxW_, float voxelSize_, float vmin, float vmax, bool stop)
            : voxelSize(voxelSize_), viewFrustum_min(vmin), viewFrustum_max(vmax), mu(mu_), maxW(maxW_),
              stopIntegratingAtMaxW(stop) {}
    };

    // TopFuParams (topfu.hpp:28-60).  Fields the hot path does not read (volume_*, tsdf_*,
    // raycast_step_factor, gradient_delta_factor, light_pose) are kept for source compatibility.
    // The capacities (hash buckets / excess / blocks / visible list / render blocks) are MI355X
    // additions with the reference's values as defaults (VoxelBlockHash.hpp:10-27).
    struct TopFuParams {
        static TopFuParams default_params()   // topfu.cpp:12-53
        {
            TopFuParams p;
            p.cols = 640; p.rows = 480;
            p.intr = Intr(504.261f, 503.905f, 352.457f, 272.202f);
            p.volume_dims = Vec3i::all(512);
            p.volume_size = Vec3f::all(3.f);
            p.volume_pose = Affine3f().translate(Vec3f(-1.5f, -1.5f, 0.5f));
            p.bilateral_sigma_depth = 0.04f;
            p.bilateral_sigma_spatial = 4.5f;
            p.bilateral_kernel_size = 7;
            p.icp_truncate_depth_dist = 2.0f;
            p.icp_dist_thres = 0.1f;
            p.icp_angle_thres = deg2rad(30.f);
            p.icp_iter_num = { 10, 5, 4, 0 };
            p.tsdf_min_camera_movement = 0.f;
            p.tsdf_trunc_dist = 0.04f;
            p.tsdf_max_weight = 64;
            p.raycast_step_factor = 0.75f;
            p.gradient_delta_factor = 0.5f;
            p.light_pose = Vec3f::all(0.f);
            p.sceneParams = std::make_shared<SceneParams>(0.02f, 100, 0.005f, 0.2f, 3.0f, false);
            tf_params d;
            tf_default_params(&d);
            p.n_buckets = d.n_buckets; p.n_excess = d.n_excess; p.n_blocks = d.n_blocks;
            p.vis_capacity = d.vis_capacity; p.max_render_blocks = d.max_render_blocks;
            p.integrate_colour = false;
            p.rgb_intr = Intr(0.f, 0.f, 0.f, 0.f);
            p.depth_to_rgb = Affine3f::Identity();
            return p;
        }

        int cols, rows;
        Intr intr;
        Vec3i volume_dims;
        Vec3f volume_size;
        Affine3f volume_pose;
        float bilateral_sigma_depth, bilateral_sigma_spatial;
        int bilateral_kernel_size;
        float icp_truncate_depth_dist, icp_dist_thres, icp_angle_thres;
        std::vector<int> icp_iter_num;
        float tsdf_min_camera_movement, tsdf_trunc_dist;
        int tsdf_max_weight;
        float raycast_step_factor, gradient_delta_factor;
        Vec3f light_pose;
        std::shared_ptr<SceneParams> sceneParams;   // the reference leaks a raw pointer (topfu.cpp:50)
        int n_buckets, n_excess, n_blocks, vis_capacity, max_render_blocks;
        // colour (an addition): Voxel_s_rgb voxels, the RGB image of operator()(depth, rgba)
        // integrated (VoxelTypes.hpp:39-67, SceneReconstructionEngine.hpp:116-148); rgb_intr all 0
        // = the depth intrinsics; depth_to_rgb = trafo_rgb_to_depth.calib_inv (identity: registered)
        bool integrate_colour;
        Intr rgb_intr;
        Affine3f depth_to_rgb;

        tf_params to_c() const
        {
            tf_params c;
            tf_default_params(&c);
            c.cols = cols; c.rows = rows;
            c.fx = intr.fx; c.fy = intr.fy; c.cx = intr.cx; c.cy = intr.cy;
            c.bilateral_sigma_depth = bilateral_sigma_depth;
            c.bilateral_sigma_spatial = bilateral_sigma_spatial;
            c.bilateral_kernel_size = bilateral_kernel_size;
            c.icp_truncate_depth_dist = icp_truncate_depth_dist;
            c.icp_dist_thres = icp_dist_thres;
            c.icp_angle_thres = icp_angle_thres;
            for (int i = 0; i < 4; ++i) c.icp_iter_num[i] = i < (int)icp_iter_num.size() ? icp_iter_num[i] : 0;
            if (sceneParams) {
                c.mu = sceneParams->mu; c.maxW = sceneParams->maxW; c.voxelSize = sceneParams->voxelSize;
                c.viewFrustum_min = sceneParams->viewFrustum_min; c.viewFrustum_max = sceneParams->viewFrustum_max;
            }
            c.n_buckets = n_buckets; c.n_excess = n_excess; c.n_blocks = n_blocks;
            c.vis_capacity = vis_capacity; c.max_render_blocks = max_render_blocks;
            c.voxel_rgb = integrate_colour ? 1 : 0;
            c.rgb_intr[0] = rgb_intr.fx; c.rgb_intr[1] = rgb_intr.fy; c.rgb_intr[2] = rgb_intr.cx; c.rgb_intr[3] = rgb_intr.cy;
            affine_to_rt(depth_to_rgb, c.depth_to_rgb);
            return c;
        }
    };

    class TopFu
    {
    public:
        typedef SharedPtr<TopFu> Ptr;   // cv::Ptr<TopFu> (topfu.hpp:65); std::shared_ptr without OpenCV

        explicit TopFu(const TopFuParams& params) : params_(params)
        {
            const tf_params c = params_.to_c();
            check(tf_create(&c, &ctx_), "tf_create");
            // topfu.cpp:77-80: the tracker takes the TopFu's thresholds and iterations
            icp_.bind(ctx_);
            icp_.setDistThreshold(params_.icp_dist_thres);
            icp_.setAngleThreshold(params_.icp_angle_thres);
            icp_.setIterationsNum(params_.icp_iter_num);
            poses_.reserve(30000);
            poses_.push_back(Affine3f::Identity());
        }
        ~TopFu() { tf_destroy(ctx_); }
        TopFu(const TopFu&) = delete;
        TopFu& operator=(const TopFu&) = delete;

        const TopFuParams& params() const { return params_; }
        TopFuParams& params() { return params_; }

        // topfu.hpp:75-76: the frame tracker; its setters change the parameters the following
        // frames use, and estimateTransform runs it on caller pyramids (through this context,
        // whose current / previous maps it overwrites)
        const cuda::ProjectiveICP& icp() const { return icp_; }
        cuda::ProjectiveICP& icp() { return icp_; }

        void reset()                                  // topfu.cpp:141-152
        {
            check(tf_reset(ctx_), "tf_reset");
            frame_counter_ = 0;
            poses_.clear();
            poses_.push_back(Affine3f::Identity());
        }

        // TopFu::operator() (topfu.cpp:161-330); the colour image is unused by the reference too
        bool operator()(const cuda::Depth& depth, const cuda::Image& = cuda::Image())
        {
            return frame(depth, nullptr);
        }
        // with params().integrate_colour: the frame's RGBA image (Vector4u, the engine's view->rgb)
        // integrated into the Voxel_s_rgb colour (an addition)
        bool operator()(const cuda::Depth& depth, const cuda::image4u& rgba)
        {
            return frame(depth, &rgba);
        }

    private:
        bool frame(const cuda::Depth& depth, const cuda::image4u* rgba)
        {
            float rt[12];
            // no tf_stats: the call returns once the frame's result is known (stats() waits for the rest)
            const tf_status s = rgba && !rgba->empty()
                ? tf_process_frame_rgb(ctx_, depth.ptr(), depth.step(), reinterpret_cast<const uint8_t*>(rgba->ptr()),
                                       rgba->step(), rt, nullptr)
                : tf_process_frame(ctx_, depth.ptr(), depth.step(), rt, nullptr);
            if (s == TF_ICP_FAIL) {                   // reset(), return false (topfu.cpp:263-264)
                frame_counter_ = 0;
                poses_.clear();
                poses_.push_back(Affine3f::Identity());
                return false;
            }
            check(s, "tf_process_frame");
            if (frame_counter_ > 0) poses_.push_back(affine_from_rt(rt));   // poses_.back() * affine
            ++frame_counter_;
            return true;
        }

    public:

        // TopFu::renderImage (topfu.cpp:332-377): grey shading of the current pose.  The type
        // argument (default: the reference's RENDER_SHADED_GREYSCALE) selects one of the engine's
        // RenderImageType modes (VisualisationEngine.hpp:15-22) -- an addition, source compatible.
        enum RenderImageType {
            RENDER_SHADED_GREYSCALE = TF_RENDER_SHADED_GREYSCALE,
            RENDER_SHADED_GREYSCALE_IMAGENORMALS = TF_RENDER_SHADED_GREYSCALE_IMAGENORMALS,
            RENDER_COLOUR_FROM_VOLUME = TF_RENDER_COLOUR_FROM_VOLUME,
            RENDER_COLOUR_FROM_NORMAL = TF_RENDER_COLOUR_FROM_NORMAL,
            RENDER_COLOUR_FROM_CONFIDENCE = TF_RENDER_COLOUR_FROM_CONFIDENCE
        };
        void renderImage(cuda::image4u& image, RenderImageType type = RENDER_SHADED_GREYSCALE)
        {
            image.create(params_.rows, params_.cols);
            check(tf_render_image_type(ctx_, (int)type, reinterpret_cast<uint8_t*>(image.ptr()), image.step()),
                  "tf_render_image_type");
        }

        // renderView (an addition: tf_view_render): the map from any camera -> world pose at any size, through a
        // free view of that size (created on first use, released with the TopFu).  The tracker's state and output
        // are untouched, so it may be called between frames.  cols / rows 0: the tracker's; at another size the
        // tracker's intrinsics are scaled with the image (the same field of view).  whole: on a swapping map the
        // blocks held in the GlobalCache as well as the resident ones (tf_set_view_reading; set before every call, so
        // one view per size serves both readings).
        void renderView(cuda::image4u& image, const Affine3f& cam_to_world, RenderImageType type = RENDER_SHADED_GREYSCALE,
                        int cols = 0, int rows = 0, bool whole = false)
        {
            if (cols <= 0) cols = params_.cols;
            if (rows <= 0) rows = params_.rows;
            tf_view* v = nullptr;
            for (const SizedView& e : views_)
                if (e.cols == cols && e.rows == rows) v = e.view;
            if (!v) {
                const tf_view_params vp = { cols, rows, 0, 0 };
                check(tf_view_create(ctx_, &vp, &v), "tf_view_create");
                views_.push_back(SizedView{ cols, rows, v });
            }
            check(tf_set_view_reading(v, whole ? TF_VIEW_WHOLE : TF_VIEW_RESIDENT), "tf_set_view_reading");
            float rt[12], in[4];
            affine_to_rt(cam_to_world, rt);
            const tf_params c = params_.to_c();
            const float sx = (float)cols / (float)c.cols, sy = (float)rows / (float)c.rows;
            in[0] = c.fx * sx; in[1] = c.fy * sy; in[2] = c.cx * sx; in[3] = c.cy * sy;
            image.create(rows, cols);
            check(tf_view_render(v, cols == c.cols && rows == c.rows ? nullptr : in, rt, (int)type,
                                 reinterpret_cast<uint8_t*>(image.ptr()), image.step()), "tf_view_render");
        }

        Affine3f getCameraPose(int time = -1) const   // topfu.cpp:154-159
        {
            if (time > (int)poses_.size() || time < 0) time = (int)poses_.size() - 1;
            return poses_[time];
        }

        tf_stats stats() const
        {
            tf_stats s;
            check(tf_get_stats(ctx_, &s), "tf_get_stats");
            return s;
        }
        // Scene queries (additions: tf_scene_query / tf_scene_slice, as Scene::query / Scene::slice): the TSDF at n
        // device points (3 floats each, voxel units or metres) or on the pixels of the plane origin + x * u + y * v,
        // into the device arrays of `out` that are not null.  The tracker does not notice.  (TopFu itself runs
        // without swapping, where whole is the resident reading byte for byte.)
        void query(const float* points, long long n, tf_query_units units, bool whole, const tf_query_out& out)
        {
            check(tf_scene_query(ctx_, points, n, (int)units, whole ? TF_VIEW_WHOLE : TF_VIEW_RESIDENT, &out), "tf_scene_query");
        }
        void slice(const float origin[3], const float u[3], const float v[3], int cols, int rows, tf_query_units units, bool whole,
                   const tf_query_out& out)
        {
            check(tf_scene_slice(ctx_, origin, u, v, cols, rows, (int)units, whole ? TF_VIEW_WHOLE : TF_VIEW_RESIDENT, &out),
                  "tf_scene_slice");
        }
        // Mesh extraction (additions: the reference has no mesher; tf_mesh_extract / tf_mesh_save_ply).
        // extractMesh: the scene's triangles as 9 floats each (three xyz vertices, right-hand normal
        // towards free space) in `triangles`, resized to fit; returns their number.
        long long extractMesh(cuda::DeviceArray<float>& triangles)
        {
            long long n = 0;
            check(tf_mesh_extract(ctx_, nullptr, 0, &n), "tf_mesh_extract");
            triangles.create((size_t)n * 9);
            if (n > 0) {
                long long m = 0;
                check(tf_mesh_extract(ctx_, triangles.ptr(), n, &m), "tf_mesh_extract");
            }
            return n;
        }
        // the mesh as a binary PLY with welded vertices
        void saveMesh(const std::string& path) { check(tf_mesh_save_ply(ctx_, path.c_str()), "tf_mesh_save_ply"); }
        // extractMesh with per-vertex attributes (tf_mesh_extract_attr): normals (9 floats per triangle,
        // unit TSDF gradient per vertex) and colours (12 bytes per triangle, RGBA per vertex; voxel_rgb
        // contexts only), each skipped when its pointer is null; the same triangles in the same order
        long long extractMesh(cuda::DeviceArray<float>& triangles, cuda::DeviceArray<float>* normals,
                              cuda::DeviceArray<unsigned char>* colours)
        {
            long long n = 0;
            check(tf_mesh_extract_attr(ctx_, nullptr, nullptr, nullptr, 0, &n), "tf_mesh_extract_attr");
            triangles.create((size_t)n * 9);
            if (normals) normals->create((size_t)n * 9);
            if (colours) colours->create((size_t)n * 12);
            if (n > 0) {
                long long m = 0;
                check(tf_mesh_extract_attr(ctx_, triangles.ptr(), normals ? normals->ptr() : nullptr,
                                           colours ? colours->ptr() : nullptr, n, &m), "tf_mesh_extract_attr");
            }
            return n;
        }
        // extractMesh by flags: TF_MESH_WHOLE = the reading over both tiers of a swapping scene
        // (tf_mesh_extract_whole; TopFu itself runs without swapping, where it is the resident mesh byte for
        // byte -- a swapping caller holds a Scene, engines.hpp, which has the same pair), 0 = as above
        long long extractMesh(cuda::DeviceArray<float>& triangles, cuda::DeviceArray<float>* normals, int flags)
        {
            if (!(flags & TF_MESH_WHOLE)) return extractMesh(triangles, normals, (cuda::DeviceArray<unsigned char>*)nullptr);
            long long n = 0;
            check(tf_mesh_extract_whole(ctx_, nullptr, nullptr, 0, &n), "tf_mesh_extract_whole");
            triangles.create((size_t)n * 9);
            if (normals) normals->create((size_t)n * 9);
            if (n > 0) {
                long long m = 0;
                check(tf_mesh_extract_whole(ctx_, triangles.ptr(), normals ? normals->ptr() : nullptr, n, &m), "tf_mesh_extract_whole");
            }
            return n;
        }
        // the mesh as a PLY with nx ny nz (TF_MESH_NORMALS) and / or red green blue alpha (TF_MESH_COLOURS);
        // TF_MESH_WHOLE passes through to tf_mesh_save_ply_attr (not with colours, not indexed);
        // with TF_MESH_INDEXED: the indexed vertex table as it leaves the GPU, no host weld (tf_mesh_save_ply_indexed)
        void saveMesh(const std::string& path, int attrs)
        {
            if (attrs & TF_MESH_INDEXED) check(tf_mesh_save_ply_indexed(ctx_, path.c_str(), attrs), "tf_mesh_save_ply_indexed");
            else check(tf_mesh_save_ply_attr(ctx_, path.c_str(), attrs), "tf_mesh_save_ply_attr");
        }
        // The mesh with shared vertices (tf_mesh_extract_indexed): 3 floats per vertex, 3 vertex numbers per
        // triangle (extractMesh's triangles in its order), and per vertex 3 normal floats / 4 RGBA bytes where
        // the pointer is not null; all resized to fit.  Returns the triangle count; vertices.size() / 3 is
        // the vertex count.
        long long extractMeshIndexed(cuda::DeviceArray<float>& vertices, cuda::DeviceArray<unsigned>& indices,
                                     cuda::DeviceArray<float>* normals = nullptr, cuda::DeviceArray<unsigned char>* colours = nullptr)
        {
            long long nv = 0, nt = 0;
            check(tf_mesh_extract_indexed(ctx_, nullptr, nullptr, nullptr, 0, nullptr, 0, &nv, &nt), "tf_mesh_extract_indexed");
            vertices.create((size_t)nv * 3);
            indices.create((size_t)nt * 3);
            if (normals) normals->create((size_t)nv * 3);
            if (colours) colours->create((size_t)nv * 4);
            if (nt > 0) {
                long long mv = 0, mt = 0;
                check(tf_mesh_extract_indexed(ctx_, vertices.ptr(), normals ? normals->ptr() : nullptr, colours ? colours->ptr() : nullptr, nv,
                                              indices.ptr(), nt, &mv, &mt), "tf_mesh_extract_indexed");
            }
            return nt;
        }

        // Scene checkpoints (additions: tf_scene_save / tf_scene_load / tf_scene_file_info).  saveScene writes
        // the state a sequence resumes from; loadScene replaces this TopFu's scene, pose and frame counter by
        // the file's (the pose history restarts at the loaded pose); the capacities, image size and scene
        // parameters must be the file's.  sceneFileInfo reads a file's header without a context.
        void saveScene(const std::string& path) { check(tf_scene_save(ctx_, path.c_str()), "tf_scene_save"); }
        void loadScene(const std::string& path)
        {
            check(tf_scene_load(ctx_, path.c_str()), "tf_scene_load");
            after_load();
        }
        static struct tf_scene_file_info sceneFileInfo(const std::string& path)
        {
            struct tf_scene_file_info info;
            check(tf_scene_file_info(path.c_str(), &info), "tf_scene_file_info");
            return info;
        }

        // Map checkpoints (additions: tf_map_save / tf_map_load / tf_map_file_info): saveScene's file on this
        // TopFu (it runs without swapping, so version 1, byte for byte); loadMap takes what saveMap wrote.  A
        // swapping caller holds a Scene (engines.hpp: Scene::saveMap / loadMap, the version-2 file).
        void saveMap(const std::string& path) { check(tf_map_save(ctx_, path.c_str()), "tf_map_save"); }
        void loadMap(const std::string& path)
        {
            check(tf_map_load(ctx_, path.c_str()), "tf_map_load");
            after_load();
        }
        // Resized load (addition: tf_map_load_resized): a file saved by a TopFu of other n_buckets / n_excess /
        // n_blocks; the map is re-hashed into this one's tables (records without a block position are dropped).
        void loadMapResized(const std::string& path, struct tf_resize_report* report = nullptr)
        {
            check(tf_map_load_resized(ctx_, path.c_str(), report), "tf_map_load_resized");
            after_load();
        }
        // Map merge (addition: tf_map_merge): a version-1 checkpoint fused into the map this TopFu holds, its block
        // positions moved by `offset` whole blocks -- combined voxel by voxel where the map already has the block,
        // inserted where it does not.  The pose, the poses so far and the tracker's maps stay.  Throws with
        // TF_CAPACITY when the free lists are too short (report, when given, says what is needed); the map is then
        // as it was.
        void mergeMap(const std::string& path, const std::array<int, 3>& offset = { 0, 0, 0 }, struct tf_merge_report* report = nullptr)
        {
            check(tf_map_merge(ctx_, path.c_str(), offset.data(), report), "tf_map_merge");
        }
        static struct tf_map_file_info mapFileInfo(const std::string& path)
        {
            struct tf_map_file_info info;
            check(tf_map_file_info(path.c_str(), &info), "tf_map_file_info");
            return info;
        }

        tf_ctx* handle() { return ctx_; }
        hipStream_t stream() const { return (hipStream_t)tf_get_stream(ctx_); }

    private:
        static void check(tf_status s, const char* what)
        {
            if (s != TF_OK) throw std::runtime_error(std::string(what) + ": " + tf_status_string(s));
        }
        // the wrapper's own frame counter and pose list follow a loaded map
        void after_load()
        {
            float rt[12];
            check(tf_get_pose(ctx_, rt), "tf_get_pose");
            frame_counter_ = stats().frame_counter;
            poses_.clear();
            poses_.push_back(affine_from_rt(rt));
        }
        struct SizedView { int cols, rows; tf_view* view; };
        TopFuParams params_;
        tf_ctx* ctx_ = nullptr;
        std::vector<SizedView> views_;    // renderView's free views, one per size (tf_destroy releases them)
        cuda::ProjectiveICP icp_;
        int frame_counter_ = 0;
        std::vector<Affine3f> poses_;
    };
}
