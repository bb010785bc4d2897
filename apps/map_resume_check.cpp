// map_resume_check.cpp -- a swapping Scene resumed from a map checkpoint, through the engine API
// (include/tfusion/engines.hpp): Scene(params, useSwapping = true), SceneReconstructionEngine_CUDA::
// {AllocateSceneFromDepth, IntegrateIntoScene} and SwappingEngine_CUDA::{IntegrateGlobalIntoLocal,
// SaveToGlobalMemory} over a camera walking round the room in place (ground-truth poses, 96 x 72, 4 cm voxels)
// with a VBA of 128 blocks, far too small for it.  Scene A fuses the first half of the walk and calls
// Scene::saveMap; a second Scene calls loadMap; both fuse the second half.  The counters and the whole-map
// mesh (TF_MESH_WHOLE, both tiers) of the two must then be byte-identical.  Prints the file's size beside the
// n_total x 2049 bytes of the GlobalCache's own SaveToFile and one verdict line; returns 1 on a difference.
//
//   ./map_resume_check [frames=20] [map=/tmp/map_resume_check.tfmap]
#include <tfusion/engines.hpp>

#include "synth_depth.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace tfusion;

typedef Scene<Voxel_s, VoxelBlockHash> SwapScene;

struct Walker {
    TopFuParams p;
    SceneReconstructionEngine_CUDA<Voxel_s, VoxelBlockHash> sceneEngine;
    SwappingEngine_CUDA<Voxel_s, VoxelBlockHash> swapEngine;
    std::vector<unsigned short> depth;
    cuda::Depth depth_device;
    cuda::Dists dists;

    // frame k of the walk into every scene of the list: 40 degrees a frame, there and back
    void fuse(int k, int frames, std::vector<SwapScene*> scenes, RenderState_VH* renderState)
    {
        const int half = frames / 2;
        const double a = 40.0 * (k < half ? k : frames - 1 - k) * M_PI / 180.0, ca = std::cos(a), sa = std::sin(a);
        const double R[9] = { ca, 0, sa, 0, 1, 0, -sa, 0, ca }, t[3] = { 0.15, -0.15, 0.6 };
        tfusion_apps::render_depth(R, t, p.cols, p.rows, p.intr, depth);
        depth_device.upload(depth.data(), (size_t)p.cols * 2, p.rows, p.cols);
        cuda::computeDists(depth_device, dists, p.intr);
        cuda::waitAllDefaultStream();
        Affine3f c2w = Affine3f::Identity();
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) c2w.matrix(r, c) = (float)R[r * 3 + c];
            c2w.matrix(r, 3) = (float)t[r];
        }
        for (SwapScene* s : scenes) {
            sceneEngine.AllocateSceneFromDepth(s, p.intr, c2w.inv(), dists, renderState);
            sceneEngine.IntegrateIntoScene(s, p.intr, c2w.inv(), dists, renderState);
            swapEngine.IntegrateGlobalIntoLocal(s, renderState);
            swapEngine.SaveToGlobalMemory(s, renderState);
        }
    }
};

static std::vector<float> whole_mesh(SwapScene& s, long long* n)
{
    cuda::DeviceArray<float> tris;
    *n = s.extractMesh(tris, nullptr, TF_MESH_WHOLE);
    std::vector<float> host((size_t)*n * 9);
    if (*n > 0) tris.download(host.data());
    return host;
}

int main(int argc, char** argv)
{
    const int frames = argc > 1 ? std::atoi(argv[1]) : 20;
    const std::string path = argc > 2 ? argv[2] : "/tmp/map_resume_check.tfmap";
    if (frames < 2) { std::fprintf(stderr, "frames >= 2\n"); return 2; }
    const int cols = 96, rows = 72;
    cuda::setDevice(0);
    Walker w;
    w.p = TopFuParams::default_params();
    w.p.cols = cols; w.p.rows = rows;
    const double s = cols / 640.0;
    w.p.intr = Intr(504.261f * s, 503.905f * s, 352.457f * s, 272.202f * s);
    w.p.sceneParams = std::make_shared<SceneParams>(0.08f, 100, 0.04f, 0.2f, 3.0f, false);
    w.p.n_buckets = 4096; w.p.n_excess = 512; w.p.n_blocks = 128;

    SwapScene a(w.p.sceneParams.get(), true, w.p), b(w.p.sceneParams.get(), true, w.p);
    RenderState_VH renderState(a.globalCache->noTotalEntries, Vector2i(cols, rows), w.p.sceneParams->viewFrustum_min,
                               w.p.sceneParams->viewFrustum_max);
    w.sceneEngine.ResetScene(&a);
    w.sceneEngine.ResetScene(&b);
    const int n_total = a.globalCache->noTotalEntries, half = frames / 2;

    for (int k = 0; k < half; ++k) w.fuse(k, frames, { &a }, &renderState);
    a.saveMap(path);
    struct tf_map_file_info info;
    tf_engine_check(tf_map_file_info(path.c_str(), &info), "tf_map_file_info");
    b.loadMap(path);
    for (int k = half; k < frames; ++k) w.fuse(k, frames, { &a, &b }, &renderState);

    int fails = 0;
    if (info.version != 2 || info.n_cache_blocks <= 0) { ++fails; std::printf("MISMATCH: version %d, %lld cache blocks in the file\n", info.version, info.n_cache_blocks); }
    const tf_stats ca = a.counters(), cb = b.counters();
    if (std::memcmp(&ca, &cb, sizeof(ca)) != 0) { ++fails; std::printf("MISMATCH: counters differ\n"); }
    int sa[3], sb[3];
    tf_engine_check(tf_swap_counts(a.context(), sa), "tf_swap_counts");
    tf_engine_check(tf_swap_counts(b.context(), sb), "tf_swap_counts");
    if (std::memcmp(sa, sb, sizeof(sa)) != 0) { ++fails; std::printf("MISMATCH: swap counts differ\n"); }
    long long na = 0, nb = 0;
    const std::vector<float> ma = whole_mesh(a, &na), mb = whole_mesh(b, &nb);
    if (na <= 0) { ++fails; std::printf("MISMATCH: an empty mesh\n"); }
    if (na != nb || std::memcmp(ma.data(), mb.data(), ma.size() * sizeof(float)) != 0) {
        ++fails;
        std::printf("MISMATCH: whole meshes differ (%lld and %lld triangles)\n", na, nb);
    }
    std::printf("map file %lld bytes (%lld records, %lld active + %lld stored blocks); GlobalCache SaveToFile %lld bytes\n",
                info.scene.file_bytes, info.scene.n_records, info.scene.n_blocks_stored, info.n_cache_blocks, (long long)n_total * 2049);
    std::printf("map_resume_check frames %d + %d whole mesh %lld triangles: %s\n", half, frames - half, na, fails ? "MISMATCH" : "MATCH");
    return fails ? 1 : 0;
}
