// mesh_whole_check.cpp -- the whole map of a swapping Scene as a mesh, through the engine API
// (include/tfusion/engines.hpp): Scene(params, useSwapping = true), SceneReconstructionEngine_CUDA::
// {AllocateSceneFromDepth, IntegrateIntoScene} and SwappingEngine_CUDA::{IntegrateGlobalIntoLocal,
// SaveToGlobalMemory} over a camera turning in place (ground-truth poses, 96 x 72, 4 cm voxels) with a VBA
// of 128 blocks, far too small for the room, then Scene::extractMesh / saveMesh with TF_MESH_WHOLE: the
// blocks in the GlobalCache are meshed where they lie.  Checks that blocks were evicted, that the whole mesh
// holds more triangles than the resident one, that the extraction left both tiers alone and that the file's
// face count is the extraction's.  Bit-exactness against the reference is the Python tests' job
// (tests/test_gpu_mesh_whole.py), which reads the state this program dumps when given a prefix.
//
//   ./mesh_whole_check [mesh.ply=/tmp/mesh_whole_check.ply] [dump_prefix] [--indexed out.ply]
//   dump_prefix: the five buffers the whole reading resolves, as <prefix>.hash .vba .state .flags .store
//   --indexed out.ply: also the whole map with shared vertices (Scene::extractMeshIndexed with TF_MESH_WHOLE,
//   Scene::saveMeshIndexedWhole -- the streaming writer), its vertex and triangle counts printed
#include <tfusion/engines.hpp>

#include "synth_depth.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <cstring>
#include <string>
#include <vector>

using namespace tfusion;

static std::vector<unsigned char> download(tf_ctx* ctx, int which)
{
    size_t n = 0;
    tf_engine_check(tf_buffer_bytes(ctx, which, 0, &n), "tf_buffer_bytes");
    std::vector<unsigned char> out(n);
    tf_engine_check(tf_download(ctx, which, 0, out.data(), n), "tf_download");
    return out;
}

static const int kBuffers[5] = { TF_BUF_HASH, TF_BUF_VBA, TF_BUF_SWAP_STATE, TF_BUF_SWAP_STORED_FLAGS, TF_BUF_SWAP_STORED };
static const char* kNames[5] = { ".hash", ".vba", ".state", ".flags", ".store" };

int main(int argc, char** argv)
{
    std::string indexedPath;
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--indexed")) {
            indexedPath = argv[i + 1];
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    const std::string path = argc > 1 ? argv[1] : "/tmp/mesh_whole_check.ply";
    const int cols = 96, rows = 72;
    cuda::setDevice(0);
    TopFuParams p = TopFuParams::default_params();
    p.cols = cols; p.rows = rows;
    const double s = cols / 640.0;
    p.intr = Intr(504.261f * s, 503.905f * s, 352.457f * s, 272.202f * s);
    p.sceneParams = std::make_shared<SceneParams>(0.08f, 100, 0.04f, 0.2f, 3.0f, false);
    p.n_buckets = 4096; p.n_excess = 512; p.n_blocks = 128;

    Scene<Voxel_s, VoxelBlockHash> scene(p.sceneParams.get(), true, p);
    SceneReconstructionEngine_CUDA<Voxel_s, VoxelBlockHash> sceneEngine;
    SwappingEngine_CUDA<Voxel_s, VoxelBlockHash> swapEngine;
    RenderState_VH renderState(scene.globalCache->noTotalEntries, Vector2i(cols, rows), p.sceneParams->viewFrustum_min,
                               p.sceneParams->viewFrustum_max);
    sceneEngine.ResetScene(&scene);
    const int n_total = scene.globalCache->noTotalEntries;

    std::vector<unsigned short> depth;
    cuda::Depth depth_device;
    cuda::Dists dists;
    for (int k = 0; k <= 12; ++k) {
        const double a = (30.0 * k) * M_PI / 180.0, ca = std::cos(a), sa = std::sin(a);
        const double R[9] = { ca, 0, sa, 0, 1, 0, -sa, 0, ca }, t[3] = { 0.15, -0.15, 0.6 };
        tfusion_apps::render_depth(R, t, cols, rows, p.intr, depth);
        depth_device.upload(depth.data(), (size_t)cols * 2, rows, cols);
        cuda::computeDists(depth_device, dists, p.intr);
        cuda::waitAllDefaultStream();
        Affine3f c2w = Affine3f::Identity();
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) c2w.matrix(r, c) = (float)R[r * 3 + c];
            c2w.matrix(r, 3) = (float)t[r];
        }
        sceneEngine.AllocateSceneFromDepth(&scene, p.intr, c2w.inv(), dists, &renderState);
        sceneEngine.IntegrateIntoScene(&scene, p.intr, c2w.inv(), dists, &renderState);
        swapEngine.IntegrateGlobalIntoLocal(&scene, &renderState);
        swapEngine.SaveToGlobalMemory(&scene, &renderState);
    }

    int fails = 0, stored = 0;
    for (int i = 0; i < n_total; ++i) stored += scene.globalCache->HasStoredData(i) ? 1 : 0;
    if (stored == 0) { ++fails; std::printf("MISMATCH: nothing was evicted\n"); }

    std::vector<unsigned char> before[5];
    for (int b = 0; b < 5; ++b) before[b] = download(scene.context(), kBuffers[b]);

    cuda::DeviceArray<float> tris, normals;
    const long long resident = scene.extractMesh(tris);
    const long long whole = scene.extractMesh(tris, &normals, TF_MESH_WHOLE);
    if (whole <= resident) { ++fails; std::printf("MISMATCH: whole %lld, resident %lld triangles\n", whole, resident); }
    if ((long long)tris.size() != whole * 9 || (long long)normals.size() != whole * 9) { ++fails; std::printf("MISMATCH: buffer sizes\n"); }
    scene.saveMesh(path, TF_MESH_WHOLE);

    // the file's face count, from its header
    long long faces = -1;
    if (std::FILE* f = std::fopen(path.c_str(), "rb")) {
        char line[256];
        while (std::fgets(line, sizeof line, f) && std::strncmp(line, "end_header", 10))
            if (!std::strncmp(line, "element face ", 13)) faces = std::atoll(line + 13);
        std::fclose(f);
    }
    if (faces != whole) { ++fails; std::printf("MISMATCH: %lld faces in the file, %lld triangles extracted\n", faces, whole); }

    if (!indexedPath.empty()) {
        cuda::DeviceArray<float> verts, vnormals;
        cuda::DeviceArray<unsigned> indices;
        const long long nt = scene.extractMeshIndexed(verts, indices, &vnormals, TF_MESH_WHOLE);
        const long long nv = (long long)verts.size() / 3;
        if (nt != whole) { ++fails; std::printf("MISMATCH: %lld indexed triangles, %lld in the soup\n", nt, whole); }
        if ((long long)indices.size() != nt * 3 || vnormals.size() != verts.size()) { ++fails; std::printf("MISMATCH: indexed buffer sizes\n"); }
        scene.saveMeshIndexedWhole(indexedPath, TF_MESH_NORMALS);
        std::printf("indexed whole mesh: %lld vertices, %lld triangles\n", nv, nt);
    }

    for (int b = 0; b < 5; ++b) {
        const std::vector<unsigned char> after = download(scene.context(), kBuffers[b]);
        if (after != before[b]) { ++fails; std::printf("MISMATCH: extraction changed buffer %s\n", kNames[b]); }
        if (argc > 2) {
            const std::string name = std::string(argv[2]) + kNames[b];
            std::FILE* f = std::fopen(name.c_str(), "wb");
            if (!f || std::fwrite(after.data(), 1, after.size(), f) != after.size()) { ++fails; std::printf("MISMATCH: cannot write %s\n", name.c_str()); }
            if (f) std::fclose(f);
        }
    }
    std::printf("mesh_whole_check frames 13 stored %d resident %lld whole %lld triangles: %s\n", stored, resident, whole,
                fails ? "MISMATCH" : "MATCH");
    return fails ? 1 : 0;
}
