// view_whole_check.cpp -- the whole map of a swapping Scene looked at through a free view, through the engine API
// (include/tfusion/engines.hpp): mesh_whole_check's scene -- Scene(params, useSwapping = true) fused over a camera
// turning in place (ground-truth poses, 96 x 72, 4 cm voxels) with a VBA of 128 blocks, far too small for the
// room -- then a RenderState_VH of another size with setWhole(true) given to VisualisationEngine_CUDA::
// {FindVisibleBlocks, CreateExpectedDepths, RenderImage} from a pose that looks where the camera was half a turn
// ago: the blocks in the GlobalCache are raycast where they lie.  Checks that blocks were evicted, that the whole
// view lists more blocks and lights more pixels than the resident one, and that the views left both tiers alone.
// Bit-exactness against the reference is the Python tests' job (tests/test_gpu_view_whole.py), which reads the
// picture, the state this program dumps and the key=value words it prints.
//
//   ./view_whole_check [whole.ppm=/tmp/view_whole_check.ppm] [dump_prefix]
//   dump_prefix: the five buffers the whole reading resolves, as <prefix>.hash .vba .state .flags .store
#include <tfusion/engines.hpp>
#include <tfusion/io.hpp>

#include "synth_depth.hpp"

#include <cmath>
#include <cstdio>
#include <memory>
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

static std::vector<unsigned char> fetch(const cuda::image4u& img)
{
    std::vector<unsigned char> px((size_t)img.cols() * img.rows() * 4);
    img.download(px.data(), (size_t)img.cols() * 4);
    return px;
}

static long lit(const std::vector<unsigned char>& px)
{
    long n = 0;
    for (size_t k = 0; k < px.size(); k += 4) n += px[k] > 0;
    return n;
}

static const int kBuffers[5] = { TF_BUF_HASH, TF_BUF_VBA, TF_BUF_SWAP_STATE, TF_BUF_SWAP_STORED_FLAGS, TF_BUF_SWAP_STORED };
static const char* kNames[5] = { ".hash", ".vba", ".state", ".flags", ".store" };

int main(int argc, char** argv)
{
    const std::string path = argc > 1 ? argv[1] : "/tmp/view_whole_check.ppm";
    const int cols = 96, rows = 72, vc = 100, vr = 76;
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
    VisualisationEngine_CUDA<Voxel_s, VoxelBlockHash> vis;
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

    // the view: from the camera's place, turned 3 rad about y -- what the tracker saw half a turn ago
    const float q[6] = { 0.15f, -0.15f, 0.6f, 0.0f, 3.0f, 0.0f };
    const Affine3f c2w(Vec3f(q[3], q[4], q[5]), Vec3f(q[0], q[1], q[2]));
    const float sx = (float)vc / (float)cols, sy = (float)vr / (float)rows;
    const Intr vi(p.intr.fx * sx, p.intr.fy * sy, p.intr.cx * sx, p.intr.cy * sy);
    const Vector4f vi4(vi.fx, vi.fy, vi.cx, vi.cy);
    int n_vis[2] = { 0, 0 };
    std::vector<unsigned char> px[2];
    {
        RenderState_VH viewState(n_total, Vector2i(vc, vr), p.sceneParams->viewFrustum_min, p.sceneParams->viewFrustum_max);
        for (int whole = 0; whole < 2; ++whole) {
            cuda::image4u img;
            viewState.setWhole(whole != 0);
            n_vis[whole] = vis.FindVisibleBlocks(&scene, Matrix4f::fromAffine(c2w.inv()), vi4, &viewState);
            vis.CreateExpectedDepths(&scene, c2w.inv(), vi, &viewState);
            vis.RenderImage(&scene, Matrix4f::fromAffine(c2w), vi4, &viewState, img);
            px[whole] = fetch(img);
        }
        if (!viewState.whole()) { ++fails; std::printf("MISMATCH: the render state lost its reading\n"); }
    }
    if (n_vis[1] <= n_vis[0] || lit(px[1]) <= lit(px[0])) {
        ++fails;
        std::printf("MISMATCH: whole %d blocks %ld pixels, resident %d blocks %ld pixels\n", n_vis[1], lit(px[1]), n_vis[0], lit(px[0]));
    }
    io::writePPM(path, px[1].data(), vc, vr);

    for (int b = 0; b < 5; ++b) {
        const std::vector<unsigned char> after = download(scene.context(), kBuffers[b]);
        if (after != before[b]) { ++fails; std::printf("MISMATCH: the views changed buffer %s\n", kNames[b]); }
        if (argc > 2) {
            const std::string name = std::string(argv[2]) + kNames[b];
            std::FILE* f = std::fopen(name.c_str(), "wb");
            if (!f || std::fwrite(after.data(), 1, after.size(), f) != after.size()) { ++fails; std::printf("MISMATCH: cannot write %s\n", name.c_str()); }
            if (f) std::fclose(f);
        }
    }
    std::printf("cols=%d rows=%d view_cols=%d view_rows=%d pose=%.9g,%.9g,%.9g,%.9g,%.9g,%.9g n_buckets=%d n_excess=%d n_blocks=%d "
                "voxel_size=%.9g mu=%.9g\n", cols, rows, vc, vr, q[0], q[1], q[2], q[3], q[4], q[5], p.n_buckets, p.n_excess, p.n_blocks,
                p.sceneParams->voxelSize, p.sceneParams->mu);
    std::printf("view_whole_check frames 13 stored %d visible %d vs %d lit %ld vs %ld: %s\n", stored, n_vis[1], n_vis[0], lit(px[1]),
                lit(px[0]), fails ? "MISMATCH" : "MATCH");
    return fails ? 1 : 0;
}
