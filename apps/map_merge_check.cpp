// map_merge_check.cpp -- two Scenes fused over the two halves of a walk and joined by a map merge, through the
// engine API (include/tfusion/engines.hpp): Scene(params, useSwapping = false), SceneReconstructionEngine_CUDA::
// {AllocateSceneFromDepth, IntegrateIntoScene} over a camera turning round the room in place (ground-truth poses,
// 96 x 72, 4 cm voxels).  Scene A fuses the first half of the walk and one frame more, scene B the second half; B
// is saved (Scene::saveMap) and merged into A (Scene::mergeMap).  The shared frame's blocks combine, the rest of B
// is inserted.  Prints the report and the counters, saves A's mesh, and checks: every record of B was combined or
// inserted, A's free-block top fell by blocks_used, the mesh grew, and a second merge of the same file combines
// every record and takes nothing from the lists.  Returns 1 when a check fails.
//
//   ./map_merge_check [frames=12] [map=/tmp/map_merge_check.tfscene] [mesh=/tmp/map_merge_check.ply]
#include <tfusion/engines.hpp>

#include "synth_depth.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

using namespace tfusion;

typedef Scene<Voxel_s, VoxelBlockHash> PlainScene;

struct Walker {
    TopFuParams p;
    SceneReconstructionEngine_CUDA<Voxel_s, VoxelBlockHash> sceneEngine;
    std::vector<unsigned short> depth;
    cuda::Depth depth_device;
    cuda::Dists dists;

    // frame k of the walk into the scene: 25 degrees a frame
    void fuse(int k, PlainScene* s, RenderState_VH* renderState)
    {
        const double a = 25.0 * k * M_PI / 180.0, ca = std::cos(a), sa = std::sin(a);
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
        sceneEngine.AllocateSceneFromDepth(s, p.intr, c2w.inv(), dists, renderState);
        sceneEngine.IntegrateIntoScene(s, p.intr, c2w.inv(), dists, renderState);
    }
};

static long long triangles(PlainScene& s)
{
    cuda::DeviceArray<float> tris;
    return s.extractMesh(tris, nullptr, 0);
}

int main(int argc, char** argv)
{
    const int frames = argc > 1 ? std::atoi(argv[1]) : 12;
    const std::string path = argc > 2 ? argv[2] : "/tmp/map_merge_check.tfscene";
    const std::string mesh = argc > 3 ? argv[3] : "/tmp/map_merge_check.ply";
    if (frames < 2) { std::fprintf(stderr, "frames >= 2\n"); return 2; }
    const int cols = 96, rows = 72;
    cuda::setDevice(0);
    Walker w;
    w.p = TopFuParams::default_params();
    w.p.cols = cols; w.p.rows = rows;
    const double s = cols / 640.0;
    w.p.intr = Intr(504.261f * s, 503.905f * s, 352.457f * s, 272.202f * s);
    w.p.sceneParams = std::make_shared<SceneParams>(0.08f, 100, 0.04f, 0.2f, 3.0f, false);
    w.p.n_buckets = 4096; w.p.n_excess = 512; w.p.n_blocks = 8192;
    TopFuParams pb = w.p;                                  // B's tables are its own: the capacities need not agree
    pb.n_buckets = 1024; pb.n_excess = 2048; pb.n_blocks = 4096;

    PlainScene a(w.p.sceneParams.get(), false, w.p), b(w.p.sceneParams.get(), false, pb);
    RenderState_VH stateA(w.p.n_buckets + w.p.n_excess, Vector2i(cols, rows), w.p.sceneParams->viewFrustum_min, w.p.sceneParams->viewFrustum_max);
    RenderState_VH stateB(pb.n_buckets + pb.n_excess, Vector2i(cols, rows), w.p.sceneParams->viewFrustum_min, w.p.sceneParams->viewFrustum_max);
    w.sceneEngine.ResetScene(&a);
    w.sceneEngine.ResetScene(&b);
    const int half = frames / 2;
    for (int k = 0; k <= half; ++k) w.fuse(k, &a, &stateA);
    for (int k = half; k < frames; ++k) w.fuse(k, &b, &stateB);
    b.saveMap(path);
    struct tf_map_file_info info;
    tf_engine_check(tf_map_file_info(path.c_str(), &info), "tf_map_file_info");

    const tf_stats before = a.counters();
    const long long tris_before = triangles(a);
    struct tf_merge_report rep, again;
    a.mergeMap(path, { 0, 0, 0 }, &rep);
    const tf_stats after = a.counters();
    const long long tris_after = triangles(a);
    a.saveMesh(mesh);
    a.mergeMap(path, { 0, 0, 0 }, &again);
    const tf_stats last = a.counters();

    int fails = 0;
    const long long carried = rep.records_combined + rep.records_inserted + rep.records_revived;
    if (info.version != 1 || carried != info.scene.n_blocks_stored || rep.records_skipped != info.scene.n_records - carried) {
        ++fails; std::printf("MISMATCH: the report does not add up to the file's records\n");
    }
    if (rep.records_combined <= 0 || rep.records_inserted <= 0) { ++fails; std::printf("MISMATCH: no combined or no inserted record\n"); }
    if (rep.blocks_used != rep.records_inserted + rep.records_revived || before.lastFreeBlockId - after.lastFreeBlockId != rep.blocks_used ||
        before.lastFreeExcessListId - after.lastFreeExcessListId != rep.excess_used) {
        ++fails; std::printf("MISMATCH: the counters did not fall by what the report says\n");
    }
    if (before.noVisibleEntries != after.noVisibleEntries) { ++fails; std::printf("MISMATCH: the visible list moved\n"); }
    if (tris_after <= tris_before) { ++fails; std::printf("MISMATCH: the mesh did not grow (%lld -> %lld triangles)\n", tris_before, tris_after); }
    if (again.records_combined != carried || again.blocks_used != 0 || again.excess_used != 0 || last.lastFreeBlockId != after.lastFreeBlockId) {
        ++fails; std::printf("MISMATCH: a second merge did not combine every record\n");
    }
    std::printf("file %lld records, %lld blocks; merged: %lld combined, %lld inserted, %lld revived, %lld skipped, %lld blocks and %lld excess "
                "slots used\n", info.scene.n_records, info.scene.n_blocks_stored, rep.records_combined, rep.records_inserted,
                rep.records_revived, rep.records_skipped, rep.blocks_used, rep.excess_used);
    std::printf("lastFreeBlockId %d -> %d, lastFreeExcessListId %d -> %d; mesh %lld -> %lld triangles, written to %s\n",
                before.lastFreeBlockId, after.lastFreeBlockId, before.lastFreeExcessListId, after.lastFreeExcessListId, tris_before,
                tris_after, mesh.c_str());
    std::printf("map_merge_check frames %d + %d: %s\n", half + 1, frames - half, fails ? "MISMATCH" : "MATCH");
    return fails ? 1 : 0;
}
