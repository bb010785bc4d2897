// view_check.cpp -- a saved map looked at through the two C++ doors of the free views (tf_view_*):
//   the engine API: VisualisationEngine_CUDA::FindVisibleBlocks binds a RenderState_VH of another size than the
//   scene's to a view of its own; CreateExpectedDepths and RenderImage given that render state work on it;
//   TopFu::renderView: the same picture in one call.
// Both pictures are written as binary PPMs; they are the same bytes, and the scene's own render state is not
// touched (the Scene renders its tracker-sized image before and after, and the two must agree).
//
//   ./view_check scene.tfs cols rows view_cols view_rows tx,ty,tz,rx,ry,rz engine.ppm topfu.ppm
//
// scene.tfs: a scene checkpoint (TopFu::saveScene) of a cols x rows context with the default parameters and the
// demo's intrinsics (demo_headless writes one with --save-scene).
#include <tfusion/engines.hpp>
#include <tfusion/io.hpp>
#include <tfusion/topfu.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace tfusion;

static std::vector<unsigned char> fetch(const cuda::image4u& img)
{
    std::vector<unsigned char> px((size_t)img.cols() * img.rows() * 4);
    img.download(px.data(), (size_t)img.cols() * 4);
    return px;
}

int main(int argc, char** argv)
{
    if (argc != 9) {
        std::fprintf(stderr, "usage: view_check scene cols rows view_cols view_rows tx,ty,tz,rx,ry,rz engine.ppm topfu.ppm\n");
        return 1;
    }
    const std::string path = argv[1];
    const int cols = std::atoi(argv[2]), rows = std::atoi(argv[3]), vc = std::atoi(argv[4]), vr = std::atoi(argv[5]);
    float q[6];
    if (std::sscanf(argv[6], "%f,%f,%f,%f,%f,%f", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5]) != 6) return 1;
    const Affine3f c2w(Vec3f(q[3], q[4], q[5]), Vec3f(q[0], q[1], q[2]));

    cuda::setDevice(0);
    TopFuParams p = TopFuParams::default_params();
    p.cols = cols;
    p.rows = rows;
    const double s = cols / 640.0;
    p.intr = Intr(504.261f * s, 503.905f * s, 352.457f * s, 272.202f * s);
    // the view's intrinsics: the tracker's scaled with the image, as TopFu::renderView scales them
    const float sx = (float)vc / (float)cols, sy = (float)vr / (float)rows;
    const Intr vi(p.intr.fx * sx, p.intr.fy * sy, p.intr.cx * sx, p.intr.cy * sy);
    const Vector4f vi4(vi.fx, vi.fy, vi.cx, vi.cy), ti4(p.intr.fx, p.intr.fy, p.intr.cx, p.intr.cy);

    // ---- the engine API over a Scene
    Scene<Voxel_s, VoxelBlockHash> scene(p.sceneParams.get(), false, p);
    scene.loadMap(path);
    VisualisationEngine_CUDA<Voxel_s, VoxelBlockHash> vis;
    cuda::image4u own_before, own_after, engine_img;
    // the scene's own render state, from the view's pose too (its tracker-sized list: what it holds after the load)
    vis.CreateExpectedDepths(&scene, c2w.inv(), p.intr);
    vis.RenderImage(&scene, Matrix4f::fromAffine(c2w), ti4, nullptr, own_before);
    int n_visible = 0;
    {
        RenderState_VH rs(VoxelBlockHash::noTotalEntries, Vector2i(vc, vr), p.sceneParams->viewFrustum_min,
                          p.sceneParams->viewFrustum_max);
        n_visible = vis.FindVisibleBlocks(&scene, Matrix4f::fromAffine(c2w.inv()), vi4, &rs);
        vis.CreateExpectedDepths(&scene, c2w.inv(), vi, &rs);
        vis.RenderImage(&scene, Matrix4f::fromAffine(c2w), vi4, &rs, engine_img);
        if (engine_img.cols() != vc || engine_img.rows() != vr) { std::fprintf(stderr, "RenderImage did not size by the view\n"); return 2; }
        // RENDER_FROM_OLD_RAYCAST on the bound state: the same picture from the view's raycast result
        cuda::image4u again;
        vis.RenderImage(&scene, Matrix4f::fromAffine(c2w), vi4, &rs, again, IVisualisationEngine::RENDER_SHADED_GREYSCALE,
                        IVisualisationEngine::RENDER_FROM_OLD_RAYCAST);
        if (fetch(again) != fetch(engine_img)) { std::fprintf(stderr, "old-raycast render differs\n"); return 2; }
    }   // the render state releases its view here, before the scene goes
    vis.RenderImage(&scene, Matrix4f::fromAffine(c2w), ti4, nullptr, own_after);
    if (fetch(own_before) != fetch(own_after)) { std::fprintf(stderr, "the scene's own render state changed\n"); return 2; }
    const std::vector<unsigned char> e = fetch(engine_img);
    io::writePPM(argv[7], e.data(), vc, vr);

    // ---- TopFu::renderView
    TopFu topfu(p);
    topfu.loadScene(path);
    cuda::image4u topfu_img;
    topfu.renderView(topfu_img, c2w, TopFu::RENDER_SHADED_GREYSCALE, vc, vr);
    const std::vector<unsigned char> t = fetch(topfu_img);
    io::writePPM(argv[8], t.data(), vc, vr);
    long lit = 0;
    for (size_t k = 0; k < t.size(); k += 4) lit += t[k] > 0;
    std::printf("view %dx%d: %d visible blocks, %ld pixels lit, engine == topfu: %s\n", vc, vr, n_visible, lit, e == t ? "yes" : "NO");
    return e == t && lit > 0 ? 0 : 2;
}
