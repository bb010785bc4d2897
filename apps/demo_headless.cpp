// demo_headless.cpp -- apps/demo.cpp's loop (tfusion/apps/demo.cpp:27-168) without OpenCV /
// OpenNI: depth frames are uploaded with cuda::Depth::upload, fused by TopFu::operator(), and
// the grey rendering is fetched with renderImage + download, exactly as the reference demo
// does.  Frames are either synthetic (the C2 orbit of SURVEY.md §8d, rendered analytically on
// the host) or read from a numbered 16-bit PGM sequence like the reference demo's
// "%04d.pgm" / "%04d.ppm" pairs (demo.cpp:91-97) through tfusion::io::FrameSequenceSource.
//
//   ./demo_headless [frames=100] [cols=640] [rows=480]
//   ./demo_headless --pgm 'dir/%04d.pgm' [--ppm 'dir/%04d.ppm'] [max_frames]
//   ... --mesh out.ply : the reconstructed surface after the last frame (TopFu::saveMesh)
//   ... --mesh-normals : with per-vertex normals (nx ny nz) in that PLY
//   ... --mesh-indexed : the indexed vertex table as the GPU extracts it, no host weld
//   ... --load-scene F : resume from the checkpoint F before the first frame (TopFu::loadScene)
//   ... --save-scene F : write the checkpoint F after the last frame (TopFu::saveScene)
//   ... --load-scene F --capacity BUCKETS,EXCESS,BLOCKS : resume in tables of these sizes, whatever F was saved
//                        with (TopFu::loadMapResized: the map is re-hashed on the way in)
//   ... --merge-scene F [--merge-offset bx,by,bz] : fuse the checkpoint F into the map before the first frame, after
//                        --load-scene, its blocks moved by that many whole blocks (TopFu::mergeMap); may be given
//                        more than once, each --merge-offset goes with the --merge-scene before it
//   ... --view-out F.ppm --view-pose tx,ty,tz,rx,ry,rz [--view-size CxR] : the final map from that camera -> world
//                        pose (translation in metres, rotation as a Rodrigues vector) at that size (default: the
//                        frames'), through a free view (TopFu::renderView), as a binary PPM.  With 0 frames and
//                        --load-scene: a saved map's picture and nothing else.
//   ... --view-whole   : that view reads the GlobalCache of a swapping map as well as the resident blocks
//   ... --slice-out F.pgm --slice-plane ox,oy,oz,ux,uy,uz,vx,vy,vz [--slice-size CxR] : a cross-section of the final
//                        map's TSDF (TopFu::slice): pixel (x, y) is the point o + x * u + y * v, in metres, at that
//                        size (default: the frames').  Grey = (unsigned char)((sdf + 1) * 127.5f), 0 where the
//                        confidence is 0 (nothing observed); a binary PGM.
//   ... --slice-whole  : the slice reads the GlobalCache of a swapping map as well
#include <tfusion/io.hpp>
#include <tfusion/topfu.hpp>

#include "synth_depth.hpp"

#include <cstring>
#include <string>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace tfusion;

int main(int argc, char** argv)
{
    std::string pgm, ppm, mesh, load_scene, save_scene, capacity, view_out, view_pose, view_size, slice_out, slice_plane, slice_size;
    bool mesh_normals = false, mesh_indexed = false, view_whole = false, slice_whole = false;
    std::vector<std::string> merge_scenes, merge_offsets;
    std::vector<const char*> pos;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--pgm") && i + 1 < argc) pgm = argv[++i];
        else if (!std::strcmp(argv[i], "--ppm") && i + 1 < argc) ppm = argv[++i];
        else if (!std::strcmp(argv[i], "--mesh") && i + 1 < argc) mesh = argv[++i];
        else if (!std::strcmp(argv[i], "--load-scene") && i + 1 < argc) load_scene = argv[++i];
        else if (!std::strcmp(argv[i], "--save-scene") && i + 1 < argc) save_scene = argv[++i];
        else if (!std::strcmp(argv[i], "--capacity") && i + 1 < argc) capacity = argv[++i];
        else if (!std::strcmp(argv[i], "--merge-scene") && i + 1 < argc) { merge_scenes.push_back(argv[++i]); merge_offsets.push_back(""); }
        else if (!std::strcmp(argv[i], "--merge-offset") && i + 1 < argc && !merge_scenes.empty()) merge_offsets.back() = argv[++i];
        else if (!std::strcmp(argv[i], "--view-out") && i + 1 < argc) view_out = argv[++i];
        else if (!std::strcmp(argv[i], "--view-pose") && i + 1 < argc) view_pose = argv[++i];
        else if (!std::strcmp(argv[i], "--view-size") && i + 1 < argc) view_size = argv[++i];
        else if (!std::strcmp(argv[i], "--mesh-normals")) mesh_normals = true;
        else if (!std::strcmp(argv[i], "--mesh-indexed")) mesh_indexed = true;
        else if (!std::strcmp(argv[i], "--view-whole")) view_whole = true;
        else if (!std::strcmp(argv[i], "--slice-out") && i + 1 < argc) slice_out = argv[++i];
        else if (!std::strcmp(argv[i], "--slice-plane") && i + 1 < argc) slice_plane = argv[++i];
        else if (!std::strcmp(argv[i], "--slice-size") && i + 1 < argc) slice_size = argv[++i];
        else if (!std::strcmp(argv[i], "--slice-whole")) slice_whole = true;
        else pos.push_back(argv[i]);
    }
    int frames = pos.size() > 0 ? std::atoi(pos[0]) : (pgm.empty() ? 100 : 1 << 30);
    int cols = pos.size() > 1 ? std::atoi(pos[1]) : 640;
    int rows = pos.size() > 2 ? std::atoi(pos[2]) : 480;
    io::FrameSequenceSource source(pgm, ppm);
    std::vector<unsigned short> depth;
    std::vector<unsigned char> image;
    bool have_first = false;
    if (!pgm.empty()) {                        // frame size from the first file
        if (!source.grab(depth, image)) { std::fprintf(stderr, "no frame %s\n", pgm.c_str()); return 1; }
        cols = source.cols(); rows = source.rows();
        have_first = true;
    }

    int device = 0;
    cuda::setDevice(device);
    cuda::printShortCudaDeviceInfo(device);
    if (cuda::checkIfPreFermiGPU(device)) return 1;

    TopFuParams params = TopFuParams::default_params();
    params.cols = cols;
    params.rows = rows;
    const double s = cols / 640.0;
    params.intr = Intr(504.261f * s, 503.905f * s, 352.457f * s, 272.202f * s);
    if (!capacity.empty() && (std::sscanf(capacity.c_str(), "%d,%d,%d", &params.n_buckets, &params.n_excess, &params.n_blocks) != 3 ||
                              load_scene.empty())) {
        std::fprintf(stderr, "--capacity BUCKETS,EXCESS,BLOCKS goes with --load-scene\n");
        return 1;
    }
    TopFu::Ptr topfu(new TopFu(params));
    auto scene_line = [](const char* what, const std::string& path) {
        const struct tf_scene_file_info info = TopFu::sceneFileInfo(path);
        std::printf("scene %s %s: %lld records, %lld blocks, %lld bytes\n", what, path.c_str(), info.n_records,
                    info.n_blocks_stored, info.file_bytes);
    };
    if (!load_scene.empty() && !capacity.empty()) {
        struct tf_resize_report rep;
        topfu->loadMapResized(load_scene, &rep);
        scene_line("loaded resized from", load_scene);
        std::printf("resized into %d buckets, %d excess, %d blocks: %lld records carried, %lld dropped, %lld blocks, %lld excess slots, "
                    "longest chain %d\n", params.n_buckets, params.n_excess, params.n_blocks, rep.records_carried, rep.records_dropped,
                    rep.blocks, rep.excess_used, rep.longest_chain);
    } else if (!load_scene.empty()) {
        topfu->loadScene(load_scene);
        scene_line("loaded from", load_scene);
    }
    for (size_t k = 0; k < merge_scenes.size(); ++k) {
        std::array<int, 3> off = { 0, 0, 0 };
        if (!merge_offsets[k].empty() && std::sscanf(merge_offsets[k].c_str(), "%d,%d,%d", &off[0], &off[1], &off[2]) != 3) {
            std::fprintf(stderr, "--merge-offset bx,by,bz\n");
            return 1;
        }
        struct tf_merge_report rep;
        topfu->mergeMap(merge_scenes[k], off, &rep);
        scene_line("merged from", merge_scenes[k]);
        std::printf("merged at block offset (%d %d %d): %lld records combined, %lld inserted, %lld revived, %lld skipped, %lld blocks, "
                    "%lld excess slots\n", off[0], off[1], off[2], rep.records_combined, rep.records_inserted, rep.records_revived,
                    rep.records_skipped, rep.blocks_used, rep.excess_used);
    }

    cuda::Depth depth_device;
    cuda::image4u view_device;
    std::vector<unsigned char> view_host((size_t)cols * rows * 4);
    double time_ms = 0;
    int n_ok = 0, n = 0;
    for (int i = 0; i < frames; ++i) {
        if (!pgm.empty()) {
            if (!have_first && !source.grab(depth, image)) break;         // end of the sequence
            have_first = false;
            if (source.cols() != cols || source.rows() != rows) { std::fprintf(stderr, "frame size changed\n"); return 1; }
        } else {
            double R[9], t[3];
            tfusion_apps::orbit_pose(i, R, t);
            tfusion_apps::render_depth(R, t, cols, rows, params.intr, depth);
        }
        ++n;
        depth_device.upload(depth.data(), (size_t)cols * 2, rows, cols);
        bool has_image;
        {
            SampledScopeTime fps(time_ms); (void)fps;
            has_image = (*topfu)(depth_device);
        }
        if (has_image) {
            ++n_ok;
            topfu->renderImage(view_device);
            view_device.download(view_host.data(), (size_t)cols * 4);
        }
    }
    const Affine3f pose = topfu->getCameraPose();
    const tf_stats st = topfu->stats();
    std::printf("frames %d ok %d resets %d visible %d  pose t = (%.4f %.4f %.4f)\n", n, n_ok, st.n_resets,
                st.noVisibleEntries, pose.translation()[0], pose.translation()[1], pose.translation()[2]);
    if (!save_scene.empty()) {
        topfu->saveScene(save_scene);
        scene_line("saved to", save_scene);
    }
    if (!mesh.empty()) {
        if (mesh_indexed) {
            topfu->saveMesh(mesh, TF_MESH_INDEXED | (mesh_normals ? TF_MESH_NORMALS : 0));
            // the same mesh through extractMeshIndexed: the file's vertices and faces, and no index past the table
            cuda::DeviceArray<float> vertices;
            cuda::DeviceArray<unsigned> indices;
            const long long nt = topfu->extractMeshIndexed(vertices, indices);
            std::vector<unsigned> idx;
            indices.download(idx);
            unsigned top = 0;
            for (unsigned i : idx) top = std::max(top, i);
            std::printf("indexed mesh: %zu vertices, %lld triangles, highest index %u\n", vertices.size() / 3, nt, top);
        }
        else if (mesh_normals) topfu->saveMesh(mesh, TF_MESH_NORMALS);
        else topfu->saveMesh(mesh);
        std::printf("mesh written to %s\n", mesh.c_str());
    }
    if (!view_out.empty()) {
        float p[6] = { 0, 0, 0, 0, 0, 0 };
        int vc = cols, vr = rows;
        if ((!view_pose.empty() && std::sscanf(view_pose.c_str(), "%f,%f,%f,%f,%f,%f", &p[0], &p[1], &p[2], &p[3], &p[4], &p[5]) != 6) ||
            (!view_size.empty() && std::sscanf(view_size.c_str(), "%dx%d", &vc, &vr) != 2)) {
            std::fprintf(stderr, "--view-pose tx,ty,tz,rx,ry,rz  --view-size CxR\n");
            return 1;
        }
        cuda::image4u free_view;
        topfu->renderView(free_view, Affine3f(Vec3f(p[3], p[4], p[5]), Vec3f(p[0], p[1], p[2])), TopFu::RENDER_SHADED_GREYSCALE, vc, vr,
                          view_whole);
        std::vector<unsigned char> px((size_t)vc * vr * 4);
        free_view.download(px.data(), (size_t)vc * 4);
        io::writePPM(view_out, px.data(), vc, vr);
        long view_lit = 0;
        for (size_t k = 0; k < px.size(); k += 4) view_lit += px[k] > 0;
        std::printf("free view %dx%d written to %s: %ld pixels lit\n", vc, vr, view_out.c_str(), view_lit);
        if (frames == 0 && slice_out.empty()) return 0;
    }
    if (!slice_out.empty()) {
        float q[9];
        int sc = cols, sr = rows;
        if (std::sscanf(slice_plane.c_str(), "%f,%f,%f,%f,%f,%f,%f,%f,%f", &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], &q[6], &q[7], &q[8]) != 9 ||
            (!slice_size.empty() && std::sscanf(slice_size.c_str(), "%dx%d", &sc, &sr) != 2) || sc <= 0 || sr <= 0) {
            std::fprintf(stderr, "--slice-plane ox,oy,oz,ux,uy,uz,vx,vy,vz  --slice-size CxR\n");
            return 1;
        }
        const size_t n = (size_t)sc * sr;
        cuda::DeviceArray<float> sdf(n), conf(n);
        tf_query_out out = {};
        out.sdf = sdf.ptr();
        out.confidence = conf.ptr();
        topfu->slice(q, q + 3, q + 6, sc, sr, TF_QUERY_METRES, slice_whole, out);
        std::vector<float> hs, hc;
        sdf.download(hs);
        conf.download(hc);
        std::vector<unsigned char> grey(n);
        long seen = 0;
        for (size_t k = 0; k < n; ++k) {               // the mapping is the host's: the library returns the TSDF itself
            grey[k] = hc[k] == 0.0f ? (unsigned char)0 : (unsigned char)((hs[k] + 1.0f) * 127.5f);
            seen += hc[k] != 0.0f;
        }
        io::writePGM8(slice_out, grey.data(), sc, sr);
        std::printf("slice %dx%d written to %s: %ld pixels observed\n", sc, sr, slice_out.c_str(), seen);
        if (frames == 0) return 0;
    }
    long lit = 0;
    for (size_t k = 0; k < view_host.size(); k += 4) lit += view_host[k] > 0;
    std::printf("rendered pixels lit: %ld of %d\n", lit, cols * rows);
    return n_ok > 0 && lit > 0 ? 0 : 2;
}
