// ref_pin_stages.cpp -- TEST INFRASTRUCTURE.  Runs the reference's OWN shared per-element functions
// (the _CPU_AND_GPU_CODE_ inline functions of tfusion/cuda/RepresentationAccess.hpp,
// VisualisationEngine_Shared.hpp and SceneReconstructionEngine.hpp, compiled for the host straight
// from the reference tree) over the scenes of tests/pin_scenes.py and writes the golden files
// tests/golden/stage_pin_<scene>_<case>.bin that pin the CPU oracle's stage functions and, through
// tests/test_gpu_stage_pin.py, the HIP kernels.  Built by oracle/Makefile (target ref) into
// oracle/_ref/ with the declaration-only stand-ins of tests/cvstub (OpenCV) and
// oracle/ref_pin/cuda_standin (CUDA); every computed bit comes from the reference's own text.
//
//   ref_pin_stages <input pin file of one scene> <output directory> <scene name>
//
// Of each __global__ body only the few lines that form the arguments are restated here, each with
// its .cu / .hpp lines.  File format and array layouts: tests/pin_scenes.py and
// tests/test_oracle_stage_pin.py.
#include "tfusion/cuda/RepresentationAccess.hpp"
#include "tfusion/cuda/VisualisationEngine_Shared.hpp"
#ifndef REF_PIN_NO_SCENE_ENGINE      // (its CUDAUtils.hpp needs clang's HIP mode; without it the integrate, alloc_pp and visibility cases are left out)
#include "tfusion/cuda/SceneReconstructionEngine.hpp"
#endif
#include "tfusion/cuda/VoxelTypes.hpp"
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

using tfusion::VoxelBlockHash;

#ifndef REF_PIN_SIZEOF_VOXEL_S_RGB
#define REF_PIN_SIZEOF_VOXEL_S_RGB 8       // what tests/golden/ref_pin_colour.bin records (its first float)
#endif
static_assert(sizeof(HashEntry) == 16, "HashEntry layout");
static_assert(sizeof(Voxel_s) == 4, "Voxel_s layout");
static_assert(sizeof(Voxel_s_rgb) == REF_PIN_SIZEOF_VOXEL_S_RGB, "Voxel_s_rgb layout");
static_assert(std::is_same<decltype(sqrt(1.0f)), float>::value, "sqrt(float) must be the float overload");
static_assert(std::is_same<decltype(floor(1.0f)), float>::value, "floor(float) must be the float overload");
static_assert(std::is_same<decltype(ceil(1.0f)), float>::value, "ceil(float) must be the float overload");
static_assert(SDF_BUCKET_NUM == 0x100000 && SDF_EXCESS_LIST_SIZE == 0x20000, "the scenes' hash sizes");

// ---- pin files (tests/pin_scenes.py) ----------------------------------------------------------------
enum { T_U8, T_I16, T_I32, T_U32, T_F32 };
static const size_t k_size[5] = { 1, 2, 4, 4, 4 };
struct Arr { int code; size_t count; std::vector<char> data; };
typedef std::vector<std::pair<std::string, Arr> > Out;

static void die(const char* what) { fprintf(stderr, "ref_pin_stages: %s\n", what); exit(1); }

static std::map<std::string, Arr> read_pin(const char* path)
{
    std::map<std::string, Arr> m;
    FILE* f = fopen(path, "rb");
    if (!f) die("cannot open the input file");
    char magic[8]; uint32_t n;
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "TFPIN1\0\0", 8) || fread(&n, 4, 1, f) != 1) die("bad input file");
    for (uint32_t i = 0; i < n; ++i) {
        char name[25] = { 0 }; uint32_t hdr[2];
        if (fread(name, 1, 24, f) != 24 || fread(hdr, 4, 2, f) != 2 || hdr[0] > 4) die("bad array header");
        Arr a; a.code = (int)hdr[0]; a.count = hdr[1];
        a.data.resize((a.count * k_size[a.code] + 3) & ~(size_t)3);
        if (a.data.size() && fread(a.data.data(), 1, a.data.size(), f) != a.data.size()) die("short array");
        m[name] = a;
    }
    fclose(f);
    return m;
}

static void write_pin(const std::string& path, const Out& out)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) die("cannot open an output file");
    uint32_t n = (uint32_t)out.size();
    fwrite("TFPIN1\0\0", 1, 8, f); fwrite(&n, 4, 1, f);
    for (size_t i = 0; i < out.size(); ++i) {
        char name[24] = { 0 };
        strncpy(name, out[i].first.c_str(), 23);
        uint32_t hdr[2] = { (uint32_t)out[i].second.code, (uint32_t)out[i].second.count };
        fwrite(name, 1, 24, f); fwrite(hdr, 4, 2, f);
        if (out[i].second.data.size()) fwrite(out[i].second.data.data(), 1, out[i].second.data.size(), f);
    }
    fclose(f);
}

template<class T> static void put(Out& o, const char* name, int code, const std::vector<T>& v)
{
    if (sizeof(T) != k_size[code]) die("array type");
    Arr a; a.code = code; a.count = v.size();
    a.data.assign((v.size() * sizeof(T) + 3) & ~(size_t)3, 0);
    if (v.size()) memcpy(a.data.data(), v.data(), v.size() * sizeof(T));
    o.push_back(std::make_pair(std::string(name), a));
}

template<class T> static const T* get(const std::map<std::string, Arr>& m, const char* name, size_t count = 0)
{
    std::map<std::string, Arr>::const_iterator it = m.find(name);
    if (it == m.end() || sizeof(T) != k_size[it->second.code] || (count && it->second.count != count)) {
        fprintf(stderr, "input array %s\n", name); die("missing or wrong input array");
    }
    return (const T*)it->second.data.data();
}
static size_t count_of(const std::map<std::string, Arr>& m, const char* name) { return m.find(name)->second.count; }

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// [R|t] row-major, as the API takes a pose -> Matrix4f, as the engines load an Affine3f
// (SceneReconstructionEngine_host.cu:212-215, VisualisationEngine_CUDA.cu:137-140: column by column)
static Matrix4f load_rt(const float* rt)
{
    return Matrix4f(rt[0], rt[4], rt[8], 0.f, rt[1], rt[5], rt[9], 0.f, rt[2], rt[6], rt[10], 0.f, rt[3], rt[7], rt[11], 1.f);
}

// counters only: where a block position sits in the hash table -- 0 no entry, 1 swapped out (ptr -1),
// 2 allocated in a bucket entry, 3 allocated in an excess entry (the walk of findVoxel, any ptr)
static int block_state(const HashEntry* hash, const Vector3i& b)
{
    int idx = hashIndex(b), swapped = 0;
    while (true) {
        const HashEntry& e = hash[idx];
        if (IS_EQUAL3(e.pos, b)) {
            if (e.ptr >= 0) return idx < SDF_BUCKET_NUM ? 2 : 3;
            if (e.ptr == -1) swapped = 1;
        }
        if (e.offset < 1) break;
        idx = SDF_BUCKET_NUM + e.offset - 1;
    }
    return swapped;
}

// counters only: castRay's march (VisualisationEngine_Shared.hpp:110-153) walked again beside the call, with
// the reference's own reads, to count the steps in missing blocks and the interpolated reads; returns
// whether the ray ends on sdf <= 0, which must agree with castRay's result
static bool march_counts(int x, int y, const Voxel_s* vox, const HashEntry* hash, const Matrix4f& invM, const Vector4f& invProj,
                         float oneOverVoxelSize, float mu, const Vector2f& range, int& missing, int& interpolated)
{
    Vector4f c; Vector3f s, e;
    const float stepScale = mu * oneOverVoxelSize;
    c.z = range.x; c.x = c.z * ((float(x) + invProj.z) * invProj.x); c.y = c.z * ((float(y) + invProj.w) * invProj.y); c.w = 1.0f;
    float totalLength = length(TO_VECTOR3(c)) * oneOverVoxelSize;
    s = TO_VECTOR3(invM * c) * oneOverVoxelSize;
    c.z = range.y; c.x = c.z * ((float(x) + invProj.z) * invProj.x); c.y = c.z * ((float(y) + invProj.w) * invProj.y); c.w = 1.0f;
    const float totalLengthMax = length(TO_VECTOR3(c)) * oneOverVoxelSize;
    e = TO_VECTOR3(invM * c) * oneOverVoxelSize;
    Vector3f dir = e - s;
    dir *= 1.0f / sqrt(dir.x * dir.x + dir.y * dir.y + dir.z * dir.z);
    Vector3f pt = s; float sdfValue = 1.0f, stepLength; int vmIndex;
    VoxelBlockHash::IndexCache cache;
    missing = interpolated = 0;
    while (totalLength < totalLengthMax) {
        sdfValue = readFromSDF_float_uninterpolated(vox, hash, pt, vmIndex, cache);
        if (!vmIndex) { stepLength = SDF_BLOCK_SIZE; missing++; }
        else {
            if ((sdfValue <= 0.1f) && (sdfValue >= -0.5f)) { sdfValue = readFromSDF_float_interpolated(vox, hash, pt, vmIndex, cache); interpolated++; }
            if (sdfValue <= 0.0f) break;
            stepLength = MAX(sdfValue * stepScale, 1.0f);
        }
        pt += stepLength * dir; totalLength += stepLength;
    }
    return sdfValue <= 0.0f;
}

struct Scene {
    const HashEntry* hash;
    std::vector<Voxel_s> vba;
    std::vector<Voxel_s_rgb> vba_rgb;
    Vector4f proj; float mu, voxelSize, vf_min, vf_max;
    Vector2i imgSize; int maxW;
    std::vector<uint32_t> crc;
};

int main(int argc, char** argv)
{
    if (argc != 4) die("usage: ref_pin_stages <input> <output directory> <scene>");
    const std::map<std::string, Arr> in = read_pin(argv[1]);
    const std::string prefix = std::string(argv[2]) + "/stage_pin_" + argv[3] + "_";
    Scene S;
    const size_t n_total = SDF_BUCKET_NUM + SDF_EXCESS_LIST_SIZE;
    S.hash = (const HashEntry*)get<uint8_t>(in, "hash", n_total * 16);
    const size_t n_vox = count_of(in, "vba") / 4;
    {
        const uint8_t* raw = get<uint8_t>(in, "vba");
        const uint32_t* clr = get<uint32_t>(in, "vba_rgb", n_vox);
        S.vba.resize(n_vox); S.vba_rgb.resize(n_vox);
        for (size_t i = 0; i < n_vox; ++i) {
            int16_t sdf; memcpy(&sdf, raw + 4 * i, 2);
            S.vba[i].sdf = sdf; S.vba[i].w_depth = raw[4 * i + 2];
            S.vba_rgb[i].sdf = sdf; S.vba_rgb[i].w_depth = raw[4 * i + 2];
            S.vba_rgb[i].clr = Vector3u((uchar)(clr[i] & 255), (uchar)((clr[i] >> 8) & 255), (uchar)((clr[i] >> 16) & 255));
            S.vba_rgb[i].w_color = (uchar)(clr[i] >> 24);
        }
    }
    const float* fp = get<float>(in, "fparams", 8);
    const int32_t* ip = get<int32_t>(in, "iparams", 3);
    S.proj = Vector4f(fp[0], fp[1], fp[2], fp[3]); S.mu = fp[4]; S.voxelSize = fp[5]; S.vf_min = fp[6]; S.vf_max = fp[7];
    S.imgSize = Vector2i(ip[0], ip[1]); S.maxW = ip[2];
    const int W = ip[0], H = ip[1];
    S.crc.assign(get<uint32_t>(in, "crc", 3), get<uint32_t>(in, "crc", 3) + 3);
    const Voxel_s* vox = S.vba.data();
    const Voxel_s_rgb* vox_rgb = S.vba_rgb.data();

    // ---- (a) sdf_read: RepresentationAccess.hpp's reads at given points, with a fresh IndexCache
    //      and with one carried along the point sequence
    {
        const size_t n = count_of(in, "sdf_points") / 3;
        const float* p = get<float>(in, "sdf_points");
        std::vector<float> uninterp(2 * n), interp(2 * n), conf_sdf(2 * n), conf(2 * n), normal(3 * n);
        std::vector<uint8_t> colour(4 * n);
        std::vector<int32_t> vm(2 * n), counts(11, 0);
        VoxelBlockHash::IndexCache cu, ci, cc;
        for (size_t i = 0; i < n; ++i) {
            const Vector3f pt(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
            int v;
            { VoxelBlockHash::IndexCache c; uninterp[2 * i] = readFromSDF_float_uninterpolated(vox, S.hash, pt, v, c); vm[2 * i] = v; }
            uninterp[2 * i + 1] = readFromSDF_float_uninterpolated(vox, S.hash, pt, v, cu); vm[2 * i + 1] = v;
            { VoxelBlockHash::IndexCache c; interp[2 * i] = readFromSDF_float_interpolated(vox, S.hash, pt, v, c); }
            interp[2 * i + 1] = readFromSDF_float_interpolated(vox, S.hash, pt, v, ci);
            { VoxelBlockHash::IndexCache c; conf_sdf[2 * i] = readWithConfidenceFromSDF_float_interpolated(conf[2 * i], vox, S.hash, pt, v, c); }
            conf_sdf[2 * i + 1] = readWithConfidenceFromSDF_float_interpolated(conf[2 * i + 1], vox, S.hash, pt, v, cc);
            const Vector3f nr = computeSingleNormalFromSDF(vox, S.hash, pt);
            normal[3 * i] = nr.x; normal[3 * i + 1] = nr.y; normal[3 * i + 2] = nr.z;
            // drawPixelColour and the colour read it uses (VisualisationEngine_Shared.hpp:312-322)
            Vector4u cl((uchar)0);
            drawPixelColour<Voxel_s_rgb, VoxelBlockHash>(cl, pt, vox_rgb, S.hash);
            colour[4 * i] = cl.x; colour[4 * i + 1] = cl.y; colour[4 * i + 2] = cl.z; colour[4 * i + 3] = cl.w;
            // branch counts: where the point's own voxel and its +1 neighbours were found
            Vector3f coeff; Vector3i pos; TO_INT_FLOOR3(pos, coeff, pt);
            int found8 = 0, other_block = 0, nb_state[4] = { 0, 0, 0, 0 };
            Vector3i b0; pointToVoxelBlockPos(pos, b0);
            for (int k = 0; k < 8; ++k) {
                const Vector3i q = pos + Vector3i(k & 1, (k >> 1) & 1, k >> 2);
                Vector3i b; pointToVoxelBlockPos(q, b);
                bool f; findVoxel(S.hash, q, f);
                found8 += f; other_block += !IS_EQUAL3(b, b0);
                if (!IS_EQUAL3(b, b0)) nb_state[block_state(S.hash, b)]++;
            }
            counts[0] += vm[2 * i] == 0;                                        // missing block
            counts[1] += vm[2 * i] > 0 && vm[2 * i] <= SDF_BUCKET_NUM;          // found in a bucket entry
            counts[2] += vm[2 * i] > SDF_BUCKET_NUM;                            // found in an excess entry
            counts[3] += vm[2 * i + 1] == 1 && vm[2 * i] != 1;                  // the carried cache hit
            counts[4] += other_block > 0 && found8 == 8;                        // neighbours in another block, all present
            counts[5] += other_block > 0 && found8 > 0 && found8 < 8;           // some neighbours missing
            counts[6] += pt.x < 0 || pt.y < 0 || pt.z < 0;                      // negative coordinates
            counts[7] += coeff.x == 0 && coeff.y == 0 && coeff.z == 0;          // exact integers
            counts[8] += nb_state[0] > 0;                                       // a +1 neighbour in a block with no entry
            counts[9] += nb_state[1] > 0;                                       // ... in a swapped-out block
            counts[10] += nb_state[3] > 0;                                      // ... in a block chained in an excess entry
        }
        Out o;
        put(o, "crc", T_U32, S.crc); put(o, "counts", T_I32, counts);
        put(o, "uninterp", T_F32, uninterp); put(o, "vm", T_I32, vm); put(o, "interp", T_F32, interp);
        put(o, "conf_sdf", T_F32, conf_sdf); put(o, "conf", T_F32, conf); put(o, "normal", T_F32, normal);
        put(o, "colour", T_U8, colour);
        write_pin(prefix + "sdf_read.bin", o);
    }

    // ---- (b) raycast: genericRaycast_device (VisualisationHelper.hpp:38-45) per pixel, both
    //      instantiations GenericRaycast launches (VisualisationEngine_CUDA.cu:176-217)
    std::vector<Vector4f> rays_a;
    {
        const Vector2f* minmaximg = (const Vector2f*)get<float>(in, "range", (size_t)W * H * 2);
        const float oneOverVoxelSize = 1.0f / S.voxelSize;                       // VisualisationEngine_CUDA.cu:179
        const Vector4f invProj = InvertProjectionParams(S.proj);                 // :197
        Out o;
        put(o, "crc", T_U32, S.crc);
        std::vector<int32_t> counts;
        for (int pose = 0; pose < 2; ++pose) {
            const Matrix4f invM = load_rt(get<float>(in, pose ? "c2w_b" : "c2w_a", 12));
            std::vector<Vector4f> pts((size_t)W * H), pts_v((size_t)W * H);
            std::vector<uchar> visType(n_total, 0);
            int found = 0, degenerate = 0, rays_missing = 0, rays_interp = 0;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const int locId = x + y * W;
                    const int locId2 = (int)floor((float)x / minmaximg_subsample) + (int)floor((float)y / minmaximg_subsample) * W;
                    const bool f0 = castRay<Voxel_s, VoxelBlockHash, false>(pts[locId], NULL, x, y, vox, S.hash, invM, invProj,
                                                                           oneOverVoxelSize, S.mu, minmaximg[locId2]);
                    const bool f1 = castRay<Voxel_s, VoxelBlockHash, true>(pts_v[locId], visType.data(), x, y, vox, S.hash, invM, invProj,
                                                                          oneOverVoxelSize, S.mu, minmaximg[locId2]);
                    if (f0 != f1 || memcmp(&pts[locId], &pts_v[locId], 16)) die("castRay<true> and <false> differ");
                    found += f0; degenerate += !(minmaximg[locId2].x < minmaximg[locId2].y);
                    int n_missing, n_interp;
                    if (march_counts(x, y, vox, S.hash, invM, invProj, oneOverVoxelSize, S.mu, minmaximg[locId2], n_missing, n_interp) != f0)
                        die("the counted march and castRay disagree");
                    rays_missing += n_missing > 0; rays_interp += n_interp > 0;
                }
            std::vector<uint32_t> vis;
            for (size_t i = 0; i < n_total; ++i) if (visType[i]) { if (visType[i] != 1) die("visible type"); vis.push_back((uint32_t)i); }
            std::vector<float> flat((size_t)W * H * 4);
            memcpy(flat.data(), pts.data(), flat.size() * 4);
            put(o, pose ? "points_b" : "points_a", T_F32, flat);
            put(o, pose ? "visible_b" : "visible_a", T_U32, vis);
            counts.push_back(found); counts.push_back(W * H - found); counts.push_back(degenerate); counts.push_back((int)vis.size());
            counts.push_back(rays_missing); counts.push_back(rays_interp);
            if (!pose) rays_a = pts;
        }
        put(o, "counts", T_I32, counts);      // per pose: found, missed, rays with min >= max, entries marked visible, rays with
                                              // steps in missing blocks, rays that took the march's interpolated read
        write_pin(prefix + "raycast.bin", o);
    }

#ifndef REF_PIN_NO_SCENE_ENGINE
    // ---- (c) integrate: integrateIntoScene_device<TVoxel, false> (SceneReconstructionEngine_host.cu:
    //      297-329; IntegrateIntoScene launches <false> as stopIntegratingAtMaxW is false, :234-249 and
    //      topfu.cpp:50), and the colour update under ComputeUpdatedVoxelInfo<true, ...>'s gate
    //      (SceneReconstructionEngine.hpp:172-174, commented out there) on a Voxel_s_rgb copy
    {
        Out o;
        put(o, "crc", T_U32, S.crc);
        const Vector4u* rgb = (const Vector4u*)get<uint8_t>(in, "rgb", (size_t)W * H * 4);
        std::vector<int32_t> counts;
        for (int frame = 0; frame < 3; ++frame) {
            const std::string fr(1, (char)('0' + frame));
            const Matrix4f M_d = load_rt(get<float>(in, ("int_pose" + fr).c_str(), 12));
            const float* depth = get<float>(in, ("int_dists" + fr).c_str(), (size_t)W * H);
            const std::string vis_name = "int_vis" + fr;
            const char* vname = vis_name.c_str();
            const int32_t* visibleEntryIDs = get<int32_t>(in, vname);
            const int noVisibleEntries = (int)count_of(in, vname);
            std::vector<Voxel_s> vba(S.vba);
            std::vector<Voxel_s_rgb> vba_c(S.vba_rgb);
            int c_skipped = 0, c_behind = 0, c_outside = 0, c_nodepth = 0, c_edge = 0, c_far = 0, c_updated = 0, c_eq = 0, c_clamped = 0, c_maxw = 0, c_colour = 0;
            for (int e = 0; e < noVisibleEntries; ++e) {
                const HashEntry& currentHashEntry = S.hash[visibleEntryIDs[e]];
                if (currentHashEntry.ptr < 0) { c_skipped++; continue; }                       // :307
                const Vector3i globalPos = currentHashEntry.pos.toInt() * SDF_BLOCK_SIZE;      // :309
                Voxel_s* localVoxelBlock = &vba[(size_t)currentHashEntry.ptr * SDF_BLOCK_SIZE3];
                Voxel_s_rgb* localColourBlock = &vba_c[(size_t)currentHashEntry.ptr * SDF_BLOCK_SIZE3];
                for (int z = 0; z < SDF_BLOCK_SIZE; ++z) for (int y = 0; y < SDF_BLOCK_SIZE; ++y) for (int x = 0; x < SDF_BLOCK_SIZE; ++x) {
                    const int locId = x + y * SDF_BLOCK_SIZE + z * SDF_BLOCK_SIZE * SDF_BLOCK_SIZE;
                    Vector4f pt_model;
                    pt_model.x = (float)(globalPos.x + x) * S.voxelSize;                       // :322-325
                    pt_model.y = (float)(globalPos.y + y) * S.voxelSize;
                    pt_model.z = (float)(globalPos.z + z) * S.voxelSize;
                    pt_model.w = 1.0f;
                    const Voxel_s before = localVoxelBlock[locId];
                    ComputeUpdatedVoxelInfo<false, false, Voxel_s>::compute(localVoxelBlock[locId], pt_model, M_d, S.proj, S.mu, S.maxW,
                                                                            depth, S.imgSize);
                    Voxel_s_rgb& cv = localColourBlock[locId];
                    const float eta = computeUpdatedVoxelDepthInfo(cv, pt_model, M_d, S.proj, S.mu, S.maxW, depth, S.imgSize);
                    if (cv.sdf != localVoxelBlock[locId].sdf || cv.w_depth != localVoxelBlock[locId].w_depth) die("Voxel_s and Voxel_s_rgb depth updates differ");
                    const bool changed = before.sdf != cv.sdf || before.w_depth != cv.w_depth;
                    const Vector4f pt_camera = M_d * pt_model;
                    if (pt_camera.z <= 0) c_behind++;
                    else if (eta == -1) {
                        // which early return: the projection of :35-37 formed again
                        const float ix = S.proj.x * pt_camera.x / pt_camera.z + S.proj.z, iy = S.proj.y * pt_camera.y / pt_camera.z + S.proj.w;
                        if ((ix < 1) || (ix > S.imgSize.x - 2) || (iy < 1) || (iy > S.imgSize.y - 2)) c_outside++; else c_nodepth++;
                    }
                    else if (eta < -S.mu) c_far++;
                    else {
                        const float ix = S.proj.x * pt_camera.x / pt_camera.z + S.proj.z, iy = S.proj.y * pt_camera.y / pt_camera.z + S.proj.w;
                        c_edge += ix == 1 || iy == 1 || ix == S.imgSize.x - 2 || iy == S.imgSize.y - 2;
                        c_updated++; c_eq += eta == -S.mu; c_clamped += eta / S.mu > 1; c_maxw += before.w_depth == S.maxW;
                        if (!changed && before.w_depth != S.maxW) die("an updated voxel kept its weight");
                    }
                    if ((eta > S.mu) || (fabs(eta / S.mu) > 0.25f)) continue;
                    c_colour++;
                    computeUpdatedVoxelColorInfo(cv, pt_model, M_d, S.proj, S.mu, (uchar)S.maxW, eta, rgb, S.imgSize);
                }
            }
            std::vector<uint32_t> idx, word, cidx, cword;
            for (size_t i = 0; i < n_vox; ++i) {
                if (vba[i].sdf != S.vba[i].sdf || vba[i].w_depth != S.vba[i].w_depth) {
                    idx.push_back((uint32_t)i); word.push_back((uint32_t)(uint16_t)vba[i].sdf | ((uint32_t)vba[i].w_depth << 16));
                }
                const Voxel_s_rgb &a = vba_c[i], &b = S.vba_rgb[i];
                if (a.clr.x != b.clr.x || a.clr.y != b.clr.y || a.clr.z != b.clr.z || a.w_color != b.w_color) {
                    cidx.push_back((uint32_t)i);
                    cword.push_back((uint32_t)a.clr.x | ((uint32_t)a.clr.y << 8) | ((uint32_t)a.clr.z << 16) | ((uint32_t)a.w_color << 24));
                }
            }
            put(o, ("voxel_idx" + fr).c_str(), T_U32, idx); put(o, ("voxel" + fr).c_str(), T_U32, word);
            put(o, ("colour_idx" + fr).c_str(), T_U32, cidx); put(o, ("colour" + fr).c_str(), T_U32, cword);
            const int c[] = { c_skipped, c_behind, c_outside, c_nodepth, c_far, c_updated, c_eq, c_clamped, c_maxw, c_colour, (int)cidx.size(), c_edge };
            counts.insert(counts.end(), c, c + 12);
        }
        // per frame: list entries with ptr < 0, voxels behind the camera, outside the image, on no depth,
        // eta < -mu, updated, eta == -mu, eta / mu > 1, already at maxW, colour gate passed, colours changed,
        // updated with pt_image exactly on the window's edge (1, W - 2, H - 2)
        put(o, "counts", T_I32, counts);
        write_pin(prefix + "integrate.bin", o);
    }

    // ---- (d) alloc_pp: buildHashAllocAndVisibleType_device (SceneReconstructionEngine_host.cu:331-341) per
    //      pixel, with the arguments AllocateSceneFromDepth forms (:94-113, :138); the pixel loop runs
    //      forwards and backwards, and the arrays must not depend on the order
    {
        const Matrix4f M_d = load_rt(get<float>(in, "alloc_pose", 12));
        Matrix4f invM_d; M_d.inv(invM_d);                                            // :102-103
        Vector4f invProjParams_d = S.proj;                                           // :110-113
        invProjParams_d.x = 1.0f / invProjParams_d.x;
        invProjParams_d.y = 1.0f / invProjParams_d.y;
        const float oneOverVoxelSize = 1.0f / (S.voxelSize * SDF_BLOCK_SIZE);        // :138
        const float* depth = get<float>(in, "alloc_dists", (size_t)W * H);
        std::vector<uchar> allocType[2], visType[2]; std::vector<Vector4s> coords[2];
        for (int dir = 0; dir < 2; ++dir) {
            allocType[dir].assign(n_total, 0); visType[dir].assign(n_total, 0); coords[dir].assign(n_total, Vector4s((short)0));
            for (int k = 0; k < W * H; ++k) {
                const int locId = dir ? W * H - 1 - k : k;
                buildHashAllocAndVisibleTypePP(allocType[dir].data(), visType[dir].data(), locId % W, locId / W, coords[dir].data(), depth,
                                               invM_d, invProjParams_d, S.mu, S.imgSize, oneOverVoxelSize, S.hash, S.vf_min, S.vf_max);
            }
        }
        if (allocType[0] != allocType[1] || visType[0] != visType[1] || memcmp(coords[0].data(), coords[1].data(), n_total * sizeof(Vector4s))) {
            // name the pixels whose writes collide, so that the input can be changed (tests/pin_scenes.py, ALLOC_DROP)
            std::vector<uchar> a(n_total), v(n_total); std::vector<Vector4s> bc(n_total);
            std::map<size_t, std::pair<int, Vector4s> > owner;
            for (int k = 0; k < W * H; ++k) {
                if (!(depth[k] > 0)) continue;
                std::fill(a.begin(), a.end(), 0); std::fill(v.begin(), v.end(), 0); std::fill(bc.begin(), bc.end(), Vector4s((short)0));
                buildHashAllocAndVisibleTypePP(a.data(), v.data(), k % W, k / W, bc.data(), depth, invM_d, invProjParams_d, S.mu, S.imgSize,
                                               oneOverVoxelSize, S.hash, S.vf_min, S.vf_max);
                for (size_t i = 0; i < n_total; ++i) {
                    if (!a[i]) continue;
                    if (!owner.count(i)) owner[i] = std::make_pair(k, bc[i]);
                    else if (memcmp(&owner[i].second, &bc[i], sizeof(Vector4s))) fprintf(stderr, "alloc_pp: pixels %d and %d request different blocks in entry %zu\n", owner[i].first, k, i);
                }
            }
            die("alloc_pp: the request arrays depend on the pixel order for this input");
        }
        std::vector<uint32_t> idx; std::vector<uint8_t> flags; std::vector<int16_t> bc;
        std::vector<int32_t> counts(11, 0);
        for (size_t i = 0; i < n_total; ++i) {
            const Vector4s& b = coords[0][i];
            if (!allocType[0][i] && !visType[0][i] && !b.x && !b.y && !b.z && !b.w) continue;
            idx.push_back((uint32_t)i); flags.push_back(allocType[0][i]); flags.push_back(visType[0][i]);
            bc.push_back(b.x); bc.push_back(b.y); bc.push_back(b.z); bc.push_back(b.w);
            counts[0] += allocType[0][i] == 1; counts[1] += allocType[0][i] == 2;
            counts[2] += visType[0][i] == 1 && !allocType[0][i]; counts[3] += visType[0][i] == 2;
            counts[4] += visType[0][i] && i >= SDF_BUCKET_NUM;                        // found in an excess entry
            counts[5] += allocType[0][i] && (b.x < 0 || b.y < 0);                     // requests at negative block coordinates
        }
        for (int k = 0; k < W * H; ++k) {
            const float d = depth[k];
            counts[6] += d <= 0; counts[7] += d > 0 && (d - S.mu) < S.vf_min; counts[8] += d > 0 && (d + S.mu) > S.vf_max;
            if (d <= 0 || (d - S.mu) < 0 || (d - S.mu) < S.vf_min || (d + S.mu) > S.vf_max) continue;
            // counters only: noSteps of SceneReconstructionEngine.hpp:223-239 formed again (noSteps == 1 would divide by zero)
            Vector4f c; c.z = d; c.x = c.z * ((float(k % W) - invProjParams_d.z) * invProjParams_d.x); c.y = c.z * ((float(k / W) - invProjParams_d.w) * invProjParams_d.y);
            float norm = sqrt(c.x * c.x + c.y * c.y + c.z * c.z);
            Vector4f b1 = c * (1.0f - S.mu / norm); b1.w = 1.0f;
            Vector4f b2 = c * (1.0f + S.mu / norm); b2.w = 1.0f;
            const Vector3f dir = TO_VECTOR3(invM_d * b2) * oneOverVoxelSize - TO_VECTOR3(invM_d * b1) * oneOverVoxelSize;
            norm = sqrt(dir.x * dir.x + dir.y * dir.y + dir.z * dir.z);
            counts[9]++; counts[10] += (int)ceil(2.0f * norm) == 1;
        }
        Out o;
        // counts: entries with alloc type 1, type 2, found visible (type 1), found swapped out (type 2), found in an
        // excess entry, requests at negative block coordinates; pixels with depth <= 0, under the near limit, over the far limit,
        // pixels walked, of them with noSteps == 1
        put(o, "crc", T_U32, S.crc); put(o, "counts", T_I32, counts);
        put(o, "entry_idx", T_U32, idx); put(o, "entry_flags", T_U8, flags); put(o, "entry_coords", T_I16, bc);
        write_pin(prefix + "alloc_pp.bin", o);
    }

    // ---- (e) visibility: checkBlockVisibility<false> and <true> (SceneReconstructionEngine.hpp:325-375) as
    //      buildVisibleList_device calls them (SceneReconstructionEngine_host.cu:434-479)
    {
        const size_t n = count_of(in, "vis_blocks") / 3;
        const int16_t* b = get<int16_t>(in, "vis_blocks");
        const Matrix4f M_d = load_rt(get<float>(in, "w2c_b", 12));
        std::vector<uint8_t> flags(4 * n);
        std::vector<int32_t> counts(4, 0);
        for (size_t i = 0; i < n; ++i) {
            const Vector3s pos(b[3 * i], b[3 * i + 1], b[3 * i + 2]);
            bool v0, e0, v1, e1;
            checkBlockVisibility<false>(v0, e0, pos, M_d, S.proj, S.voxelSize, S.imgSize);
            checkBlockVisibility<true>(v1, e1, pos, M_d, S.proj, S.voxelSize, S.imgSize);
            flags[4 * i] = v0; flags[4 * i + 1] = e0; flags[4 * i + 2] = v1; flags[4 * i + 3] = e1;
            counts[0] += v1; counts[1] += !v1 && e1; counts[2] += !e1;
            const Vector4f c = M_d * Vector4f((float)pos.x * 8 * S.voxelSize, (float)pos.y * 8 * S.voxelSize, (float)pos.z * 8 * S.voxelSize, 1.0f);
            counts[3] += c.z < 1e-10f;
        }
        Out o;
        put(o, "crc", T_U32, S.crc); put(o, "counts", T_I32, counts);   // visible, enlarged only, invisible, first corner behind the camera
        put(o, "flags", T_U8, flags);                                    // per block: visible<false>, enlarged<false>, visible<true>, enlarged<true>
        write_pin(prefix + "visibility.bin", o);
    }

#else
    printf("ref_pin_stages: built without SceneReconstructionEngine.hpp -- cases skipped: integrate, alloc_pp, visibility\n");
#endif

    // ---- (f) expected_depths: CreateExpectedDepths (VisualisationEngine_CUDA.cu:119-173) with
    //      projectAndSplitBlocks_device and fillBlocks_device (VisualisationHelper.cu:52-77, 105-121);
    //      the prefix sum hands out offsets in entry order here
    {
        const Matrix4f pose = load_rt(get<float>(in, "w2c_d", 12));
        const int32_t* visibleEntryIDs = get<int32_t>(in, "ed_vis");
        const int noVisibleEntries = (int)count_of(in, "ed_vis");
        Vector2f init; init.x = FAR_AWAY; init.y = VERY_CLOSE;                       // VisualisationEngine_CUDA.cu:130-133
        std::vector<Vector2f> minmaxData((size_t)W * H, init);
        std::vector<RenderingBlock> list;
        unsigned noTotalBlocks = 0;
        std::vector<int32_t> counts(9, 0);
        std::vector<uint8_t> entry_valid; std::vector<int16_t> entry_box; std::vector<float> entry_z;
        for (int in_offset = 0; in_offset < noVisibleEntries; ++in_offset) {
            const HashEntry& blockData = S.hash[visibleEntryIDs[in_offset]];
            Vector2i upperLeft, lowerRight; Vector2f zRange;
            bool validProjection = false;
            if (blockData.ptr >= 0)                                                 // VisualisationHelper.cu:63-64
                validProjection = ProjectSingleBlock(blockData.pos, pose, S.proj, S.imgSize, S.voxelSize, upperLeft, lowerRight, zRange);
            entry_valid.push_back(validProjection);
            entry_box.push_back(validProjection ? upperLeft.x : 0); entry_box.push_back(validProjection ? upperLeft.y : 0);
            entry_box.push_back(validProjection ? lowerRight.x : 0); entry_box.push_back(validProjection ? lowerRight.y : 0);
            entry_z.push_back(validProjection ? zRange.x : 0); entry_z.push_back(validProjection ? zRange.y : 0);
            counts[0] += blockData.ptr < 0; counts[1] += blockData.ptr >= 0 && !validProjection; counts[2] += validProjection;
            if (blockData.ptr >= 0) {
                int behind = 0;
                for (int corner = 0; corner < 8; ++corner) {
                    const Vector4f c = pose * Vector4f((float)(blockData.pos.x + (corner & 1)) * 8 * S.voxelSize, (float)(blockData.pos.y + ((corner >> 1) & 1)) * 8 * S.voxelSize,
                                                       (float)(blockData.pos.z + (corner >> 2)) * 8 * S.voxelSize, 1.0f);
                    behind += c.z < 1e-6;
                }
                counts[3] += validProjection && behind > 0 && behind < 8;
            }
            if (!validProjection) continue;                                         // :70, :73 (no blocks required)
            const Vector2i requiredRenderingBlocks((int)ceilf((float)(lowerRight.x - upperLeft.x + 1) / renderingBlockSizeX),
                                                   (int)ceilf((float)(lowerRight.y - upperLeft.y + 1) / renderingBlockSizeY));   // :66-67
            const size_t requiredNumBlocks = (size_t)requiredRenderingBlocks.x * requiredRenderingBlocks.y;
            const unsigned out_offset = noTotalBlocks;
            noTotalBlocks += (unsigned)requiredNumBlocks;
            if (out_offset + requiredNumBlocks > (size_t)MAX_RENDERING_BLOCKS) continue;   // :74
            list.resize(out_offset + requiredNumBlocks);
            CreateRenderingBlocks(list.data(), (int)out_offset, upperLeft, lowerRight, zRange);
            counts[4] += upperLeft.x == 0; counts[5] += upperLeft.y == 0;
            counts[6] += lowerRight.x == W - 1; counts[7] += lowerRight.y == H - 1;
            counts[8] += requiredNumBlocks > 1;
        }
        if (noTotalBlocks > (unsigned)MAX_RENDERING_BLOCKS) noTotalBlocks = MAX_RENDERING_BLOCKS;   // VisualisationEngine_CUDA.cu:163
        for (unsigned block = 0; block < noTotalBlocks; ++block) {
            const RenderingBlock& b(list[block]);
            for (int y = 0; y < renderingBlockSizeY; ++y) for (int x = 0; x < renderingBlockSizeX; ++x) {
                const int xpos = b.upperLeft.x + x; if (xpos > b.lowerRight.x) continue;           // VisualisationHelper.cu:114-117
                const int ypos = b.upperLeft.y + y; if (ypos > b.lowerRight.y) continue;
                Vector2f& pixel(minmaxData[xpos + ypos * W]);
                pixel.x = ::fminf(b.zRange.x, pixel.x); pixel.y = ::fmaxf(b.zRange.y, pixel.y);   // atomicMin / atomicMax, CUDAUtils.hpp:75-95
            }
        }
        std::vector<int16_t> corners; std::vector<float> z, range((size_t)W * H * 2);
        for (unsigned i = 0; i < noTotalBlocks; ++i) {
            corners.push_back(list[i].upperLeft.x); corners.push_back(list[i].upperLeft.y);
            corners.push_back(list[i].lowerRight.x); corners.push_back(list[i].lowerRight.y);
            z.push_back(list[i].zRange.x); z.push_back(list[i].zRange.y);
        }
        memcpy(range.data(), minmaxData.data(), range.size() * 4);
        Out o;
        // counts: list entries with ptr < 0, rejected, accepted projections, accepted with some corners behind the
        // camera, boxes touching the left, top, right, bottom image side, boxes of more than one rendering block
        put(o, "crc", T_U32, S.crc); put(o, "counts", T_I32, counts);
        put(o, "entry_valid", T_U8, entry_valid); put(o, "entry_box", T_I16, entry_box); put(o, "entry_z", T_F32, entry_z);
        put(o, "block_corners", T_I16, corners); put(o, "block_z", T_F32, z); put(o, "range", T_F32, range);
        write_pin(prefix + "expected_depths.bin", o);
    }

    // ---- (g) pixels, from the raycast of camera a: renderICP_device<false> (VisualisationHelper.hpp:64-73,
    //      launched at VisualisationEngine_CUDA.cu:356), renderGrey_device, renderGrey_ImageNormals_device<false>,
    //      renderColourFromNormal_device, renderColourFromConfidence_device, renderColour_device
    //      (VisualisationHelper.hpp:75-148, 200-213; launched at VisualisationEngine_CUDA.cu:254-290)
    {
        const Matrix4f invM = load_rt(get<float>(in, "c2w_a", 12));
        const Vector3f lightSource = -Vector3f(invM.getColumn(2));               // VisualisationEngine_CUDA.cu:243, :341
        const Vector4f* pointsRay = rays_a.data();
        std::vector<Vector4f> pointsMap((size_t)W * H), normalsMap((size_t)W * H);
        std::vector<Vector4u> grey((size_t)W * H, Vector4u((uchar)0)), grey_in(grey), normal(grey), confidence(grey), colour(grey);
        std::vector<uint32_t> icp_idx; std::vector<float> icp;
        std::vector<int32_t> counts(8, 0);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int locId = x + y * W;
                processPixelICP<false, false>(pointsMap.data(), normalsMap.data(), pointsRay, S.imgSize, x, y, S.voxelSize, lightSource);
                const Vector4f ptRay = pointsRay[locId];
                processPixelGrey<Voxel_s, VoxelBlockHash>(grey[locId], ptRay.toVector3(), ptRay.w > 0, vox, S.hash, lightSource);
                processPixelGrey_ImageNormals<true, false>(grey_in.data(), pointsRay, S.imgSize, x, y, S.voxelSize, lightSource);
                processPixelNormal<Voxel_s, VoxelBlockHash>(normal[locId], ptRay.toVector3(), ptRay.w > 0, vox, S.hash, lightSource);
                processPixelConfidence<Voxel_s, VoxelBlockHash>(confidence[locId], ptRay, ptRay.w > 0, vox, S.hash, lightSource);
                processPixelColour<Voxel_s_rgb, VoxelBlockHash>(colour[locId], ptRay.toVector3(), ptRay.w > 0, vox_rgb, S.hash);
                // the host build writes 0 where the device build writes a quiet NaN
                // (VisualisationEngine_Shared.hpp:387-391): found pixels are stored, the others are not
                if (normalsMap[locId].w == 1.0f) {
                    if (pointsMap[locId].w != 1.0f) die("processPixelICP w");
                    icp_idx.push_back((uint32_t)locId);
                    icp.push_back(pointsMap[locId].x); icp.push_back(pointsMap[locId].y); icp.push_back(pointsMap[locId].z);
                    icp.push_back(normalsMap[locId].x); icp.push_back(normalsMap[locId].y); icp.push_back(normalsMap[locId].z);
                } else if (bits(normalsMap[locId].w) != 0 || bits(pointsMap[locId].w) != 0) die("processPixelICP not-found value");
                counts[0] += normalsMap[locId].w == 1.0f;
                // doPlus1 of computeNormalAndAngle<true, false> (VisualisationEngine_Shared.hpp:216-241), formed again
                if (ptRay.w > 0.0f && !(y <= 2 || y >= H - 3 || x <= 2 || x >= W - 3)) {
                    const Vector4f xp = pointsRay[(x + 2) + y * W], yp = pointsRay[x + (y + 2) * W], xm = pointsRay[(x - 2) + y * W], ym = pointsRay[x + (y - 2) * W];
                    bool doPlus1 = xp.w <= 0 || yp.w <= 0 || xm.w <= 0 || ym.w <= 0;
                    if (!doPlus1) {
                        const Vector4f dx = xp - xm, dy = yp - ym;
                        const float length_diff = MAX(dx.x * dx.x + dx.y * dx.y + dx.z * dx.z, dy.x * dy.x + dy.y * dy.y + dy.z * dy.z);
                        doPlus1 = length_diff * S.voxelSize * S.voxelSize > (0.15f * 0.15f);
                    }
                    counts[doPlus1 ? 6 : 7]++;
                }
                counts[1] += grey[locId].w != 0; counts[2] += grey_in[locId].w != 0; counts[3] += normal[locId].x != 0;
                counts[4] += confidence[locId].w != 0; counts[5] += colour[locId].w != 0;
            }
        Out o;
        put(o, "crc", T_U32, S.crc); put(o, "counts", T_I32, counts);   // lit pixels: ICP, grey, grey from image normals, normal, confidence, colour; doPlus1 taken, not taken
        put(o, "icp_idx", T_U32, icp_idx); put(o, "icp", T_F32, icp);
        const std::vector<Vector4u>* imgs[5] = { &grey, &grey_in, &normal, &confidence, &colour };
        const char* names[5] = { "grey", "grey_imagenormals", "normal", "confidence", "colour" };
        for (int k = 0; k < 5; ++k) {
            std::vector<uint8_t> raw((size_t)W * H * 4);
            memcpy(raw.data(), imgs[k]->data(), raw.size());
            put(o, names[k], T_U8, raw);
        }
        write_pin(prefix + "pixels.bin", o);
    }
    printf("ref_pin_stages: wrote %s*.bin\n", prefix.c_str());
    return 0;
}
