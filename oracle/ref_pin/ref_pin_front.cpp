// ref_pin_front.cpp -- TEST INFRASTRUCTURE.  Runs the reference's OWN front-end kernels (imgproc.cu) and
// the per-pixel half of its projective ICP (proj_icp.cu: ComputeIcpHelper::find_coresp, proj, reproj and the
// operators of device.hpp beneath them) on the host, and writes the golden files
// tests/golden/front_pin_<case>_p<k>.bin that pin the oracle's stateless stage functions and, through
// tests/test_gpu_front_pin.py, the HIP kernels.
//
// Built by oracle/Makefile (target ref) into oracle/_ref/: the two .cu files are included from the
// reference tree through the recipe, which rewrites each `kernel<<<g, b>>>(args);` statement into
// `cuda_exec::launch(g, b, [&]{ kernel(args); });` on the way to the compiler (the rewritten text exists
// under oracle/_ref/ only); device_memory.cpp is compiled beside it.  CUDA is replaced by the EXECUTING
// stand-ins of oracle/ref_pin/cuda_exec, which hold DESIGN.md section 3 as code: every other computed bit
// comes from the reference's own text.
//
//   ref_pin_front <input pin file> <output directory> <case name>
//
// Of the host side only the lines that form the kernels' arguments are restated here, each with its
// lines.  Every buffer handed to a kernel is pitched, padded to whole 32 x 8 CTAs in both directions and
// prefilled, because compute_dists_kernel guards with `x < cols || y < rows` (imgproc.cu:268) and so
// touches every pixel of its grid; only the image region is stored.  Input, file format and array
// names: tests/front_pin_cases.py.
#include "cuda_runtime.h"      // first: kernel_containers.hpp makes __tf_device__ functions inline only under __CUDACC__
#include "imgproc.inc"
#include "proj_icp.inc"
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;

using namespace tfusion::device;

static_assert(sizeof(float4) == 16 && sizeof(float3) == 12 && sizeof(float2) == 8, "vector type layout");
static_assert(sizeof(Mat3f) == 36 && sizeof(Aff3f) == 48, "Aff3f layout");
static_assert(sizeof(Reprojector) == 16, "Reprojector layout");
static_assert(sizeof(PtrStep<float4>) == 2 * sizeof(void*) && sizeof(PtrStepSz<ushort>) == 3 * sizeof(void*), "PtrStep layout");
static_assert(sizeof(ComputeIcpHelper) == 2 * 4 + 48 + 2 * 4 + 3 * 8 + 3 * sizeof(PtrStep<float4>), "ComputeIcpHelper layout");
static_assert(std::is_same<decltype(ComputeIcpHelper::cols), float>::value, "find_coresp's image test compares with float cols / rows");
static_assert(std::is_same<decltype(std::cos(1.0f)), float>::value, "cos(float) must be the float overload");
static_assert(ComputeIcpHelper::Policy::CTA_SIZE_X == 32 && ComputeIcpHelper::Policy::CTA_SIZE_Y == 8 && ComputeIcpHelper::Policy::TOTAL == 27, "ICP policy");

static void die(const char* what) { fprintf(stderr, "ref_pin_front: %s\n", what); exit(1); }

// ---- pin files (tests/pin_scenes.py); 16-bit depths travel as type 1 (i16), bits unchanged ------------
enum { T_U8, T_I16, T_I32, T_U32, T_F32 };
static const size_t k_size[5] = { 1, 2, 4, 4, 4 };
struct Arr { int code; size_t count; std::vector<char> data; };
typedef std::vector<std::pair<std::string, Arr> > Out;

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
        if (a.data.size() && fread(&a.data[0], 1, a.data.size(), f) != a.data.size()) die("short array");
        m[name] = a;
    }
    fclose(f);
    return m;
}

static size_t bytes_of(const Arr& a) { return 32 + a.data.size(); }

// the arrays in order, over as many files <prefix>_p<k>.bin as keep each within max_bytes; `head`
// (the CRC32 of the input) opens every file
static void write_array(FILE* f, const std::string& nm, const Arr& a)
{
    char name[24] = { 0 };
    if (nm.size() > 23) die("array name too long");
    memcpy(name, nm.c_str(), nm.size());
    uint32_t hdr[2] = { (uint32_t)a.code, (uint32_t)a.count };
    fwrite(name, 1, 24, f); fwrite(hdr, 4, 2, f);
    if (a.data.size()) fwrite(&a.data[0], 1, a.data.size(), f);
}

static void write_parts(const std::string& prefix, const Arr& head, const Out& out, size_t max_bytes)
{
    size_t i = 0; int part = 0;
    while (i < out.size()) {
        size_t j = i, total = 12 + bytes_of(head);
        while (j < out.size() && total + bytes_of(out[j].second) <= max_bytes) total += bytes_of(out[j++].second);
        if (j == i) { fprintf(stderr, "%s\n", out[i].first.c_str()); die("one array exceeds the size limit of a golden"); }
        char tail[32]; snprintf(tail, sizeof tail, "_p%d.bin", part++);
        FILE* f = fopen((prefix + tail).c_str(), "wb");
        if (!f) die("cannot open an output file");
        const uint32_t n = (uint32_t)(j - i + 1);
        fwrite("TFPIN1\0\0", 1, 8, f); fwrite(&n, 4, 1, f);
        write_array(f, "crc", head);
        for (size_t k = i; k < j; ++k) write_array(f, out[k].first, out[k].second);
        fclose(f);
        i = j;
    }
}

template<class T> static const T* get(const std::map<std::string, Arr>& m, const std::string& name, size_t count)
{
    std::map<std::string, Arr>::const_iterator it = m.find(name);
    if (it == m.end() || sizeof(T) != k_size[it->second.code] || it->second.count != count) {
        fprintf(stderr, "input array %s\n", name.c_str()); die("missing or wrong input array");
    }
    return (const T*)&it->second.data[0];
}

// ---- buffers: pitched, padded to whole CTAs, prefilled; only the image region is stored ---------------
template<class T> struct Img {
    int rows, cols; size_t step; std::vector<char> mem;
    Img() : rows(0), cols(0), step(0) {}
    Img(int r, int c) { create(r, c); }
    void create(int r, int c)
    {
        rows = r; cols = c;
        const int pc = (c + 31) / 32 * 32 + 32, pr = (r + 7) / 8 * 8 + 8;
        step = (size_t)pc * sizeof(T) + 64;
        mem.assign(step * pr, (char)0xA5);
    }
    T* data() { return (T*)&mem[0]; }
    PtrStepSz<T> sz() { return PtrStepSz<T>(rows, cols, data(), step); }
    PtrStep<T> st() { return PtrStep<T>(data(), step); }
    T& at(int y, int x) { return *(T*)(&mem[0] + (size_t)y * step + (size_t)x * sizeof(T)); }
    void load(const T* src) { for (int y = 0; y < rows; ++y) memcpy(&at(y, 0), src + (size_t)y * cols, (size_t)cols * sizeof(T)); }
    void put(Out& o, const std::string& name, int code)
    {
        Arr a; a.code = code; a.count = (size_t)rows * cols * sizeof(T) / k_size[code];
        a.data.assign(((size_t)rows * cols * sizeof(T) + 3) & ~(size_t)3, 0);
        for (int y = 0; y < rows; ++y) if (cols) memcpy(&a.data[(size_t)y * cols * sizeof(T)], &at(y, 0), (size_t)cols * sizeof(T));
        if (a.count) o.push_back(std::make_pair(name, a));          // (an empty level is left out)
    }
};

template<class T> static void put_vec(Out& o, const std::string& name, int code, const std::vector<T>& v)
{
    Arr a; a.code = code; a.count = v.size();
    a.data.assign((v.size() * sizeof(T) + 3) & ~(size_t)3, 0);
    if (v.size()) memcpy(&a.data[0], &v[0], v.size() * sizeof(T));
    o.push_back(std::make_pair(name, a));
}

// the launch geometry every front-end wrapper forms (imgproc.cu:55-56, 84-85, 135-136, 249-250, 285-286, 396-397)
static const dim3 k_block(32, 8);
static dim3 grid_of(int cols, int rows) { return dim3(divUp(cols, k_block.x), divUp(rows, k_block.y)); }

// ---- the wrappers' argument lines, restated ------------------------------------------------------------
static void run_bilateral(Img<ushort>& src, Img<ushort>& dst, int kernel_size, float sigma_spatial, float sigma_depth)
{
    sigma_depth *= 1000;                                                                  // imgproc.cu:53
    PtrStepSz<ushort> s = src.sz(); PtrStep<ushort> d = dst.st();
    cuda_exec::launch(grid_of(src.cols, src.rows), k_block, [&]{                          // :59
        bilateral_kernel(s, d, kernel_size, 0.5f / (sigma_spatial * sigma_spatial), 0.5f / (sigma_depth * sigma_depth)); });
}

static void run_truncate(Img<ushort>& depth, float max_dist)
{
    PtrStepSz<ushort> d = depth.sz();
    cuda_exec::launch(grid_of(depth.cols, depth.rows), k_block, [&]{ truncate_depth_kernel(d, static_cast<ushort>(max_dist * 1000.f)); });   // :87
}

static void run_pyramid(Img<ushort>& source, Img<ushort>& pyramid, float sigma_depth)
{
    sigma_depth *= 1000;                                                                  // :133
    PtrStepSz<ushort> s = source.sz(), d = pyramid.sz();
    cuda_exec::launch(grid_of(pyramid.cols, pyramid.rows), k_block, [&]{ pyramid_kernel(s, d, sigma_depth * 3); });                          // :138
}

static void run_points_normals(const float intr[4], int level, Img<ushort>& depth, Img<float4>& points, Img<float4>& normals)
{
    const int div = 1 << level;                                                           // Intr::operator(), precomp.cpp:10-14
    Reprojector reproj;                                                                   // Reprojector::Reprojector, precomp.cpp:55
    reproj.finv = make_float2(1.f / (intr[0] / div), 1.f / (intr[1] / div));
    reproj.c = make_float2(intr[2] / div, intr[3] / div);
    PtrStepSz<ushort> d = depth.sz(); PtrStep<Point> p = points.st(); PtrStep<Normal> n = normals.st();
    cuda_exec::launch(grid_of(depth.cols, depth.rows), k_block, [&]{ points_normals_kernel(reproj, d, p, n); });                             // :252
}

static void run_resize(Img<float4>& points, Img<float4>& normals, Img<float4>& points_out, Img<float4>& normals_out)
{
    PtrStep<Point> v = points.st(); PtrStep<Normal> n = normals.st();
    PtrStepSz<Point> vo = points_out.sz(); PtrStep<Normal> no = normals_out.st();
    cuda_exec::launch(grid_of(points_out.cols, points_out.rows), k_block, [&]{ resize_points_normals_kernel(v, n, vo, no); });               // :393-399
}

// bilateral (7, 4.5, 0.04), truncation at 2 m, two pyramid steps, points and normals of every level: what
// TopFu::operator() runs on a frame (topfu.cpp:166-197) with the default parameters (topfu.cpp:30-35)
struct Pyramid { Img<ushort> depth[3]; Img<float4> points[3], normals[3]; };
static void build_pyramid(const ushort* raw, int W, int H, const float intr[4], Pyramid& P)
{
    Img<ushort> src(H, W);
    src.load(raw);
    P.depth[0].create(H, W);
    run_bilateral(src, P.depth[0], 7, 4.5f, 0.04f);
    run_truncate(P.depth[0], 2.0f);
    for (int l = 1; l < 3; ++l) {
        P.depth[l].create(P.depth[l - 1].rows / 2, P.depth[l - 1].cols / 2);              // depthBuildPyramid, imgproc.cpp:14: (rows / 2) x (cols / 2)
        run_pyramid(P.depth[l - 1], P.depth[l], 0.04f);
    }
    for (int l = 0; l < 3; ++l) {
        P.points[l].create(P.depth[l].rows, P.depth[l].cols); P.normals[l].create(P.depth[l].rows, P.depth[l].cols);
        run_points_normals(intr, l, P.depth[l], P.points[l], P.normals[l]);
    }
}

// ---- front end -------------------------------------------------------------------------------------------
static void front(const std::map<std::string, Arr>& in, int W, int H, bool u16_only, Out& o)
{
    const float* intr = get<float>(in, "fparams", 4);
    const ushort* raw = get<ushort>(in, "depth", (size_t)W * H);
    Img<ushort> src(H, W);
    src.load(raw);
    {   // compute_dists (imgproc.cu:283-290): finv = (1 / f.x, 1 / f.y)
        Img<float> dists(H, W);
        PtrStepSz<ushort> d = src.sz(); Dists out = dists.sz();
        const float2 f = make_float2(intr[0], intr[1]), c = make_float2(intr[2], intr[3]);
        cuda_exec::launch(grid_of(W, H), k_block, [&]{ compute_dists_kernel(d, out, make_float2(1.f / f.x, 1.f / f.y), c); });
        dists.put(o, "dists", T_F32);
    }
    const int ksz[4] = { 1, 4, 7, 9 };
    Img<ushort> bil7;
    for (int k = 0; k < 4; ++k) {
        Img<ushort> dst(H, W);
        run_bilateral(src, dst, ksz[k], 4.5f, 0.04f);
        char name[16]; snprintf(name, sizeof name, "bil_k%d", ksz[k]);
        dst.put(o, name, T_I16);
        if (ksz[k] == 7) bil7 = dst;
    }
    {
        Img<ushort> dst(H, W);
        run_bilateral(src, dst, 5, 1.5f, 0.01f);
        dst.put(o, "bil_k5_s1.5_0.01", T_I16);
    }
    // truncation of the 7-tap image at 2.0 m, 1.2 m and 0 (the ushort formed from 0 is 0: every depth goes)
    Img<ushort> d0;
    const float max_dist[3] = { 2.0f, 1.2f, 0.0f };
    const char* tname[3] = { "trunc_2.0", "trunc_1.2", "trunc_0" };
    for (int k = 0; k < 3; ++k) {
        Img<ushort> t = bil7;
        run_truncate(t, max_dist[k]);
        t.put(o, tname[k], T_I16);
        if (k == 0) d0 = t;
    }
    Pyramid P;
    P.depth[0] = d0;
    for (int l = 1; l < 3; ++l) {
        P.depth[l].create(P.depth[l - 1].rows / 2, P.depth[l - 1].cols / 2);
        if (P.depth[l - 1].rows >= 2 && P.depth[l - 1].cols >= 2) run_pyramid(P.depth[l - 1], P.depth[l], 0.04f);
        P.depth[l].put(o, l == 1 ? "pyr1" : "pyr2", T_I16);
    }
    if (u16_only) return;
    for (int l = 0; l < 3; ++l) {
        P.points[l].create(P.depth[l].rows, P.depth[l].cols); P.normals[l].create(P.depth[l].rows, P.depth[l].cols);
        if (P.depth[l].rows && P.depth[l].cols) run_points_normals(intr, l, P.depth[l], P.points[l], P.normals[l]);
        const char c = (char)('0' + l);
        P.points[l].put(o, std::string("points") + c, T_F32); P.normals[l].put(o, std::string("normals") + c, T_F32);
    }
    Img<float4> rp[3], rn[3];
    rp[0] = P.points[0]; rn[0] = P.normals[0];
    for (int l = 1; l < 3; ++l) {
        rp[l].create(rp[l - 1].rows / 2, rp[l - 1].cols / 2); rn[l].create(rp[l - 1].rows / 2, rp[l - 1].cols / 2);
        if (rp[l].rows && rp[l].cols) run_resize(rp[l - 1], rn[l - 1], rp[l], rn[l]);
        const char c = (char)('0' + l);
        rp[l].put(o, std::string("resized_points") + c, T_F32); rn[l].put(o, std::string("resized_normals") + c, T_F32);
    }
}

// ---- ICP rows ----------------------------------------------------------------------------------------------
static void icp(const std::map<std::string, Arr>& in, int W, int H, Out& o)
{
    const float* intr = get<float>(in, "fparams", 4);
    Pyramid curr, prev;
    build_pyramid(get<ushort>(in, "depth1", (size_t)W * H), W, H, intr, curr);            // frame 1: the current maps
    build_pyramid(get<ushort>(in, "depth0", (size_t)W * H), W, H, intr, prev);            // frame 0: the previous maps
    for (int l = 0; l < 3; ++l) {
        const char c = (char)('0' + l);
        curr.points[l].put(o, std::string("vcurr") + c, T_F32); curr.normals[l].put(o, std::string("ncurr") + c, T_F32);
        prev.points[l].put(o, std::string("vprev") + c, T_F32); prev.normals[l].put(o, std::string("nprev") + c, T_F32);
    }
    const float* thr = get<float>(in, "thr", 4);                                          // (dist, angle) x 2
    for (int l = 0; l < 3; ++l) for (int t = 0; t < 2; ++t) for (int a = 0; a < 4; ++a) {
        char key[16]; snprintf(key, sizeof key, "L%dt%da%d", l, t, a);
        if (a == 3 && in.find(std::string("aff_") + key) == in.end()) continue;           // (the fourth affine is given for one case only)
        const float* aff = get<float>(in, std::string("aff_") + key, 12);                 // [R|t] row-major
        const int w = curr.points[l].cols, h = curr.points[l].rows;
        ComputeIcpHelper* hp = (ComputeIcpHelper*)calloc(1, sizeof(ComputeIcpHelper));    // (its constructor lies in projective_icp.cpp)
        ComputeIcpHelper& helper = *hp;
        helper.min_cosine = std::cos(thr[2 * t + 1]);                                     // projective_icp.cpp:13-14 (under its `using namespace std`: the float overload)
        helper.dist2_thres = thr[2 * t] * thr[2 * t];
        helper.rows = (float)h; helper.cols = (float)w;                                   // :181-182
        const int div = 1 << l;                                                           // setLevelIntr, :19-22
        helper.f = make_float2(intr[0] / div, intr[1] / div);
        helper.c = make_float2(intr[2] / div, intr[3] / div);
        helper.finv = make_float2(1.f / helper.f.x, 1.f / helper.f.y);
        helper.vcurr = curr.points[l].st(); helper.ncurr = curr.normals[l].st();          // :184-185
        for (int r = 0; r < 3; ++r) helper.aff.R.data[r] = make_float3(aff[4 * r], aff[4 * r + 1], aff[4 * r + 2]);   // device_cast<Aff3f>(affine), :189
        helper.aff.t = make_float3(aff[3], aff[7], aff[11]);
        // TextureBinder (texture_binder.hpp:28-32; proj_icp.cu:434-437): point filter, the level's own size and step
        vprev_tex.filterMode = cudaFilterModePoint; nprev_tex.filterMode = cudaFilterModePoint;
        cudaBindTexture2D(0, vprev_tex, prev.points[l].data(), cudaChannelFormatDesc(), w, h, prev.points[l].step);
        cudaBindTexture2D(0, nprev_tex, prev.normals[l].data(), cudaChannelFormatDesc(), w, h, prev.normals[l].step);
        std::vector<uint8_t> codes((size_t)w * h);
        std::vector<float> rows;
        std::vector<int32_t> counts(12, 0);
        for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
            float3 n, d, s;
            const int filtered = helper.find_coresp(x, y, n, d, s);                       // icp_helper_kernel, proj_icp.cu:364-365
            codes[(size_t)y * w + x] = (uint8_t)filtered;
            if (filtered % 40 || filtered > 200) die("find_coresp returned an unknown code");
            counts[filtered / 40]++;
            if (!filtered) {
                const float3 c = cross(s, n);                                             // the row, :372-374
                const float row[7] = { c.x, c.y, c.z, n.x, n.y, n.z, dot(n, d - s) };
                rows.insert(rows.end(), row, row + 7);
            }
            if (filtered == 80) {
                // counters only: which of the image test's comparisons (:90) hold, formed again with the reference's own operators
                const float3 p = helper.aff * tr(helper.vcurr(y, x));
                const float2 coo = helper.proj(p);
                counts[6] += p.z <= 0; counts[7] += coo.x < 0; counts[8] += coo.y < 0;
                counts[9] += coo.x >= helper.cols; counts[10] += coo.y >= helper.rows;
                counts[11] += coo.x == helper.cols || coo.y == helper.rows;
            }
        }
        free(hp);
        std::vector<float> a12(aff, aff + 12);
        put_vec(o, std::string("aff_") + key, T_F32, a12);
        put_vec(o, std::string("code_") + key, T_U8, codes);
        put_vec(o, std::string("rows_") + key, T_F32, rows);
        // counts: pixels per return code 0, 40, 80, 120, 160, 200; of the 80s: s.z <= 0, coo.x < 0, coo.y < 0, coo.x >= cols, coo.y >= rows,
        // coo.x == cols or coo.y == rows exactly
        put_vec(o, std::string("counts_") + key, T_I32, counts);
    }
    std::vector<float> t4(thr, thr + 4);
    put_vec(o, "thr", T_F32, t4);
}

int main(int argc, char** argv)
{
    if (argc != 4) die("usage: ref_pin_front <input> <output directory> <case>");
    const std::map<std::string, Arr> in = read_pin(argv[1]);
    const int32_t* ip = get<int32_t>(in, "iparams", 5);          // mode (0 front end, 1 ICP), cols, rows, u16 stages only, size limit of a file
    Arr head; head.code = T_U32; head.count = 1;
    head.data.assign((const char*)get<uint32_t>(in, "crc", 1), (const char*)get<uint32_t>(in, "crc", 1) + 4);
    Out o;
    if (ip[0] == 0) front(in, ip[1], ip[2], ip[3] != 0, o);
    else icp(in, ip[1], ip[2], o);
    const std::string prefix = std::string(argv[2]) + "/front_pin_" + argv[3];
    write_parts(prefix, head, o, (size_t)ip[4]);
    printf("ref_pin_front: wrote %s_p*.bin\n", prefix.c_str());
    return 0;
}
