// view_host_main.cpp -- drives the host-only code of the free views on the CPU: the registry of a context's live
// views (TfCtxViews, topfusion_amd/csrc/tf_ctx_mem.h) and the PPM writer (tfusion::io::writePPM,
// include/tfusion/io.hpp).  tests/test_view_host.py builds it with -fsanitize=address,undefined and runs it.
//
// The views are heap objects of the C library, so one dropped twice, or used after its drop, is a sanitizer report.
//
//   ./view_host_main <directory to write in>
//
// Prints "ok <views dropped> views, <ppm bytes> ppm bytes" and returns 0.
#include "../topfusion_amd/csrc/tf_ctx_mem.h"
#include "../include/tfusion/io.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

static long g_failures, g_dropped;
static std::vector<int> g_drop_order;

#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) { ++g_failures; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
    } while (0)

struct FakeView { int id; char pad[28]; };

static FakeView* make_view(int id)
{
    FakeView* v = (FakeView*)malloc(sizeof(FakeView));
    if (!v) abort();
    v->id = id;
    return v;
}
static void drop_view(void* p)
{
    g_drop_order.push_back(((FakeView*)p)->id);
    ++g_dropped;
    free(p);
}

static void views()
{
    FakeView* v[5];
    {
        TfCtxViews reg;
        EXPECT(reg.count() == 0 && !reg.live(nullptr) && !reg.remove(nullptr));
        for (int i = 0; i < 5; ++i) {
            v[i] = make_view(i);
            EXPECT(reg.add(v[i], drop_view, 9) == 0);
        }
        EXPECT(reg.count() == 5 && reg.live(v[0]) && reg.live(v[4]));
        // tf_view_destroy: the caller releases the view itself after a successful remove
        EXPECT(reg.remove(v[2]));
        drop_view(v[2]);
        EXPECT(!reg.live(v[2]) && !reg.remove(v[2]) && reg.count() == 4);      // a second destroy finds nothing
        EXPECT(reg.remove(v[0]));
        drop_view(v[0]);
        int other = 0;
        EXPECT(!reg.remove(&other) && !reg.live(&other) && reg.count() == 3);  // not a view of this context
        EXPECT(g_dropped == 2);
    }   // tf_destroy: the three still alive, newest first
    EXPECT(g_dropped == 5);
    const std::vector<int> want = { 2, 0, 4, 3, 1 };
    EXPECT(g_drop_order == want);
    {
        TfCtxViews empty;                      // nothing to drop
    }
    EXPECT(g_dropped == 5);
}

static long ppm(const std::string& dir)
{
    const int cols = 5, rows = 3;
    const size_t step = cols * 4 + 12;         // pitched: 12 bytes of padding per row, never read as pixels
    std::vector<uint8_t> img(step * rows, 0xee);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x)
            for (int c = 0; c < 4; ++c) img[y * step + 4 * x + c] = (uint8_t)(40 * y + 7 * x + c);
    const std::string path = dir + "/view_host.ppm";
    tfusion::io::writePPM(path, img.data(), cols, rows, step);
    FILE* f = fopen(path.c_str(), "rb");
    EXPECT(f != nullptr);
    if (!f) return 0;
    std::vector<unsigned char> got(4096);
    const size_t n = fread(got.data(), 1, got.size(), f);
    fclose(f);
    const char* head = "P6\n5 3\n255\n";
    const size_t hl = strlen(head);
    EXPECT(n == hl + (size_t)cols * rows * 3);
    EXPECT(n >= hl && memcmp(got.data(), head, hl) == 0);
    for (int y = 0; y < rows && n == hl + (size_t)cols * rows * 3; ++y)
        for (int x = 0; x < cols; ++x)
            for (int c = 0; c < 3; ++c) EXPECT(got[hl + (y * cols + x) * 3 + c] == (unsigned char)(40 * y + 7 * x + c));
    // the packed form (step 0) gives the same file; it round-trips through the library's own reader (B, G, R)
    std::vector<uint8_t> packed((size_t)cols * rows * 4);
    for (int y = 0; y < rows; ++y) memcpy(&packed[(size_t)y * cols * 4], &img[y * step], (size_t)cols * 4);
    const std::string path2 = dir + "/view_host_packed.ppm";
    tfusion::io::writePPM(path2, packed.data(), cols, rows);
    std::vector<uint8_t> bgr;
    int rc = 0, rr = 0;
    tfusion::io::readPPM(path2, bgr, rc, rr);
    EXPECT(rc == cols && rr == rows && bgr.size() == (size_t)cols * rows * 3);
    for (size_t i = 0; i + 2 < bgr.size() && bgr.size() == (size_t)cols * rows * 3; i += 3)
        EXPECT(bgr[i] == got[hl + i + 2] && bgr[i + 1] == got[hl + i + 1] && bgr[i + 2] == got[hl + i]);
    // refusals: no image, no size, a step shorter than a row, a directory that is not there
    int thrown = 0;
    try { tfusion::io::writePPM(path, nullptr, cols, rows); } catch (const std::runtime_error&) { ++thrown; }
    try { tfusion::io::writePPM(path, img.data(), 0, rows); } catch (const std::runtime_error&) { ++thrown; }
    try { tfusion::io::writePPM(path, img.data(), cols, rows, cols * 4 - 1); } catch (const std::runtime_error&) { ++thrown; }
    try { tfusion::io::writePPM(dir + "/no/such/dir/x.ppm", img.data(), cols, rows, step); } catch (const std::runtime_error&) { ++thrown; }
    EXPECT(thrown == 4);
    return (long)n;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    views();
    const long n = ppm(argv[1]);
    if (g_failures) return 1;
    printf("ok %ld views, %ld ppm bytes\n", g_dropped, n);
    return 0;
}
