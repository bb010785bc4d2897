// scene_merge_records_main.cpp -- drives the map merge's host pass over a record table
// (tf_merge_records_check, topfusion_amd/csrc/tf_scene_file.cpp); tests/test_scene_merge_ref.py builds it for the
// CPU with -fsanitize=address,undefined.  The records section of a validated file is handed over in a heap buffer
// of exactly its length, so a read past the end is a sanitizer report.
//
//   scene_merge_records_main FILE n_carried
//
// Prints "ok <checks>" and returns 0 when the file's own table passes with n_carried carried records, with no
// offset, a null one and the largest ones that keep every carried position inside int16; one step further is
// refused on each axis and side; so are extreme offsets; so is the table with one carried record's position
// copied onto another's, for the first, a middle and the last pair -- while the same copy onto a record without a
// block passes.  An empty table passes.
#include "../topfusion_amd/csrc/tf_scene_file.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static long g_checks = 0, g_failures = 0;

static void expect(const std::vector<unsigned char>& rec, const int* off, tf_status want, long long want_carried, const char* what)
{
    const size_t len = rec.size();
    unsigned char* exact = (unsigned char*)malloc(len ? len : 1);
    if (!exact) abort();
    if (len) memcpy(exact, rec.data(), len);
    long long carried = -1;
    const tf_status s = tf_merge_records_check(exact, (long long)(len / TF_SCENE_RECORD_BYTES), off, &carried);
    free(exact);
    ++g_checks;
    if (s != want || (want == TF_OK && carried != want_carried)) {
        ++g_failures;
        fprintf(stderr, "%s: status %d (want %d), carried %lld (want %lld)\n", what, (int)s, (int)want, carried, want_carried);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> data;
    unsigned char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + n);
    fclose(f);
    const long long want_carried = atoll(argv[2]);
    struct tf_map_file_info info;
    TfSceneLayout lay;
    if (tf_map_file_validate(data.data(), data.size(), &info, &lay) != TF_OK) return 3;
    const size_t n = (size_t)info.scene.n_records;
    const std::vector<unsigned char> rec(data.begin() + (ptrdiff_t)lay.records_off,
                                         data.begin() + (ptrdiff_t)(lay.records_off + n * TF_SCENE_RECORD_BYTES));
    // the carried records and the range of their positions
    std::vector<size_t> carried, plain;
    int lo[3] = { INT_MAX, INT_MAX, INT_MAX }, hi[3] = { INT_MIN, INT_MIN, INT_MIN };
    for (size_t k = 0; k < n; ++k) {
        int32_t ptr;
        int16_t xyz[3];
        memcpy(&ptr, rec.data() + k * TF_SCENE_RECORD_BYTES + 16, 4);
        memcpy(xyz, rec.data() + k * TF_SCENE_RECORD_BYTES + 4, 6);
        if (ptr < 0) { plain.push_back(k); continue; }
        carried.push_back(k);
        for (int a = 0; a < 3; ++a) {
            if (xyz[a] < lo[a]) lo[a] = xyz[a];
            if (xyz[a] > hi[a]) hi[a] = xyz[a];
        }
    }
    if ((long long)carried.size() != want_carried || carried.size() < 3 || plain.empty()) return 4;
    const int zero[3] = { 0, 0, 0 };
    expect(rec, nullptr, TF_OK, want_carried, "no offset");
    expect(rec, zero, TF_OK, want_carried, "zero offset");
    expect(std::vector<unsigned char>(), nullptr, TF_OK, 0, "empty table");
    for (int a = 0; a < 3; ++a) {
        int off[3] = { 0, 0, 0 };
        off[a] = SHRT_MAX - hi[a];
        expect(rec, off, TF_OK, want_carried, "largest offset");
        off[a] += 1;
        expect(rec, off, TF_INVALID_ARG, 0, "one above the largest offset");
        off[a] = SHRT_MIN - lo[a];
        expect(rec, off, TF_OK, want_carried, "smallest offset");
        off[a] -= 1;
        expect(rec, off, TF_INVALID_ARG, 0, "one below the smallest offset");
        off[a] = INT_MAX;
        expect(rec, off, TF_INVALID_ARG, 0, "INT_MAX");
        off[a] = INT_MIN;
        expect(rec, off, TF_INVALID_ARG, 0, "INT_MIN");
        off[a] = 65536;                                    // (a wrap of 16 bits is not an identity)
        expect(rec, off, TF_INVALID_ARG, 0, "65536");
    }
    const size_t pairs[3][2] = { { carried[0], carried[1] }, { carried[carried.size() / 2], carried[0] },
                                 { carried.back(), carried[carried.size() / 2] } };
    for (const auto& p : pairs) {
        std::vector<unsigned char> dup = rec;
        memcpy(dup.data() + p[0] * TF_SCENE_RECORD_BYTES + 4, rec.data() + p[1] * TF_SCENE_RECORD_BYTES + 4, 6);
        expect(dup, nullptr, TF_INVALID_ARG, 0, "a duplicated position");
        const int off[3] = { 1, -1, 2 };
        expect(dup, off, TF_INVALID_ARG, 0, "a duplicated position, moved");
    }
    {   // a record without a block is not carried: its position may be anyone's
        std::vector<unsigned char> dup = rec;
        memcpy(dup.data() + plain[0] * TF_SCENE_RECORD_BYTES + 4, rec.data() + carried[0] * TF_SCENE_RECORD_BYTES + 4, 6);
        expect(dup, nullptr, TF_OK, want_carried, "a position shared with a record without a block");
    }
    if (g_failures) return 1;
    printf("ok %ld checks\n", g_checks);
    return 0;
}
