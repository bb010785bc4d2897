// scene_map_parser_main.cpp -- drives the checkpoint file's host parser (topfusion_amd/csrc/tf_scene_file.cpp)
// over a valid version-2 file (the map checkpoint of a swapping context) and its damaged variants in one
// process; tests/test_scene_map_ref.py builds it for the CPU with -fsanitize=address,undefined.  Every variant
// is handed to the validator in a heap buffer of exactly its length, so a read past the end is a sanitizer
// report.
//
//   scene_map_parser_main FILE n_records n_blocks_stored n_cache_blocks frame_counter lastFreeBlockId
//                         lastFreeExcessListId noVisibleEntries pose_algebra n_blocks cols rows
//
// Prints "ok <variants> rejected" and returns 0 when the intact file is accepted with those info fields
// (version 2) and every variant is rejected, by tf_map_file_validate and -- as an unknown version -- by
// tf_scene_file_validate.
#include "../topfusion_amd/csrc/tf_scene_file.h"

#include <limits.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static long g_variants = 0, g_failures = 0;

static tf_status validate_copy(const std::vector<unsigned char>& v, size_t len, struct tf_map_file_info* info)
{
    unsigned char* exact = (unsigned char*)malloc(len ? len : 1);
    if (!exact) abort();
    if (len) memcpy(exact, v.data(), len);
    TfSceneLayout lay;
    const tf_status s = tf_map_file_validate(exact, len, info, &lay);
    struct tf_scene_file_info v1;
    if (tf_scene_file_validate(exact, len, &v1, &lay) != TF_INVALID_ARG) {      // version 1's reader takes none of them
        ++g_failures;
        fprintf(stderr, "tf_scene_file_validate accepted a version-2 variant of %zu bytes\n", len);
    }
    free(exact);
    return s;
}

static void expect_rejected(const std::vector<unsigned char>& v, size_t len, const char* what, long a, long b)
{
    struct tf_map_file_info info;
    ++g_variants;
    if (validate_copy(v, len, &info) != TF_INVALID_ARG) {
        ++g_failures;
        fprintf(stderr, "accepted: %s %ld %ld\n", what, a, b);
    }
}

static void fix_crcs(std::vector<unsigned char>& v, long long n_records)
{
    const uint32_t h = tf_scene_crc32(0u, v.data(), TF_MAP_OFF_CRC);
    const uint32_t r = tf_scene_crc32(0u, v.data() + TF_MAP_HEADER_BYTES, (size_t)n_records * TF_SCENE_RECORD_BYTES);
    memcpy(v.data() + TF_MAP_OFF_CRC, &h, 4);
    memcpy(v.data() + TF_MAP_OFF_RECORDS_CRC, &r, 4);
}

// the 32-bit word at `off` overwritten by 0, -1, INT_MAX and the value one below / above; `also_fixed`: again
// with both checksums recomputed, where the structure alone must refuse the value (`plus_one`: the value one
// above too)
static void word_variants(const std::vector<unsigned char>& file, size_t off, long long n_records, bool also_fixed, bool plus_one,
                          const char* what)
{
    int32_t orig;
    memcpy(&orig, file.data() + off, 4);
    const int32_t vals[5] = { 0, -1, INT_MAX, (int32_t)((uint32_t)orig - 1u), (int32_t)((uint32_t)orig + 1u) };
    for (int k = 0; k < 5; ++k) {
        if (vals[k] == orig) continue;
        std::vector<unsigned char> v = file;
        memcpy(v.data() + off, &vals[k], 4);
        expect_rejected(v, v.size(), what, (long)off, (long)vals[k]);
        if (also_fixed && (plus_one || k != 4)) {
            fix_crcs(v, n_records);
            expect_rejected(v, v.size(), "checksums recomputed", (long)off, (long)vals[k]);
        }
    }
}

// the byte at `off` overwritten by 0, 255, 127 (the byte's -1 and maximum) and the value one below / above;
// `fixed_from`: values >= it are also tried with the checksums recomputed (the structure must refuse them)
static void byte_variants(const std::vector<unsigned char>& file, size_t off, long long n_records, int fixed_from, const char* what)
{
    const int orig = file[off];
    const int vals[5] = { 0, 255, 127, (orig + 255) & 255, (orig + 1) & 255 };
    for (int k = 0; k < 5; ++k) {
        if (vals[k] == orig) continue;
        std::vector<unsigned char> v = file;
        v[off] = (unsigned char)vals[k];
        expect_rejected(v, v.size(), what, (long)off, (long)vals[k]);
        if (vals[k] >= fixed_from) {
            fix_crcs(v, n_records);
            expect_rejected(v, v.size(), "byte, checksums recomputed", (long)off, (long)vals[k]);
        }
    }
}

int main(int argc, char** argv)
{
    if (argc != 13) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "no file\n"); return 2; }
    std::vector<unsigned char> file;
    unsigned char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + got);
    fclose(f);

    // the intact file: accepted, the info fields as given; and through the path entry points
    struct tf_map_file_info info, info2;
    struct tf_scene_file_info v1;
    if (validate_copy(file, file.size(), &info) != TF_OK) { fprintf(stderr, "intact file rejected\n"); return 1; }
    if (tf_map_file_info(argv[1], &info2) != TF_OK || info2.version != info.version || info2.n_cache_blocks != info.n_cache_blocks ||
        memcmp(&info.scene, &info2.scene, sizeof(info.scene)) != 0) {
        fprintf(stderr, "tf_map_file_info differs\n");
        return 1;
    }
    if (tf_scene_file_info(argv[1], &v1) != TF_INVALID_ARG) { fprintf(stderr, "tf_scene_file_info took version 2\n"); return 1; }
    const long long want[12] = { 2, atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5]), atoll(argv[6]), atoll(argv[7]),
                                 atoll(argv[8]), atoll(argv[9]), atoll(argv[10]), atoll(argv[11]), atoll(argv[12]) };
    const struct tf_scene_file_info& s = info.scene;
    const long long have[12] = { info.version, s.n_records, s.n_blocks_stored, info.n_cache_blocks, s.frame_counter, s.lastFreeBlockId,
                                 s.lastFreeExcessListId, s.noVisibleEntries, s.pose_algebra, s.params.n_blocks, s.params.cols,
                                 s.params.rows };
    for (int i = 0; i < 12; ++i)
        if (want[i] != have[i]) { fprintf(stderr, "info field %d: %lld, expected %lld\n", i, have[i], want[i]); return 1; }
    if (s.file_bytes != (long long)file.size()) { fprintf(stderr, "file_bytes\n"); return 1; }

    // every truncated length
    for (size_t len = 0; len < file.size(); ++len) expect_rejected(file, len, "truncated to", (long)len, 0);
    {   // and a byte too many
        std::vector<unsigned char> v = file;
        v.push_back(0);
        expect_rejected(v, v.size(), "extended", 0, 0);
    }

    // every header word.  With the checksums recomputed the structure alone must still refuse: the magic, the
    // version (1 included: its header is another length and has no swapping), the sizes, the table sizes that
    // the section lengths and the records depend on, use_swapping (only 1) and voxel_rgb (only 0), the counters
    // that size a section, the counts, n_cache_blocks.  (A different intrinsic, threshold, pose or frame counter
    // is another valid file: only the checksum tells.)
    const size_t P = TF_SCENE_OFF_PARAMS;
    const size_t fixed_all[] = { 0, 4, TF_SCENE_OFF_VERSION, TF_SCENE_OFF_PARAMS_BYTES, P + offsetof(tf_params, cols),
                                 P + offsetof(tf_params, rows), P + offsetof(tf_params, n_buckets), P + offsetof(tf_params, n_excess),
                                 P + offsetof(tf_params, use_swapping), P + offsetof(tf_params, voxel_rgb),
                                 TF_SCENE_OFF_ALGEBRA + 8, TF_SCENE_OFF_ALGEBRA + 12, TF_SCENE_OFF_ALGEBRA + 16,
                                 TF_SCENE_OFF_COUNTS, TF_SCENE_OFF_COUNTS + 4, TF_SCENE_OFF_COUNTS + 8, TF_SCENE_OFF_COUNTS + 12,
                                 TF_SCENE_OFF_COUNTS + 16, TF_SCENE_OFF_COUNTS + 20, TF_MAP_OFF_CACHE_BLOCKS,
                                 TF_MAP_OFF_CACHE_BLOCKS + 4 };
    for (size_t off = 0; off < TF_MAP_HEADER_BYTES; off += 4) {
        bool fixed = false;
        for (size_t k : fixed_all) fixed = fixed || k == off;
        // n_blocks: one more block is a valid table for these records; every other value is refused
        const bool n_blocks_word = off == P + offsetof(tf_params, n_blocks);
        word_variants(file, off, s.n_records, fixed || n_blocks_word, !n_blocks_word, "header word");
    }

    // the first records' index, ptr, swap state, stored flag and pad byte
    const long long nrec = s.n_records < 6 ? s.n_records : 6;
    for (long long k = 0; k < nrec; ++k) {
        const size_t r = TF_MAP_HEADER_BYTES + (size_t)k * TF_SCENE_RECORD_BYTES;
        word_variants(file, r, s.n_records, false, true, "record index");
        word_variants(file, r + 16, s.n_records, false, true, "record ptr");
        int32_t ptr, prev_idx = -1;
        memcpy(&ptr, file.data() + r + 16, 4);
        if (k > 0) memcpy(&prev_idx, file.data() + r - TF_SCENE_RECORD_BYTES, 4);
        const int32_t bad_idx[4] = { -1, INT_MAX, prev_idx, k > 0 ? 0 : -1 };
        for (int32_t bi : bad_idx) {
            std::vector<unsigned char> v = file;
            memcpy(v.data() + r, &bi, 4);
            fix_crcs(v, s.n_records);
            expect_rejected(v, v.size(), "record index, checksums recomputed", (long)k, (long)bi);
        }
        // a ptr that enters or leaves [0, n_blocks) changes the number of active blocks; INT_MAX lies outside the
        // VBA.  (Inside it another value may name a free block: a valid file but for the checksum.)
        const int32_t ptrs[3] = { ptr >= 0 ? -1 : 0, INT_MAX, ptr >= 0 ? -2 : 1 };
        for (int32_t bp : ptrs) {
            std::vector<unsigned char> v = file;
            memcpy(v.data() + r + 16, &bp, 4);
            fix_crcs(v, s.n_records);
            expect_rejected(v, v.size(), "record ptr, checksums recomputed", (long)k, (long)bp);
        }
        // state: 3 and above are no state; flag: any other value changes the flag count or is no flag; pad: any
        byte_variants(file, r + 21, s.n_records, 3, "record swap state");
        byte_variants(file, r + 22, s.n_records, 0, "record stored flag");
        byte_variants(file, r + 23, s.n_records, 1, "record pad byte");
    }
    if (g_failures) { fprintf(stderr, "%ld of %ld variants accepted\n", g_failures, g_variants); return 1; }
    printf("ok %ld rejected\n", g_variants);
    return 0;
}
