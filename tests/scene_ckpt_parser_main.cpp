// scene_ckpt_parser_main.cpp -- drives the checkpoint file's host parser (topfusion_amd/csrc/tf_scene_file.cpp)
// over a valid file and its damaged variants in one process; tests/test_scene_ckpt_ref.py builds it for
// the CPU with -fsanitize=address,undefined.  Every variant is handed to the validator in a heap buffer
// of exactly its length, so a read past the end is a sanitizer report.
//
//   scene_ckpt_parser_main FILE n_records n_blocks_stored frame_counter lastFreeBlockId lastFreeExcessListId
//                          noVisibleEntries pose_algebra n_blocks cols rows
//
// Prints "ok <variants> rejected" and returns 0 when the intact file is accepted with those info fields
// and every variant is rejected.
#include "../topfusion_amd/csrc/tf_scene_file.h"

#include <limits.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static long g_variants = 0, g_failures = 0;

static tf_status validate_copy(const std::vector<unsigned char>& v, size_t len, struct tf_scene_file_info* info)
{
    unsigned char* exact = (unsigned char*)malloc(len ? len : 1);
    if (!exact) abort();
    if (len) memcpy(exact, v.data(), len);
    TfSceneLayout lay;
    const tf_status s = tf_scene_file_validate(exact, len, info, &lay);
    free(exact);
    return s;
}

static void expect_rejected(const std::vector<unsigned char>& v, size_t len, const char* what, long a, long b)
{
    struct tf_scene_file_info info;
    ++g_variants;
    if (validate_copy(v, len, &info) != TF_INVALID_ARG) {
        ++g_failures;
        fprintf(stderr, "accepted: %s %ld %ld\n", what, a, b);
    }
}

static void fix_crcs(std::vector<unsigned char>& v, long long n_records)
{
    const uint32_t h = tf_scene_crc32(0u, v.data(), TF_SCENE_OFF_CRC);
    const uint32_t r = tf_scene_crc32(0u, v.data() + TF_SCENE_HEADER_BYTES, (size_t)n_records * TF_SCENE_RECORD_BYTES);
    memcpy(v.data() + TF_SCENE_OFF_CRC, &h, 4);
    memcpy(v.data() + TF_SCENE_OFF_RECORDS_CRC, &r, 4);
}

// the 32-bit word at `off` overwritten by 0, -1, INT_MAX and the value one above / below; `also_fixed`:
// again with both checksums recomputed, where the structure alone must refuse the value
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

int main(int argc, char** argv)
{
    if (argc != 12) { fprintf(stderr, "usage\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "no file\n"); return 2; }
    std::vector<unsigned char> file;
    unsigned char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + got);
    fclose(f);

    // the intact file: accepted, the info fields as given; and through the path entry point
    struct tf_scene_file_info info, info2;
    if (validate_copy(file, file.size(), &info) != TF_OK) { fprintf(stderr, "intact file rejected\n"); return 1; }
    if (tf_scene_file_info(argv[1], &info2) != TF_OK || memcmp(&info, &info2, sizeof(info)) != 0) {
        fprintf(stderr, "tf_scene_file_info differs\n");
        return 1;
    }
    const long long want[10] = { atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5]), atoll(argv[6]), atoll(argv[7]),
                                 atoll(argv[8]), atoll(argv[9]), atoll(argv[10]), atoll(argv[11]) };
    const long long have[10] = { info.n_records, info.n_blocks_stored, info.frame_counter, info.lastFreeBlockId,
                                 info.lastFreeExcessListId, info.noVisibleEntries, info.pose_algebra, info.params.n_blocks,
                                 info.params.cols, info.params.rows };
    for (int i = 0; i < 10; ++i)
        if (want[i] != have[i]) { fprintf(stderr, "info field %d: %lld, expected %lld\n", i, have[i], want[i]); return 1; }
    if (info.file_bytes != (long long)file.size()) { fprintf(stderr, "file_bytes\n"); return 1; }

    // every truncated length
    for (size_t len = 0; len < file.size(); ++len) expect_rejected(file, len, "truncated to", (long)len, 0);
    {   // and a byte too many
        std::vector<unsigned char> v = file;
        v.push_back(0);
        expect_rejected(v, v.size(), "extended", 0, 0);
    }

    // every header word.  With the checksums recomputed the structure alone must still refuse: the magic,
    // the version, the sizes, the table sizes that the section lengths and the records depend on, the
    // counters that size a section, the counts.  (A different intrinsic, threshold, pose or frame counter
    // is another valid file: only the checksum tells.)
    const size_t P = TF_SCENE_OFF_PARAMS;
    const size_t fixed_all[] = { 0, 4, TF_SCENE_OFF_VERSION, TF_SCENE_OFF_PARAMS_BYTES, P + offsetof(tf_params, cols),
                                 P + offsetof(tf_params, rows), P + offsetof(tf_params, n_buckets), P + offsetof(tf_params, n_excess),
                                 P + offsetof(tf_params, use_swapping), P + offsetof(tf_params, voxel_rgb),
                                 TF_SCENE_OFF_ALGEBRA + 8, TF_SCENE_OFF_ALGEBRA + 12, TF_SCENE_OFF_ALGEBRA + 16,
                                 TF_SCENE_OFF_COUNTS, TF_SCENE_OFF_COUNTS + 4, TF_SCENE_OFF_COUNTS + 8, TF_SCENE_OFF_COUNTS + 12,
                                 TF_SCENE_OFF_COUNTS + 16, TF_SCENE_OFF_COUNTS + 20 };
    for (size_t off = 0; off < TF_SCENE_HEADER_BYTES; off += 4) {
        bool fixed = false;
        for (size_t k : fixed_all) fixed = fixed || k == off;
        // n_blocks: one more block is a valid table for these records; every other value is refused
        const bool n_blocks_word = off == P + offsetof(tf_params, n_blocks);
        word_variants(file, off, info.n_records, fixed || n_blocks_word, !n_blocks_word, "header word");
    }

    // the first records' index and ptr
    const long long nrec = info.n_records < 4 ? info.n_records : 4;
    for (long long k = 0; k < nrec; ++k) {
        const size_t r = TF_SCENE_HEADER_BYTES + (size_t)k * TF_SCENE_RECORD_BYTES;
        word_variants(file, r, info.n_records, false, true, "record index");
        word_variants(file, r + 16, info.n_records, false, true, "record ptr");
        int32_t ptr, prev_idx = -1;
        memcpy(&ptr, file.data() + r + 16, 4);
        if (k > 0) memcpy(&prev_idx, file.data() + r - TF_SCENE_RECORD_BYTES, 4);
        // with the checksums recomputed: an index outside the table or not above the one before; a ptr that
        // enters or leaves [0, n_blocks) changes the number of stored blocks, and inside it (every block of the
        // scene is in use) names a block twice or lies outside the VBA
        const int32_t bad_idx[4] = { -1, INT_MAX, prev_idx, k > 0 ? 0 : -1 };
        for (int32_t bi : bad_idx) {
            std::vector<unsigned char> v = file;
            memcpy(v.data() + r, &bi, 4);
            fix_crcs(v, info.n_records);
            expect_rejected(v, v.size(), "record index, checksums recomputed", (long)k, (long)bi);
        }
        const int32_t ptrs[5] = { 0, -1, INT_MAX, ptr - 1, ptr + 1 };
        for (int32_t bp : ptrs) {
            if (bp == ptr || (bp < 0 && ptr < 0)) continue;
            std::vector<unsigned char> v = file;
            memcpy(v.data() + r + 16, &bp, 4);
            fix_crcs(v, info.n_records);
            expect_rejected(v, v.size(), "record ptr, checksums recomputed", (long)k, (long)bp);
        }
    }
    if (g_failures) { fprintf(stderr, "%ld of %ld variants accepted\n", g_failures, g_variants); return 1; }
    printf("ok %ld rejected\n", g_variants);
    return 0;
}
