// tf_scene_file.cpp -- the scene checkpoint file's header, layout and validation (tf_scene_file.h).
// Host only, no HIP call.  Every read of the file's bytes goes through memcpy at an offset checked
// against the length first; every size is formed in 64 bits from fields bounded before.
#include "tf_scene_file.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const unsigned char k_magic[8] = { 'T', 'F', 'S', 'C', 'E', 'N', 'E', 0 };

// CRC-32 (IEEE 802.3, as zlib's crc32): crc = 0 starts, the result continues over the next piece.
// Slicing by eight over tables built at compile time (nothing to initialise at run time, so
// contexts on several threads share them freely); little-endian words, as the file itself.
struct CrcTables {
    uint32_t t[8][256];
    constexpr CrcTables() : t()
    {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int k = 1; k < 8; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 255u];
    }
};
static constexpr CrcTables k_crc;

uint32_t tf_scene_crc32(uint32_t crc, const unsigned char* p, size_t n)
{
    uint32_t c = ~crc;
    for (; n >= 8; n -= 8, p += 8) {
        uint32_t a, b;
        memcpy(&a, p, 4);
        memcpy(&b, p + 4, 4);
        a ^= c;
        c = k_crc.t[7][a & 255u] ^ k_crc.t[6][a >> 8 & 255u] ^ k_crc.t[5][a >> 16 & 255u] ^ k_crc.t[4][a >> 24] ^
            k_crc.t[3][b & 255u] ^ k_crc.t[2][b >> 8 & 255u] ^ k_crc.t[1][b >> 16 & 255u] ^ k_crc.t[0][b >> 24];
    }
    for (size_t i = 0; i < n; ++i) c = k_crc.t[0][(c ^ p[i]) & 255u] ^ (c >> 8);
    return ~c;
}

static void put32(unsigned char* p, uint32_t v) { memcpy(p, &v, 4); }
static void put64(unsigned char* p, uint64_t v) { memcpy(p, &v, 8); }
static uint32_t get32(const unsigned char* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static int64_t get64(const unsigned char* p) { int64_t v; memcpy(&v, p, 8); return v; }

// the layout of either version: version 2 is a swapping context's (no colour plane), with n_cache stored blocks
static bool layout_of(const struct tf_scene_file_info* info, unsigned version, long long n_cache, TfSceneLayout* lay)
{
    const tf_params& p = info->params;
    // the bounds tf_create puts on a context's tables (params_valid, tf_capi.hip), so that every
    // product below fits 64 bits with room to spare
    if (p.cols <= 0 || p.rows <= 0 || p.cols > 65535 || p.rows > 65535 || (p.cols % 4) || (p.rows % 4)) return false;
    if (p.n_buckets <= 0 || (p.n_buckets & (p.n_buckets - 1)) || p.n_buckets > (1 << 30)) return false;
    if (p.n_excess <= 0 || p.n_excess > (1 << 30) || ((p.n_buckets + p.n_excess) % 16)) return false;
    if (p.n_blocks <= 0 || p.n_blocks > (1 << 21) - 1) return false;
    if (p.vis_capacity <= 0) return false;
    if (version == TF_SCENE_VERSION) {
        if (p.use_swapping != 0 || n_cache != 0) return false;     // (voxel_rgb: any non-zero value is a colour context, as tf_create takes it)
    } else if (p.use_swapping != 1 || p.voxel_rgb != 0) return false;
    const long long n_total = (long long)p.n_buckets + p.n_excess;
    if (info->lastFreeBlockId < -1 || info->lastFreeBlockId >= p.n_blocks) return false;
    if (info->lastFreeExcessListId < -1 || info->lastFreeExcessListId >= p.n_excess) return false;
    if (info->noVisibleEntries < 0 || info->noVisibleEntries > p.vis_capacity) return false;
    if (info->frame_counter < 0) return false;
    if (info->n_records < 0 || info->n_records > n_total) return false;
    if (info->n_blocks_stored < 0 || info->n_blocks_stored > info->n_records || info->n_blocks_stored > p.n_blocks) return false;
    if (n_cache < 0 || n_cache > info->n_records) return false;
    lay->block_bytes = (size_t)TF_SCENE_BLOCK_BYTES * (p.voxel_rgb ? 2 : 1);
    lay->n_vis = (size_t)info->noVisibleEntries;
    lay->n_alloc = (size_t)(info->lastFreeBlockId + 1);
    lay->n_excess = (size_t)(info->lastFreeExcessListId + 1);
    lay->records_off = version == TF_SCENE_VERSION ? TF_SCENE_HEADER_BYTES : TF_MAP_HEADER_BYTES;
    lay->blocks_off = lay->records_off + (size_t)info->n_records * TF_SCENE_RECORD_BYTES;
    lay->stored_off = lay->blocks_off + (size_t)info->n_blocks_stored * lay->block_bytes;
    lay->n_stored = (size_t)n_cache;
    lay->vis_off = lay->stored_off + lay->n_stored * TF_SCENE_BLOCK_BYTES;
    lay->alloc_off = lay->vis_off + 4 * lay->n_vis;
    lay->excess_off = lay->alloc_off + 4 * lay->n_alloc;
    lay->maps_off = lay->excess_off + 4 * lay->n_excess;
    size_t maps = 0;
    for (int l = 0; l < TF_SCENE_LEVELS; ++l) {
        lay->map_bytes[l] = (size_t)16 * (size_t)(p.cols >> l) * (size_t)(p.rows >> l);
        maps += 2 * lay->map_bytes[l];
    }
    lay->file_bytes = lay->maps_off + maps;
    return true;
}

bool tf_scene_layout(const struct tf_scene_file_info* info, TfSceneLayout* lay)
{
    return layout_of(info, TF_SCENE_VERSION, 0, lay);
}

bool tf_map_layout(const struct tf_map_file_info* info, TfSceneLayout* lay)
{
    if (info->version != (int)TF_SCENE_VERSION && info->version != (int)TF_MAP_VERSION) return false;
    return layout_of(&info->scene, (unsigned)info->version, info->n_cache_blocks, lay);
}

// bytes [0, 288) of either version's header
static void header_fields_encode(const struct tf_scene_file_info* info, uint32_t version, unsigned char* hdr)
{
    static_assert(sizeof(tf_params) == 180, "the header stores tf_params as it is laid out");
    memset(hdr, 0, TF_SCENE_OFF_CRC);
    memcpy(hdr + TF_SCENE_OFF_MAGIC, k_magic, 8);
    put32(hdr + TF_SCENE_OFF_VERSION, version);
    put32(hdr + TF_SCENE_OFF_PARAMS_BYTES, (uint32_t)sizeof(tf_params));
    memcpy(hdr + TF_SCENE_OFF_PARAMS, &info->params, sizeof(tf_params));
    const int32_t ints[5] = { info->pose_algebra, info->frame_counter, info->lastFreeBlockId, info->lastFreeExcessListId,
                              info->noVisibleEntries };
    memcpy(hdr + TF_SCENE_OFF_ALGEBRA, ints, sizeof(ints));
    put64(hdr + TF_SCENE_OFF_COUNTS, (uint64_t)info->n_records);
    put64(hdr + TF_SCENE_OFF_COUNTS + 8, (uint64_t)info->n_blocks_stored);
    put64(hdr + TF_SCENE_OFF_COUNTS + 16, (uint64_t)info->file_bytes);
    memcpy(hdr + TF_SCENE_OFF_POSE, info->pose, sizeof(float) * 12);
}

void tf_scene_header_encode(const struct tf_scene_file_info* info, uint32_t records_crc, unsigned char hdr[TF_SCENE_HEADER_BYTES])
{
    header_fields_encode(info, TF_SCENE_VERSION, hdr);
    put32(hdr + TF_SCENE_OFF_CRC, tf_scene_crc32(0u, hdr, TF_SCENE_OFF_CRC));
    put32(hdr + TF_SCENE_OFF_RECORDS_CRC, records_crc);
}

void tf_map_header_encode(const struct tf_map_file_info* info, uint32_t records_crc, unsigned char hdr[TF_MAP_HEADER_BYTES])
{
    header_fields_encode(&info->scene, TF_MAP_VERSION, hdr);
    put64(hdr + TF_MAP_OFF_CACHE_BLOCKS, (uint64_t)info->n_cache_blocks);
    put32(hdr + TF_MAP_OFF_CRC, tf_scene_crc32(0u, hdr, TF_MAP_OFF_CRC));
    put32(hdr + TF_MAP_OFF_RECORDS_CRC, records_crc);
}

// a header of `version` (1 or 2): magic, version, sizes, checksum, the fields, the layout, file_bytes
static tf_status header_decode(const unsigned char* hdr, size_t len, uint32_t version, struct tf_scene_file_info* info,
                               long long* n_cache, TfSceneLayout* lay)
{
    const bool v1 = version == TF_SCENE_VERSION;
    const size_t hdr_bytes = v1 ? TF_SCENE_HEADER_BYTES : TF_MAP_HEADER_BYTES, crc_off = v1 ? TF_SCENE_OFF_CRC : TF_MAP_OFF_CRC;
    if (!hdr || !info || !lay || len < hdr_bytes) return TF_INVALID_ARG;
    if (memcmp(hdr + TF_SCENE_OFF_MAGIC, k_magic, 8) != 0) return TF_INVALID_ARG;
    if (get32(hdr + TF_SCENE_OFF_VERSION) != version) return TF_INVALID_ARG;
    if (get32(hdr + TF_SCENE_OFF_PARAMS_BYTES) != (uint32_t)sizeof(tf_params)) return TF_INVALID_ARG;
    if (get32(hdr + crc_off) != tf_scene_crc32(0u, hdr, crc_off)) return TF_INVALID_ARG;
    *n_cache = v1 ? 0 : get64(hdr + TF_MAP_OFF_CACHE_BLOCKS);
    memset(info, 0, sizeof(*info));
    memcpy(&info->params, hdr + TF_SCENE_OFF_PARAMS, sizeof(tf_params));
    int32_t ints[5];
    memcpy(ints, hdr + TF_SCENE_OFF_ALGEBRA, sizeof(ints));
    info->pose_algebra = ints[0]; info->frame_counter = ints[1]; info->lastFreeBlockId = ints[2];
    info->lastFreeExcessListId = ints[3]; info->noVisibleEntries = ints[4];
    info->n_records = get64(hdr + TF_SCENE_OFF_COUNTS);
    info->n_blocks_stored = get64(hdr + TF_SCENE_OFF_COUNTS + 8);
    info->file_bytes = get64(hdr + TF_SCENE_OFF_COUNTS + 16);
    memcpy(info->pose, hdr + TF_SCENE_OFF_POSE, sizeof(float) * 12);
    if (!layout_of(info, version, *n_cache, lay)) return TF_INVALID_ARG;
    if (info->file_bytes < 0 || (unsigned long long)info->file_bytes != (unsigned long long)lay->file_bytes) return TF_INVALID_ARG;
    return TF_OK;
}

tf_status tf_scene_header_decode(const unsigned char* hdr, size_t len, struct tf_scene_file_info* info, TfSceneLayout* lay)
{
    long long n_cache;
    return header_decode(hdr, len, TF_SCENE_VERSION, info, &n_cache, lay);
}

tf_status tf_map_header_decode(const unsigned char* hdr, size_t len, struct tf_map_file_info* info, TfSceneLayout* lay)
{
    if (!hdr || !info || !lay || len < TF_SCENE_OFF_VERSION + 4) return TF_INVALID_ARG;
    const uint32_t version = get32(hdr + TF_SCENE_OFF_VERSION);
    if (version != TF_SCENE_VERSION && version != TF_MAP_VERSION) return TF_INVALID_ARG;
    struct tf_map_file_info tmp;
    memset(&tmp, 0, sizeof(tmp));
    const tf_status s = header_decode(hdr, len, version, &tmp.scene, &tmp.n_cache_blocks, lay);
    if (s != TF_OK) return s;
    tmp.version = (int)version;
    *info = tmp;
    return TF_OK;
}

bool tf_scene_list_within(const unsigned char* p, size_t n, int32_t bound)
{
    for (size_t i = 0; i < n; ++i) {
        const int32_t v = (int32_t)get32(p + 4 * i);
        if (v < 0 || v >= bound) return false;
    }
    return true;
}

// version 1: bytes 21..23 are padding; version 2: swapState, hasStoredData, one padding byte
static tf_status records_check(const unsigned char* r, long long n_records, const tf_params* pp, long long n_blocks_stored, bool v2,
                               long long n_cache_blocks)
{
    const tf_params& p = *pp;
    const int64_t n_total = (int64_t)p.n_buckets + p.n_excess;
    unsigned char* used = (unsigned char*)calloc(((size_t)p.n_blocks + 7) / 8, 1);     // ptr seen
    if (!used) return TF_OOM;
    tf_status s = TF_OK;
    int64_t prev = -1, stored = 0, cached = 0;
    for (long long k = 0; k < n_records && s == TF_OK; ++k, r += TF_SCENE_RECORD_BYTES) {
        const int64_t idx = (int64_t)get32(r);
        int16_t xyzp[4];
        memcpy(xyzp, r + 4, 8);
        const int32_t offset = (int32_t)get32(r + 12), ptr = (int32_t)get32(r + 16);
        const unsigned char vis = r[20];
        if (idx <= prev || idx >= n_total) s = TF_INVALID_ARG;                 // strictly ascending, in the table
        else if (v2 ? (r[21] > 2 || r[22] > 1 || r[23]) : (r[21] | r[22] | r[23])) s = TF_INVALID_ARG;   // padding; state, flag
        else if (offset > p.n_excess) s = TF_INVALID_ARG;                      // the chain's next entry: n_buckets + offset - 1
        else if (ptr >= p.n_blocks) s = TF_INVALID_ARG;
        else if (!(xyzp[0] | xyzp[1] | xyzp[2] | xyzp[3]) && offset == 0 && ptr == -2 && vis == 0 && !(r[21] | r[22]))
            s = TF_INVALID_ARG;                                                // ResetScene's entry has no record
        else if (ptr >= 0) {
            if (used[ptr >> 3] >> (ptr & 7) & 1) s = TF_INVALID_ARG;           // two entries, one block
            used[ptr >> 3] |= (unsigned char)(1u << (ptr & 7));
            ++stored;
        }
        if (s == TF_OK && v2) cached += r[22];
        prev = idx;
    }
    free(used);
    if (s != TF_OK) return s;
    return stored == n_blocks_stored && cached == n_cache_blocks ? TF_OK : TF_INVALID_ARG;
}

tf_status tf_scene_records_check(const unsigned char* r, long long n_records, const tf_params* pp, long long n_blocks_stored)
{
    return records_check(r, n_records, pp, n_blocks_stored, false, 0);
}

tf_status tf_map_records_check(const unsigned char* r, long long n_records, const tf_params* pp, long long n_blocks_stored,
                               long long n_cache_blocks)
{
    return records_check(r, n_records, pp, n_blocks_stored, true, n_cache_blocks);
}

// the map merge's own rule over a validated record table (tf_map_merge, DESIGN.md §5 Map merge): the carried
// records (ptr >= 0) moved by block_offset stay inside the int16 range, and no two of them share a position.
// The positions as 48-bit keys, sorted: equal neighbours are a duplicate.
static int key_cmp(const void* a, const void* b)
{
    const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
    return x < y ? -1 : x > y ? 1 : 0;
}

tf_status tf_merge_records_check(const unsigned char* r, long long n_records, const int block_offset[3], long long* n_carried)
{
    if (n_records < 0 || (!r && n_records > 0) || !n_carried) return TF_INVALID_ARG;
    *n_carried = 0;
    uint64_t* keys = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)(n_records > 0 ? n_records : 1));
    if (!keys) return TF_OOM;
    size_t n = 0;
    tf_status s = TF_OK;
    for (long long k = 0; k < n_records && s == TF_OK; ++k, r += TF_SCENE_RECORD_BYTES) {
        if ((int32_t)get32(r + 16) < 0) continue;
        int16_t xyz[3];
        memcpy(xyz, r + 4, 6);
        uint64_t key = 0;
        for (int a = 0; a < 3; ++a) {
            const int64_t v = (int64_t)xyz[a] + (block_offset ? (int64_t)block_offset[a] : 0);
            if (v < INT16_MIN || v > INT16_MAX) s = TF_INVALID_ARG;
            key = key << 16 | (uint64_t)(uint16_t)(int16_t)(s == TF_OK ? v : 0);
        }
        keys[n++] = key;
    }
    if (s == TF_OK) {
        qsort(keys, n, sizeof(uint64_t), key_cmp);
        for (size_t i = 1; i < n && s == TF_OK; ++i)
            if (keys[i] == keys[i - 1]) s = TF_INVALID_ARG;
    }
    free(keys);
    *n_carried = (long long)n;
    return s;
}

// what follows a decoded header of either version
static tf_status body_validate(const unsigned char* data, size_t len, const struct tf_scene_file_info* info, bool v2, long long n_cache,
                               const TfSceneLayout* lay)
{
    if (len != lay->file_bytes) return TF_INVALID_ARG;
    const tf_params& p = info->params;
    const int64_t n_total = (int64_t)p.n_buckets + p.n_excess;
    if (get32(data + (v2 ? TF_MAP_OFF_RECORDS_CRC : TF_SCENE_OFF_RECORDS_CRC)) !=
        tf_scene_crc32(0u, data + lay->records_off, (size_t)info->n_records * TF_SCENE_RECORD_BYTES))
        return TF_INVALID_ARG;
    const tf_status rs = records_check(data + lay->records_off, info->n_records, &p, info->n_blocks_stored, v2, n_cache);
    if (rs != TF_OK) return rs;
    if (!tf_scene_list_within(data + lay->vis_off, lay->n_vis, (int32_t)n_total)) return TF_INVALID_ARG;
    if (!tf_scene_list_within(data + lay->alloc_off, lay->n_alloc, p.n_blocks)) return TF_INVALID_ARG;
    if (!tf_scene_list_within(data + lay->excess_off, lay->n_excess, p.n_excess)) return TF_INVALID_ARG;
    return TF_OK;
}

tf_status tf_scene_file_validate(const unsigned char* data, size_t len, struct tf_scene_file_info* info, TfSceneLayout* lay)
{
    const tf_status hs = tf_scene_header_decode(data, len, info, lay);
    return hs != TF_OK ? hs : body_validate(data, len, info, false, 0, lay);
}

tf_status tf_map_file_validate(const unsigned char* data, size_t len, struct tf_map_file_info* info, TfSceneLayout* lay)
{
    const tf_status hs = tf_map_header_decode(data, len, info, lay);
    return hs != TF_OK ? hs : body_validate(data, len, &info->scene, info->version == (int)TF_MAP_VERSION, info->n_cache_blocks, lay);
}

extern "C" tf_status tf_scene_file_info(const char* path, struct tf_scene_file_info* info)
{
    if (!path || !info) return TF_INVALID_ARG;
    FILE* f = fopen(path, "rb");
    if (!f) return TF_INVALID_ARG;
    unsigned char hdr[TF_SCENE_HEADER_BYTES];
    const size_t got = fread(hdr, 1, sizeof(hdr), f);
    long long size = -1;
    if (fseeko(f, 0, SEEK_END) == 0) size = (long long)ftello(f);
    fclose(f);
    struct tf_scene_file_info tmp;
    TfSceneLayout lay;
    const tf_status s = tf_scene_header_decode(hdr, got, &tmp, &lay);
    if (s != TF_OK) return s;
    if (size != tmp.file_bytes) return TF_INVALID_ARG;
    *info = tmp;
    return TF_OK;
}

extern "C" tf_status tf_map_file_info(const char* path, struct tf_map_file_info* info)
{
    if (!path || !info) return TF_INVALID_ARG;
    FILE* f = fopen(path, "rb");
    if (!f) return TF_INVALID_ARG;
    unsigned char hdr[TF_MAP_HEADER_BYTES];
    const size_t got = fread(hdr, 1, sizeof(hdr), f);
    long long size = -1;
    if (fseeko(f, 0, SEEK_END) == 0) size = (long long)ftello(f);
    fclose(f);
    struct tf_map_file_info tmp;
    TfSceneLayout lay;
    const tf_status s = tf_map_header_decode(hdr, got, &tmp, &lay);
    if (s != TF_OK) return s;
    if (size != tmp.scene.file_bytes) return TF_INVALID_ARG;
    *info = tmp;
    return TF_OK;
}
