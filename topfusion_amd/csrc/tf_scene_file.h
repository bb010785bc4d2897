// tf_scene_file.h -- the scene checkpoint file (DESIGN.md §5 Scene checkpoints): layout, header
// encoding and validation.  Host C++ with no HIP call: this is the code that reads untrusted
// bytes, and it compiles on its own for a CPU (tests/test_scene_ckpt_ref.py runs it under
// AddressSanitizer / UBSan from a stand-alone program).
//
// Little-endian, fixed order:
//   header   TF_SCENE_HEADER_BYTES
//   records  n_records x 24 B: u32 entry index, the 16-byte HashEntry, u8 visType, 3 zero bytes;
//            ascending entry index; an entry has one when its HashEntry is not ResetScene's
//            {0,0,0,0, 0, -2} or its visType is non-zero
//   blocks   in record order, for records with ptr >= 0: 2048 B of voxels, then (voxel_rgb) 2048 B of colour
//   visibleIds[0, noVisibleEntries)                       4 B each
//   allocList[0, lastFreeBlockId + 1)                     4 B each
//   excessList[0, lastFreeExcessListId + 1)               4 B each
//   maps     previous points then normals of level 0, 1, 2: 16 B x (cols >> l) x (rows >> l) each
//
// Version 2, the map checkpoint of a swapping context (DESIGN.md §5 Map checkpoints; use_swapping == 1,
// voxel_rgb == 0, so a block is always 2048 B):
//   header   TF_MAP_HEADER_BYTES: bytes [0, 288) as version 1 with version = 2 and this layout's
//            file_bytes; i64 n_cache_blocks at 288; CRC-32 of [0, 296) at 296, of the records at 300
//   records  n_records x 24 B: u32 entry index, the HashEntry, u8 visType, u8 swapState (0..2),
//            u8 hasStoredData (0 / 1), one zero byte; an entry has one when its HashEntry is not
//            ResetScene's or any of the three bytes is non-zero (an entry with no hash entry left but a
//            stored block still has one)
//   blocks   active blocks, in record order, for records with ptr >= 0
//   stored   GlobalCache blocks, in record order, for records with hasStoredData: n_cache_blocks of them
//   visibleIds, allocList, excessList, maps as version 1
//   file_bytes = 304 + 24 R + 2048 (b + s) + 4 (V + A + E) + M
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/tfusion_hip.h"

#define TF_SCENE_VERSION 1u
#define TF_SCENE_HEADER_BYTES 296
#define TF_SCENE_RECORD_BYTES 24
#define TF_SCENE_BLOCK_BYTES 2048          // 512 voxels x 4 B (and as much colour)
#define TF_SCENE_LEVELS 3
// header offsets
#define TF_SCENE_OFF_MAGIC 0               // "TFSCENE\0"
#define TF_SCENE_OFF_VERSION 8             // u32
#define TF_SCENE_OFF_PARAMS_BYTES 12       // u32 sizeof(tf_params)
#define TF_SCENE_OFF_PARAMS 16             // tf_params (180 B)
#define TF_SCENE_OFF_ALGEBRA 196           // i32 x 5: pose_algebra, frame_counter, lastFreeBlockId,
#define TF_SCENE_OFF_COUNTS 216            //   lastFreeExcessListId, noVisibleEntries; i64 x 3: n_records,
#define TF_SCENE_OFF_POSE 240              //   n_blocks_stored, file_bytes; float[12] pose
#define TF_SCENE_OFF_CRC 288               // u32 CRC-32 (IEEE, zlib's) of the header bytes [0, 288)
#define TF_SCENE_OFF_RECORDS_CRC 292       // u32 CRC-32 of the records section
// version 2: the same offsets up to 288, then
#define TF_MAP_VERSION 2u
#define TF_MAP_HEADER_BYTES 304
#define TF_MAP_OFF_CACHE_BLOCKS 288        // i64 n_cache_blocks
#define TF_MAP_OFF_CRC 296                 // u32 CRC-32 of the header bytes [0, 296)
#define TF_MAP_OFF_RECORDS_CRC 300         // u32 CRC-32 of the records section

// where the sections of a file with these counts lie
struct TfSceneLayout {
    size_t records_off, blocks_off, vis_off, alloc_off, excess_off, maps_off, file_bytes;
    size_t block_bytes;                    // per stored block: 2048, or 4096 with colour
    size_t n_vis, n_alloc, n_excess;       // list slots stored
    size_t map_bytes[TF_SCENE_LEVELS];     // one map (points or normals) of the level
    size_t stored_off, n_stored;           // version 2: the GlobalCache blocks' section (n_stored = 0 in version 1)
};

// zlib's crc32: start with crc = 0, feed the result back in to continue
uint32_t tf_scene_crc32(uint32_t crc, const unsigned char* p, size_t n);
// true when the params and counters describe a file (sizes positive and bounded, counters within
// their lists); fills the layout from them (n_records / n_blocks_stored as given in info)
bool tf_scene_layout(const struct tf_scene_file_info* info, TfSceneLayout* lay);
// the header of a file with info's params, counters, counts, file_bytes and pose, and the records' checksum
void tf_scene_header_encode(const struct tf_scene_file_info* info, uint32_t records_crc, unsigned char hdr[TF_SCENE_HEADER_BYTES]);
// the header alone: magic, version, sizes, its checksum, tf_scene_layout, file_bytes == the layout's
tf_status tf_scene_header_decode(const unsigned char* hdr, size_t len, struct tf_scene_file_info* info, TfSceneLayout* lay);
// the record table on its own (save checks what it is about to write by the rule load will apply): ascending
// indices < n_total, zero padding, chain offsets and ptr within the tables, no record for ResetScene's entry,
// ptr >= 0 distinct and n_blocks_stored of them; and n list values within [0, bound)
tf_status tf_scene_records_check(const unsigned char* records, long long n_records, const tf_params* p, long long n_blocks_stored);
bool tf_scene_list_within(const unsigned char* values, size_t n, int32_t bound);
// a whole file in memory: the header, len == file_bytes, the records (their checksum; ascending indices < n_total,
// canonical, chain offsets and ptr within the tables, ptr >= 0 distinct and n_blocks_stored of
// them), the list values within their tables.  TF_OK or TF_INVALID_ARG (TF_OOM: no scratch).
tf_status tf_scene_file_validate(const unsigned char* data, size_t len, struct tf_scene_file_info* info, TfSceneLayout* lay);

// the map merge's rule over a validated record table (tf_map_merge): every carried record (ptr >= 0) moved by
// block_offset (NULL: none) keeps its position inside the int16 range, and no two carried records share a position.
// *n_carried: the records with ptr >= 0.  TF_OK or TF_INVALID_ARG (TF_OOM: no scratch)
tf_status tf_merge_records_check(const unsigned char* records, long long n_records, const int block_offset[3], long long* n_carried);

// ---- both versions (tf_map_save / tf_map_load / tf_map_file_info) ----
// as tf_scene_layout, by info->version: 1 is tf_scene_layout itself (n_cache_blocks must be 0); 2 requires
// use_swapping == 1, voxel_rgb == 0 and 0 <= n_cache_blocks <= n_records
bool tf_map_layout(const struct tf_map_file_info* info, TfSceneLayout* lay);
// the version-2 header (info->version is not read)
void tf_map_header_encode(const struct tf_map_file_info* info, uint32_t records_crc, unsigned char hdr[TF_MAP_HEADER_BYTES]);
// the header of either version (len >= the version's header bytes)
tf_status tf_map_header_decode(const unsigned char* hdr, size_t len, struct tf_map_file_info* info, TfSceneLayout* lay);
// version 2's record table: tf_scene_records_check's rules with the record's bytes 21 (swapState <= 2), 22
// (hasStoredData <= 1) and 23 (zero), no record with every field at its reset value, and n_cache_blocks flags
tf_status tf_map_records_check(const unsigned char* records, long long n_records, const tf_params* p, long long n_blocks_stored,
                               long long n_cache_blocks);
// a whole file of either version in memory, as tf_scene_file_validate
tf_status tf_map_file_validate(const unsigned char* data, size_t len, struct tf_map_file_info* info, TfSceneLayout* lay);
