// tf_mesh_dev.h -- what the mesh extraction's translation units share on the device side (tf_mesh.hip: the
// triangle soup; tf_mesh_indexed.hip: the indexed form): the scene view, the block look-ups and the LDS
// tiles of a hash entry's cube corners.
#pragma once

#include "tf_internal.h"
#include "tf_mesh.h"

#define TFM_WG 512               // threads per workgroup = voxels per block = entries per group
#define TFM_TILE 9
#define TFM_TILE3 (TFM_TILE * TFM_TILE * TFM_TILE)
#define TFM_GRID 2048            // workgroups of the count / emit passes (groups are taken round robin)
#define TFM_SCAN_GROUPS 4        // groups (of TFM_WG entries) per k_mesh_prefix workgroup

struct MeshScene {
    SceneView v;                 // v.vba: the guard block of Voxel_s() (sdf 32767, w 0), then the VBA -- a missing block reads it
    int n_total;
};

// (hash entry, VBA voxel offset) of a neighbour block; a block coordinate outside the short range,
// a block the hash does not hold, and a swapped-out entry (ptr -1) are all missing
__device__ __forceinline__ int mesh_block_voff(const MeshScene& s, int bx, int by, int bz)
{
    if (tf_grid_in(bx, by, bz)) return s.v.grid[tf_grid_cell(bx, by, bz)].y;
    if (bx > 32767 || by > 32767 || bz > 32767) return TF_VOFF_NONE;
    return blk_walk(s.v, bx, by, bz).y;
}

// The entry's 729 corner voxels into LDS (sdf | w << 16 per voxel, index x + 9 y + 81 z).  All
// threads of the workgroup call it; e is uniform.
__device__ __forceinline__ void mesh_stage(const MeshScene& s, const TfHashEntry& e, unsigned* tile, int* nvoff)
{
    const int t = threadIdx.x;
    __syncthreads();             // the previous entry's reads of tile / nvoff are done
    if (t < 8) {
        const int dx = t & 1, dy = t >> 1 & 1, dz = t >> 2;
        nvoff[t] = t == 0 ? e.ptr * TF_BLK3 : mesh_block_voff(s, e.x + dx, e.y + dy, e.z + dz);
    }
    __syncthreads();
    for (int i = t; i < TFM_TILE3; i += TFM_WG) {
        const int z = i / (TFM_TILE * TFM_TILE), r = i - z * (TFM_TILE * TFM_TILE), y = r / TFM_TILE, x = r - y * TFM_TILE;
        const int voff = nvoff[(x >> 3) | (y >> 3) << 1 | (z >> 3) << 2];
        const TfVoxel v = s.v.vba[TF_BLK3 + voff + (x & 7) + ((y & 7) << 3) + ((z & 7) << 6)];
        tile[i] = (unsigned)(unsigned short)v.sdf | (unsigned)v.w << 16;
    }
    __syncthreads();
}

// this thread's cube: voxel threadIdx.x = x + 8 y + 64 z
__device__ __forceinline__ TfmCube mesh_cube(const unsigned* tile)
{
    const int t = threadIdx.x, x = t & 7, y = t >> 3 & 7, z = t >> 6;
    const int b = x + TFM_TILE * y + TFM_TILE * TFM_TILE * z;
    TfmCube q;
    unsigned wmin = 255u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const unsigned v = tile[b + (c & 1) + TFM_TILE * (c >> 1 & 1) + TFM_TILE * TFM_TILE * (c >> 2)];
        q.sdf[c] = (int)(short)(v & 0xffffu);
        wmin = min(wmin, v >> 16);
    }
    q.valid = wmin > 0;
    return q;
}

// ---- the attributed tile (k_mesh_emit_attr, k_mesh_emit_vertices) ----
#define TFM_ATILE 11
#define TFM_ATILE3 (TFM_ATILE * TFM_ATILE * TFM_ATILE)

// mesh_block_voff for offsets that also step down: block -32769 does not exist either (blk_walk
// compares shorts and would wrap)
__device__ __forceinline__ int mesh_block_voff_attr(const MeshScene& s, int bx, int by, int bz)
{
    if (tf_grid_in(bx, by, bz)) return s.v.grid[tf_grid_cell(bx, by, bz)].y;
    if (bx > 32767 || by > 32767 || bz > 32767 || bx < -32768 || by < -32768 || bz < -32768) return TF_VOFF_NONE;
    return blk_walk(s.v, bx, by, bz).y;
}

// tile: sdf | w << 16 at (x + 1) + 11 (y + 1) + 121 (z + 1), x, y, z in -1 .. 9 (NORMALS; else 0 .. 8 only,
// the rim reads as w = 0); ctile: colour words at x + 9 y + 81 z (COLOURS); nvoff: the 27 block offsets
// (ox + 1) + 3 (oy + 1) + 9 (oz + 1), those with more than one -1 (without NORMALS: any -1) unused
template <bool NORMALS, bool COLOURS>
__device__ __forceinline__ void mesh_stage_attr(const MeshScene& s, const unsigned* __restrict__ rgb, const TfHashEntry& e, unsigned* tile,
                                                unsigned* ctile, int* nvoff)
{
    const int t = threadIdx.x;
    __syncthreads();             // the previous entry's reads of tile / gradients / ctile / nvoff are done
    if (t < 27) {
        const int ox = t % 3 - 1, oy = t / 3 % 3 - 1, oz = t / 9 - 1;
        const int down = (ox < 0) + (oy < 0) + (oz < 0);
        int voff = TF_VOFF_NONE;
        if (t == 13) voff = e.ptr * TF_BLK3;
        else if (down <= (NORMALS ? 1 : 0)) voff = mesh_block_voff_attr(s, e.x + ox, e.y + oy, e.z + oz);
        nvoff[t] = voff;
    }
    __syncthreads();
    for (int i = t; i < TFM_ATILE3; i += TFM_WG) {
        const int zi = i / (TFM_ATILE * TFM_ATILE), r = i - zi * (TFM_ATILE * TFM_ATILE), yi = r / TFM_ATILE, xi = r - yi * TFM_ATILE;
        const int x = xi - 1, y = yi - 1, z = zi - 1;
        const int rim = ((unsigned)x > 8u) + ((unsigned)y > 8u) + ((unsigned)z > 8u);
        unsigned packed = 0u;
        if (rim <= (NORMALS ? 1 : 0)) {
            const int voff = nvoff[((x >> 3) + 1) + 3 * ((y >> 3) + 1) + 9 * ((z >> 3) + 1)];
            const int at = TF_BLK3 + voff + (x & 7) + ((y & 7) << 3) + ((z & 7) << 6);
            const TfVoxel v = s.v.vba[at];
            packed = (unsigned)(unsigned short)v.sdf | (unsigned)v.w << 16;
            if (COLOURS && rim == 0) ctile[x + TFM_TILE * y + TFM_TILE * TFM_TILE * z] = rgb[at];
        }
        tile[i] = packed;
    }
    __syncthreads();
}

// this thread's cube from the 11-wide tile
__device__ __forceinline__ TfmCube mesh_cube_attr(const unsigned* tile)
{
    const int t = threadIdx.x, x = t & 7, y = t >> 3 & 7, z = t >> 6;
    const int b = (x + 1) + TFM_ATILE * (y + 1) + TFM_ATILE * TFM_ATILE * (z + 1);
    TfmCube q;
    unsigned wmin = 255u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const unsigned v = tile[b + (c & 1) + TFM_ATILE * (c >> 1 & 1) + TFM_ATILE * TFM_ATILE * (c >> 2)];
        q.sdf[c] = (int)(short)(v & 0xffffu);
        wmin = min(wmin, v >> 16);
    }
    q.valid = wmin > 0;
    return q;
}

// the lattice data of this thread's cube corners, out of LDS
template <bool NORMALS, bool COLOURS>
struct MeshAttrSrc {
    static constexpr bool normals = NORMALS, colours = COLOURS;
    const int* grad3;            // [3][TFM_TILE3]
    const unsigned* ctile;
    int b;                       // corner 0 at x + 9 y + 81 z
    __device__ __forceinline__ int at(unsigned c) const { return b + (int)(c & 1) + TFM_TILE * (int)(c >> 1 & 1) + TFM_TILE * TFM_TILE * (int)(c >> 2); }
    __device__ __forceinline__ void grad(unsigned c, int* g) const
    {
        const int i = at(c);
        g[0] = grad3[i]; g[1] = grad3[TFM_TILE3 + i]; g[2] = grad3[2 * TFM_TILE3 + i];
    }
    __device__ __forceinline__ unsigned colour(unsigned c) const { return ctile[at(c)]; }
};

static inline MeshScene mesh_scene(const tf_ctx* c)
{
    MeshScene s;
    s.v.hash = c->hash; s.v.vba = c->vba_guard; s.v.grid = c->bgrid;
    s.v.mask = (unsigned)c->p.n_buckets - 1u; s.v.n_buckets = c->p.n_buckets; s.n_total = c->n_total;
    return s;
}

static inline int mesh_groups(const tf_ctx* c) { return (c->n_total + TFM_WG - 1) / TFM_WG; }
