// tf_mesh_dev.h -- the workgroup skeleton of mesh extraction's kernels (tf_mesh.hip), each piece written
// once: the scene view, the live list of a 512-entry group, the workgroup scan, the block look-up, the
// LDS tiles of a hash entry's corner voxels with their gradient fill and cube read, the stores and the
// <NORMALS, COLOURS> dispatch.  Every piece that holds a barrier says so, and says what its caller may
// assume before and after.  The pieces that look at a block take the reading of the scene -- resident, or
// whole: both tiers of a swapping scene -- as the scene's type; the rule of what an entry holds across the tiers
// is tf_tier.h's (shared with the free views), the mesher's look-up and voxel read over it (mesh_block_resolve,
// mesh_voxel_whole) stand once, beside mesh_block_look.
#pragma once

#include <type_traits>

#include "tf_internal.h"
#include "tf_mesh.h"
#include "tf_tier.h"

#define TFM_WG 512               // threads per workgroup = voxels per block = entries per group
#define TFM_TILE 9
#define TFM_TILE3 (TFM_TILE * TFM_TILE * TFM_TILE)
#define TFM_GRID 2048            // workgroups of the count / emit passes (groups are taken round robin)
#define TFM_SCAN_GROUPS 4        // groups (of TFM_WG entries) per k_mesh_prefix workgroup

// The two readings of the scene (DESIGN.md §Mesh extraction, the whole map).  Every piece below that looks
// at a block takes the scene's type as a template parameter: MeshScene is the resident reading (blocks with
// ptr >= 0, as they lie in the VBA), MeshSceneWhole adds the GlobalCache (blocks resolved over both tiers).
struct MeshScene {
    static constexpr bool whole = false;
    SceneView v;                 // v.vba: the guard block of Voxel_s() (sdf 32767, w 0), then the VBA -- a missing block reads it
    int n_total;
};
struct MeshSceneWhole {
    static constexpr bool whole = true;
    SceneView v;
    int n_total;
    int maxW;                    // CombineVoxelInformation's clamp (tf_params::maxW)
    const unsigned char* state;  // HashSwapState::state per entry
    const unsigned char* flags;  // hasStoredData per entry
    const TfVoxel* store;        // storedVoxelBlocks: 512 voxels per entry
};

// The entries of group g that pred(idx) accepts, into live[] (any order); returns their number.  pred
// runs once per entry below n_total and may leave a side effect for a rejected one (the count passes
// write its 0).  Three barriers: the first ends the previous group's reads of live / nlive (and of
// whatever thread 0 reset just before the call), the third publishes the list.
template <class Pred>
__device__ __forceinline__ int mesh_live_list(int g, int n_total, int* live, int* nlive, Pred pred)
{
    const int t = threadIdx.x;
    __syncthreads();
    if (t == 0) *nlive = 0;
    __syncthreads();
    const int idx = g * TFM_WG + t;
    if (idx < n_total && pred(idx)) live[atomicAdd(nlive, 1)] = idx;
    __syncthreads();
    return *nlive;
}

// inclusive scan of one int per lane of the wave
__device__ __forceinline__ int mesh_wave_scan(int v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// Exclusive scan of `mine` over the workgroup's 512 threads: inclusive within the wave, then the lower
// waves' sums out of wsum[TFM_WG / 64].  One barrier, between wsum's writes and its reads: it also
// publishes whatever the caller wrote to LDS before the call.  No barrier behind the reads: the caller
// keeps one (the next entry's staging) between them and the next call.
__device__ __forceinline__ int mesh_scan(int mine, int* wsum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = mesh_wave_scan(mine);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int off = inc - mine;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    return off;
}

// (hash entry, VBA voxel offset) of a neighbour block, or (-1, TF_VOFF_NONE): a block coordinate
// outside the short range (blk_walk compares shorts and would wrap), a block the hash does not hold
// and a swapped-out entry (ptr -1) are all missing.  Both ends of the range are checked for every
// caller; the 9-wide tile only ever steps up from a short, so the lower compare cannot change its result.
__device__ __forceinline__ int2 mesh_block_look(const MeshScene& s, int bx, int by, int bz)
{
    if (tf_grid_in(bx, by, bz)) return s.v.grid[tf_grid_cell(bx, by, bz)];
    if (bx > 32767 || by > 32767 || bz > 32767 || bx < -32768 || by < -32768 || bz < -32768) return make_int2(-1, TF_VOFF_NONE);
    return blk_walk(s.v, bx, by, bz);
}

// ---- the whole reading's resolution (DESIGN.md §Mesh extraction, the whole map) ----
// The rule itself -- what an entry holds across the two tiers (tier_resolve_entry, tier_entry_resolves) and the
// walk over both (tier_walk) -- is tf_tier.h's, shared with the free views' whole reading.
// mesh_block_look for the whole reading: tf_tier.h's look-up (the grid, then the walk over both tiers -- inside the
// grid too), behind mesh_block_look's check of the short range for a block outside the grid
__device__ __forceinline__ TierBlk mesh_block_resolve(const MeshSceneWhole& s, int bx, int by, int bz)
{
    if (!tf_grid_in(bx, by, bz) && (bx > 32767 || by > 32767 || bz > 32767 || bx < -32768 || by < -32768 || bz < -32768)) {
        const TierBlk none = { TF_VOFF_NONE, TIER_STO_NONE, -1 };
        return none;
    }
    return tier_block_find(s, bx, by, bz);
}

// one voxel of a resolved block as the tiles hold it (sdf | w << 16): the active voxel (the guard's
// (32767, 0) where there is none), the stored one as it is, or CombineVoxelInformation of the two
__device__ __forceinline__ unsigned mesh_voxel_whole(const MeshSceneWhole& s, int act, int sto, int lin)
{
    unsigned a = reinterpret_cast<const unsigned*>(s.v.vba)[TF_BLK3 + act + lin] & 0xffffffu;
    if (sto >= 0) {                  // (per block: the lanes of a tile row share it but for the row's last voxel)
        const unsigned st = reinterpret_cast<const unsigned*>(s.store)[sto + lin] & 0xffffffu;
        a = act == TF_VOFF_NONE ? st : sw_combine(st, a, s.maxW);
    }
    return a;
}

struct MeshNoHook {
    __device__ __forceinline__ void operator()(int, int2) const {}
};

// Entry ei's 729 corner voxels into LDS (sdf | w << 16 per voxel, index x + 9 y + 81 z) and its eight
// blocks' voxel offsets into nvoff.  All threads of the workgroup call it; ei and e are uniform.
// Three barriers: the leading one ends the previous entry's reads of tile / nvoff and of any LDS of the
// caller's; between it and the second every thread calls hook(t, b) -- for t < 8, b is block t's
// (entry, voff) as found, so the caller can keep what belongs to the entry, and any thread may fill
// LDS of the caller's there; the trailing one publishes the tile, nvoff and what the hook wrote.
// The whole reading: nvoff holds TFM_NVOFF(Scene, 8) ints, the blocks' store offsets behind their active
// ones, each voxel comes from where its block's descriptor says, and the hook sees (entry, active offset) --
// the entry the block resolved at (the grid's on a hit, the walk's otherwise), -1 for a missing block; a block
// that lies in the GlobalCache alone has an entry and no active offset.
#define TFM_NVOFF(Scene, n) ((Scene::whole ? 2 : 1) * (n))
template <class Scene, class Hook = MeshNoHook>
__device__ __forceinline__ void mesh_stage(const Scene& s, int ei, const TfHashEntry& e, unsigned* tile, int* nvoff, Hook hook = Hook())
{
    const int t = threadIdx.x;
    __syncthreads();
    int2 b = make_int2(-1, TF_VOFF_NONE);
    if (t < 8) {
        if constexpr (Scene::whole) {
            const TierBlk d = t == 0 ? tier_resolve_entry(s, ei, e.ptr) : mesh_block_resolve(s, e.x + (t & 1), e.y + (t >> 1 & 1), e.z + (t >> 2));
            b = make_int2(d.ent, d.act);
            nvoff[8 + t] = d.sto;
        } else {
            b = t == 0 ? make_int2(ei, e.ptr * TF_BLK3) : mesh_block_look(s, e.x + (t & 1), e.y + (t >> 1 & 1), e.z + (t >> 2));
        }
        nvoff[t] = b.y;
    }
    hook(t, b);
    __syncthreads();
    for (int i = t; i < TFM_TILE3; i += TFM_WG) {
        const int z = i / (TFM_TILE * TFM_TILE), r = i - z * (TFM_TILE * TFM_TILE), y = r / TFM_TILE, x = r - y * TFM_TILE;
        const int bi = (x >> 3) | (y >> 3) << 1 | (z >> 3) << 2;
        const int voff = nvoff[bi];
        if constexpr (Scene::whole) {
            tile[i] = mesh_voxel_whole(s, voff, nvoff[8 + bi], (x & 7) + ((y & 7) << 3) + ((z & 7) << 6));
        } else {
            const TfVoxel v = s.v.vba[TF_BLK3 + voff + (x & 7) + ((y & 7) << 3) + ((z & 7) << 6)];
            tile[i] = (unsigned)(unsigned short)v.sdf | (unsigned)v.w << 16;
        }
    }
    __syncthreads();
}

// This thread's cube (voxel threadIdx.x = x + 8 y + 64 z) out of a tile STRIDE wide whose voxel (0, 0, 0)
// sits at ORIGIN on each axis: <TFM_TILE, 0> for mesh_stage's, <TFM_ATILE, 1> for mesh_stage_attr's.
template <int STRIDE, int ORIGIN>
__device__ __forceinline__ TfmCube mesh_cube(const unsigned* tile)
{
    const int t = threadIdx.x, x = t & 7, y = t >> 3 & 7, z = t >> 6;
    const int b = (x + ORIGIN) + STRIDE * (y + ORIGIN) + STRIDE * STRIDE * (z + ORIGIN);
    TfmCube q;
    unsigned wmin = 255u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const unsigned v = tile[b + (c & 1) + STRIDE * (c >> 1 & 1) + STRIDE * STRIDE * (c >> 2)];
        q.sdf[c] = (int)(short)(v & 0xffffu);
        wmin = min(wmin, v >> 16);
    }
    q.valid = wmin > 0;
    return q;
}

// ---- the attributed tile (k_mesh_emit_attr, k_mesh_emit_vertices) ----
#define TFM_ATILE 11
#define TFM_ATILE3 (TFM_ATILE * TFM_ATILE * TFM_ATILE)

// tile: sdf | w << 16 at (x + 1) + 11 (y + 1) + 121 (z + 1), x, y, z in -1 .. 9 (NORMALS; else 0 .. 8 only,
// the rim reads as w = 0); ctile: colour words at x + 9 y + 81 z (COLOURS); nvoff: the 27 block offsets
// (ox + 1) + 3 (oy + 1) + 9 (oz + 1), those with more than one -1 (without NORMALS: any -1) unused.
// Three barriers, as mesh_stage's: the leading one ends the previous entry's reads of tile / gradients /
// ctile / nvoff, the trailing one publishes the tiles.
// The whole reading (never with COLOURS: a swapping scene has no colour plane): ei is the entry's index,
// nvoff holds TFM_NVOFF(Scene, 27) ints, the store offsets behind the active ones, as mesh_stage's.
template <bool NORMALS, bool COLOURS, class Scene>
__device__ __forceinline__ void mesh_stage_attr(const Scene& s, const unsigned* __restrict__ rgb, int ei, const TfHashEntry& e, unsigned* tile,
                                                unsigned* ctile, int* nvoff)
{
    static_assert(!(Scene::whole && COLOURS), "the whole reading has no colours");
    const int t = threadIdx.x;
    __syncthreads();
    if (t < 27) {
        const int ox = t % 3 - 1, oy = t / 3 % 3 - 1, oz = t / 9 - 1;
        const int down = (ox < 0) + (oy < 0) + (oz < 0);
        int voff = TF_VOFF_NONE;
        if constexpr (Scene::whole) {
            TierBlk d = { TF_VOFF_NONE, TIER_STO_NONE, -1 };
            if (t == 13) d = tier_resolve_entry(s, ei, e.ptr);
            else if (down <= (NORMALS ? 1 : 0)) d = mesh_block_resolve(s, e.x + ox, e.y + oy, e.z + oz);
            voff = d.act;
            nvoff[27 + t] = d.sto;
        } else {
            if (t == 13) voff = e.ptr * TF_BLK3;
            else if (down <= (NORMALS ? 1 : 0)) voff = mesh_block_look(s, e.x + ox, e.y + oy, e.z + oz).y;
        }
        nvoff[t] = voff;
    }
    __syncthreads();
    for (int i = t; i < TFM_ATILE3; i += TFM_WG) {
        const int zi = i / (TFM_ATILE * TFM_ATILE), r = i - zi * (TFM_ATILE * TFM_ATILE), yi = r / TFM_ATILE, xi = r - yi * TFM_ATILE;
        const int x = xi - 1, y = yi - 1, z = zi - 1;
        const int rim = ((unsigned)x > 8u) + ((unsigned)y > 8u) + ((unsigned)z > 8u);
        unsigned packed = 0u;
        if (rim <= (NORMALS ? 1 : 0)) {
            const int bi = ((x >> 3) + 1) + 3 * ((y >> 3) + 1) + 9 * ((z >> 3) + 1);
            const int voff = nvoff[bi];
            if constexpr (Scene::whole) {
                packed = mesh_voxel_whole(s, voff, nvoff[27 + bi], (x & 7) + ((y & 7) << 3) + ((z & 7) << 6));
            } else {
                const int at = TF_BLK3 + voff + (x & 7) + ((y & 7) << 3) + ((z & 7) << 6);
                const TfVoxel v = s.v.vba[at];
                packed = (unsigned)(unsigned short)v.sdf | (unsigned)v.w << 16;
                if (COLOURS && rim == 0) ctile[x + TFM_TILE * y + TFM_TILE * TFM_TILE * z] = rgb[at];
            }
        }
        tile[i] = packed;
    }
    __syncthreads();
}

// The 9^3 lattice gradients of a complete 11-wide tile into grad3[3][TFM_TILE3], once per entry.  No
// barrier: the caller's next one (the scan's, or its own) publishes them.
__device__ __forceinline__ void mesh_grad_fill(const unsigned* tile, int* grad3)
{
    for (int i = threadIdx.x; i < TFM_TILE3; i += TFM_WG) {
        const int z = i / (TFM_TILE * TFM_TILE), r = i - z * (TFM_TILE * TFM_TILE), y = r / TFM_TILE, x = r - y * TFM_TILE;
        const int c = (x + 1) + TFM_ATILE * (y + 1) + TFM_ATILE * TFM_ATILE * (z + 1);
        const unsigned v0 = tile[c];
        grad3[i] = tfm_grad_axis_packed(tile[c - 1], v0, tile[c + 1]);
        grad3[TFM_TILE3 + i] = tfm_grad_axis_packed(tile[c - TFM_ATILE], v0, tile[c + TFM_ATILE]);
        grad3[2 * TFM_TILE3 + i] = tfm_grad_axis_packed(tile[c - TFM_ATILE * TFM_ATILE], v0, tile[c + TFM_ATILE * TFM_ATILE]);
    }
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

// ---- stores: dword-aligned vectors (a triangle is 36 bytes, a vertex 12) ----
typedef float tfm_f4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float tfm_f3 __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned tfm_u3 __attribute__((ext_vector_type(3), aligned(4)));

__device__ __forceinline__ void mesh_store9(float* p, const float* v)
{
    tfm_f4 a, b;
    a.x = v[0]; a.y = v[1]; a.z = v[2]; a.w = v[3];
    b.x = v[4]; b.y = v[5]; b.z = v[6]; b.w = v[7];
    *reinterpret_cast<tfm_f4*>(p) = a;
    *reinterpret_cast<tfm_f4*>(p + 4) = b;
    p[8] = v[8];
}

__device__ __forceinline__ void mesh_store3(float* p, const float* v)
{
    tfm_f3 a;
    a.x = v[0]; a.y = v[1]; a.z = v[2];
    *reinterpret_cast<tfm_f3*>(p) = a;
}

// ---- the host side ----
static inline MeshScene mesh_scene(const tf_ctx* c)
{
    MeshScene s;
    s.v.hash = c->hash; s.v.vba = c->vba_guard; s.v.grid = c->bgrid;
    s.v.mask = (unsigned)c->p.n_buckets - 1u; s.v.n_buckets = c->p.n_buckets; s.n_total = c->n_total;
    return s;
}

// ... of a swapping context (the others have no GlobalCache: their whole reading is the resident one)
static inline MeshSceneWhole mesh_scene_whole(const tf_ctx* c)
{
    MeshSceneWhole s;
    s.v = mesh_scene(c).v;
    s.n_total = c->n_total; s.maxW = c->p.maxW;
    s.state = c->swapState; s.flags = c->swapFlags; s.store = c->swapStore;
    return s;
}

static inline int mesh_groups(const tf_ctx* c) { return (c->n_total + TFM_WG - 1) / TFM_WG; }
static inline dim3 mesh_grid(const tf_ctx* c) { return dim3(mesh_groups(c) < TFM_GRID ? mesh_groups(c) : TFM_GRID); }

// f(std::bool_constant<NORMALS>, std::bool_constant<COLOURS>) for the run-time pair
template <class F>
static inline void mesh_dispatch_attr(bool normals, bool colours, F f)
{
    if (normals && colours) f(std::true_type(), std::true_type());
    else if (normals) f(std::true_type(), std::false_type());
    else if (colours) f(std::false_type(), std::true_type());
    else f(std::false_type(), std::false_type());
}
