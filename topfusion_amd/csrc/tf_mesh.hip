// tf_mesh.hip -- mesh extraction from the voxel block hash for gfx950 (an addition: the reference has no
// mesher).  Marching tetrahedra on the Kuhn split of every voxel cube (tf_mesh.h, DESIGN.md §Mesh
// extraction), as plain launches on the context stream.  The kernels are assembled from the pieces of
// tf_mesh_dev.h (live list, staging, cube read, scan, gradient fill, stores) and differ in what they do
// with an entry's cubes.
//
// The triangle soup:
//   k_mesh_count  : per live hash entry (ptr >= 0) the 9 x 9 x 9 corner voxels of its 512 cubes staged in
//                   LDS (own block + up to seven neighbours, found through the block grid, outside it by
//                   the hash walk), every cube classified, the entry's triangle count (64-bit) written;
//                   dead entries get 0; each 512-entry group's total written beside
//   k_mesh_prefix : exclusive scan of the counts in entry order -> every entry's base, and the total
//   k_mesh_emit   : the classification again, an exclusive scan over the 512 voxels inside the
//                   workgroup, triangles written at base + offset while below the caller's capacity
//   k_mesh_emit_attr<NORMALS, COLOURS> : k_mesh_emit with per-vertex normals (TSDF gradient) and / or colours
//                   (colour plane) beside the positions, from the larger tile (mesh_stage_attr)
// k_mesh_count, k_mesh_emit and k_mesh_emit_attr<true, false> exist in two readings of the scene, chosen by the
// scene type they are instantiated with (tf_mesh_dev.h): MeshScene, the resident blocks as above, and
// MeshSceneWhole (TF_MESH_WHOLE, tf_mesh_extract_whole), where an entry is live when it holds voxel data in
// either tier and every block -- own, cube neighbour, gradient neighbour -- is resolved over the VBA and the
// GlobalCache: active, stored, or CombineVoxelInformation of both where a merge is pending.  Counts and bases
// are per hash entry in both, so the scratch and k_mesh_prefix are shared.
//
// The indexed form (shared vertices, u32 indices; DESIGN.md §Mesh extraction, indexed).  A vertex is its
// Kuhn edge (tf_mesh.h): per VBA block a mask of 512 x 7 edge bits (TFM_EDGE_WORDS words, indexed by the
// block number ptr) and the words' exclusive popcount prefixes; per hash entry its vertex count and
// base, by k_mesh_prefix on a second pair of arrays.
//   k_mesh_mark          : k_mesh_count's loop; every valid cube ORs its sign-changing Kuhn edges into the
//                          owners' masks -- gathered in LDS, flushed with one global atomicOr per non-zero
//                          word (integer OR: the result does not depend on the order of arrival)
//   k_mesh_vcount        : one wave per live entry: the 112 words' popcounts, scanned -> prefixes, count
//   k_mesh_emit_vertices : per live entry with vertices, each thread its voxel's seven edges; a set bit is
//                          the vertex base + prefix + popcount below
//   k_mesh_emit_indices  : k_mesh_emit's structure; a triangle vertex (lo, hi) -> owner block, bit, index
//
// The indexed form's four kernels exist in both readings too, and differ in one thing: the row of a block's edge
// words.  The resident one keys them by VBA block (MeshKeyBlock); a stored block has none, so the whole one
// (tf_mesh_extract_indexed_whole) keys them by slot, the entry's rank among the entries that resolve
// (MeshKeySlot; k_mesh_slot_count + k_mesh_slot_assign number them per extraction), in a scratch of its own.
//
// No workgroup waits on another inside a grid.  The scene (hash, VBA, block grid) and the GlobalCache are only read.
#include "tf_mesh_dev.h"
#include "tf_host.h"

#include <stdlib.h>

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the live-list predicates: entries with a block (a dead one gets its count of 0 here, where `count` is
// given), and entries with output below the capacity (count and base are uniform per entry)
struct MeshHasBlock {
    const TfHashEntry* hash;
    long long* count;            // may be nullptr
    __device__ __forceinline__ bool operator()(int idx) const
    {
        if (hash[idx].ptr >= 0) return true;
        if (count) count[idx] = 0;
        return false;
    }
};
// ... the whole reading's: entries whose block resolves in either tier (tier_entry_resolves)
struct MeshHasData {
    MeshSceneWhole s;
    long long* count;
    __device__ __forceinline__ bool operator()(int idx) const
    {
        if (tier_entry_resolves(s, idx)) return true;
        if (count) count[idx] = 0;
        return false;
    }
};
__device__ __forceinline__ MeshHasBlock mesh_has_block(const MeshScene& s, long long* count) { return MeshHasBlock{ s.v.hash, count }; }
__device__ __forceinline__ MeshHasData mesh_has_block(const MeshSceneWhole& s, long long* count) { return MeshHasData{ s, count }; }
struct MeshHasOutput {
    const long long* count;
    const long long* base;
    long long capacity;
    __device__ __forceinline__ bool operator()(int idx) const { return count[idx] > 0 && base[idx] < capacity; }
};

template <class Scene>
__global__ __launch_bounds__(TFM_WG) void k_mesh_count(Scene s, long long* __restrict__ count, long long* __restrict__ groupTot)
{
    __shared__ unsigned tile[TFM_TILE3];
    __shared__ int nvoff[TFM_NVOFF(Scene, 8)];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ int wsum[TFM_WG / 64];
    const int t = threadIdx.x;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int n = mesh_live_list(g, s.n_total, live, &nlive, mesh_has_block(s, count));      // (any order: each entry's count stands alone)
        long long tot = 0;
        for (int k = 0; k < n; ++k) {
            const int ei = live[k];
            mesh_stage(s, ei, s.v.hash[ei], tile, nvoff);
            const int c = wave_sum(tfm_cube_count(mesh_cube<TFM_TILE, 0>(tile)));
            if ((t & 63) == 0) wsum[t >> 6] = c;
            __syncthreads();
            if (t == 0) {
                int sum = 0;
                for (int w = 0; w < TFM_WG / 64; ++w) sum += wsum[w];
                count[ei] = sum;
                tot += sum;
            }
        }
        if (t == 0) groupTot[g] = tot;
    }
}

// Exclusive scan of count[0 .. n_total) into base, base[n_total] = the total.  Workgroup w owns
// TFM_SCAN_GROUPS groups: its start is the sum of the lower groups' totals (read, not waited for: they
// were written by the launch before), then a scan of its own TFM_SCAN_GROUPS * TFM_WG counts.
__global__ __launch_bounds__(256) void k_mesh_prefix(const long long* __restrict__ count, const long long* __restrict__ groupTot,
                                                     long long* __restrict__ base, int n_total)
{
    __shared__ long long red[256];
    __shared__ long long carry;
    const int t = threadIdx.x;
    const int ngroups = (n_total + TFM_WG - 1) / TFM_WG;
    const int g0 = blockIdx.x * TFM_SCAN_GROUPS;
    long long s = 0;
    for (int g = t; g < g0 && g < ngroups; g += 256) s += groupTot[g];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) carry = red[0];
    __syncthreads();
    const int first = g0 * TFM_WG, last = min(first + TFM_SCAN_GROUPS * TFM_WG, n_total);
    for (int i0 = first; i0 < last; i0 += 256) {
        const int i = i0 + t;
        const long long v = i < last ? count[i] : 0;
        __syncthreads();
        red[t] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {                 // Hillis-Steele inclusive scan
            const long long a = t >= o ? red[t - o] : 0;
            __syncthreads();
            red[t] += a;
            __syncthreads();
        }
        const long long c = carry;
        if (i < last) base[i] = c + red[t] - v;
        __syncthreads();
        if (t == 255) carry = c + red[255];
        __syncthreads();
    }
    if (last == n_total && t == 0) base[n_total] = carry;
}

// a triangle's positions (tri may be nullptr, uniform), normals and colours, clipped at the capacity
template <bool NORMALS, bool COLOURS>
struct MeshAttrWriter {
    float* tri;
    float* nrm;
    unsigned* col;
    long long idx;               // the next triangle's index
    long long capacity;
    __device__ __forceinline__ void operator()(const float* t9, const float* n9, const unsigned* rgba)
    {
        if (idx < capacity) {
            if (tri) mesh_store9(tri + idx * 9, t9);
            if (NORMALS) mesh_store9(nrm + idx * 9, n9);
            if (COLOURS) {
                tfm_u3 c;
                c.x = rgba[0]; c.y = rgba[1]; c.z = rgba[2];
                *reinterpret_cast<tfm_u3*>(col + idx * 3) = c;
            }
        }
        ++idx;
    }
};

template <class Scene>
__global__ __launch_bounds__(TFM_WG) void k_mesh_emit(Scene s, const long long* __restrict__ count, const long long* __restrict__ base,
                                                      float* __restrict__ out, long long capacity, float voxelSize)
{
    __shared__ unsigned tile[TFM_TILE3];
    __shared__ int nvoff[TFM_NVOFF(Scene, 8)];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ int wsum[TFM_WG / 64];
    const int t = threadIdx.x;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int n = mesh_live_list(g, s.n_total, live, &nlive, MeshHasOutput{ count, base, capacity });
        for (int k = 0; k < n; ++k) {
            const int ei = live[k];
            const TfHashEntry e = s.v.hash[ei];
            mesh_stage(s, ei, e, tile, nvoff);
            const TfmCube q = mesh_cube<TFM_TILE, 0>(tile);
            const int mine = tfm_cube_count(q);
            const int off = mesh_scan(mine, wsum);
            if (mine) {
                MeshAttrWriter<false, false> wr = { out, nullptr, nullptr, base[ei] + off, capacity };
                tfm_cube_emit_attr(q, e.x * TF_BLK + (t & 7), e.y * TF_BLK + (t >> 3 & 7), e.z * TF_BLK + (t >> 6), voxelSize, TfmNoAttr(), wr);
            }
        }
    }
}

// The emit pass with per-vertex attributes: per entry the 11 x 11 x 11 voxels around the block (local
// coordinates -1 .. 9; only points with at most one coordinate outside 0 .. 8 are read) from the block and
// up to 19 neighbours, the 9 x 9 x 9 integer gradients formed once from it, the colour words of the same
// 9 x 9 x 9 corners; then k_mesh_emit's classification and scan, and per triangle vertex two LDS gradient /
// colour reads per end.
template <bool NORMALS, bool COLOURS, class Scene>
__global__ __launch_bounds__(TFM_WG) void k_mesh_emit_attr(Scene s, const unsigned* __restrict__ rgb, const long long* __restrict__ count,
                                                           const long long* __restrict__ base, float* __restrict__ outTri,
                                                           float* __restrict__ outNrm, unsigned* __restrict__ outCol, long long capacity,
                                                           float voxelSize)
{
    __shared__ unsigned tile[TFM_ATILE3];
    __shared__ int grad3[NORMALS ? 3 * TFM_TILE3 : 1];
    __shared__ unsigned ctile[COLOURS ? TFM_TILE3 : 1];
    __shared__ int nvoff[TFM_NVOFF(Scene, 27)];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ int wsum[TFM_WG / 64];
    const int t = threadIdx.x;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int n = mesh_live_list(g, s.n_total, live, &nlive, MeshHasOutput{ count, base, capacity });
        for (int k = 0; k < n; ++k) {
            const int ei = live[k];
            const TfHashEntry e = s.v.hash[ei];
            mesh_stage_attr<NORMALS, COLOURS>(s, rgb, ei, e, tile, ctile, nvoff);
            if (NORMALS) mesh_grad_fill(tile, grad3);
            const TfmCube q = mesh_cube<TFM_ATILE, 1>(tile);
            const int mine = tfm_cube_count(q);
            const int off = mesh_scan(mine, wsum);       // (its barrier also publishes the gradients)
            if (mine) {
                const MeshAttrSrc<NORMALS, COLOURS> src = { grad3, ctile, (t & 7) + TFM_TILE * (t >> 3 & 7) + TFM_TILE * TFM_TILE * (t >> 6) };
                MeshAttrWriter<NORMALS, COLOURS> wr = { outTri, outNrm, outCol, base[ei] + off, capacity };
                tfm_cube_emit_attr(q, e.x * TF_BLK + (t & 7), e.y * TF_BLK + (t >> 3 & 7), e.z * TF_BLK + (t >> 6), voxelSize, src, wr);
            }
        }
    }
}

// ---- the indexed form -------------------------------------------------------------------------------------
// Where a block's TFM_EDGE_WORDS edge words lie in the mask and prefix arrays -- the one thing the two readings'
// indexed kernels differ in.  key(b), b = (hash entry, VBA voxel offset) of a block as mesh_stage's hook sees it,
// is the block's row there, or -1 for a block that owns nothing (missing, or outside the scratch).
// Resident: the VBA block number.  Whole: the entry's slot, its rank among the entries that resolve
// (k_mesh_slot_count / k_mesh_slot_assign below), so the scratch is as large as the map and no larger.
struct MeshKeyBlock {
    int n_blocks;
    __device__ __forceinline__ int operator()(int2 b) const { return b.y >= 0 && (b.y >> 9) < n_blocks ? b.y >> 9 : -1; }
};
struct MeshKeySlot {
    const int* slot;             // [n_total]
    __device__ __forceinline__ int operator()(int2 b) const { return b.x >= 0 ? slot[b.x] : -1; }
};

// The slot numbering: slot[ei] = the number of resolving entries below ei where ei resolves, else -1; the
// total behind the group counts.  An exclusive scan of a 0 / 1 predicate in 32 bits, in two launches (no
// workgroup waits on another): each 512-entry group's count, then per group the sum of the lower groups'
// counts (read, written by the launch before) plus the rank inside the group by wave ballots.
__global__ __launch_bounds__(TFM_WG) void k_mesh_slot_count(MeshSceneWhole s, int* __restrict__ gcount)
{
    __shared__ int wsum[TFM_WG / 64];
    const int t = threadIdx.x;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int idx = g * TFM_WG + t;
        const bool r = idx < s.n_total && tier_entry_resolves(s, idx);
        const int c = __popcll(__ballot(r));
        __syncthreads();             // the previous group's reads of wsum
        if ((t & 63) == 0) wsum[t >> 6] = c;
        __syncthreads();
        if (t == 0) {
            int sum = 0;
            for (int w = 0; w < TFM_WG / 64; ++w) sum += wsum[w];
            gcount[g] = sum;
        }
    }
}

__global__ __launch_bounds__(TFM_WG) void k_mesh_slot_assign(MeshSceneWhole s, const int* __restrict__ gcount, int* __restrict__ slot,
                                                             int* __restrict__ total)
{
    __shared__ int wsum[TFM_WG / 64];
    __shared__ int red[TFM_WG / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        int below = 0;
        for (int i = t; i < g; i += TFM_WG) below += gcount[i];
        below = wave_sum(below);
        const int idx = g * TFM_WG + t;
        const bool r = idx < s.n_total && tier_entry_resolves(s, idx);
        const unsigned long long bal = __ballot(r);
        __syncthreads();             // the previous group's reads of wsum / red
        if (lane == 0) { wsum[wave] = __popcll(bal); red[wave] = below; }
        __syncthreads();
        int base = 0, mine = 0;
        for (int w = 0; w < TFM_WG / 64; ++w) { base += red[w]; mine += w < wave ? wsum[w] : 0; }
        if (idx < s.n_total) slot[idx] = r ? base + mine + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
        if (g == ngroups - 1 && t == 0) {
            int sum = base;
            for (int w = 0; w < TFM_WG / 64; ++w) sum += wsum[w];
            *total = sum;
        }
    }
}

struct MeshMarker {
    unsigned* lmask;             // LDS, [8][TFM_EDGE_WORDS]
    __device__ __forceinline__ void operator()(const TfmEdgeRef& r) { atomicOr(&lmask[r.owner * TFM_EDGE_WORDS + (r.bit >> 5)], 1u << (r.bit & 31u)); }
};

// mesh_stage's hook of the mark pass: the eight blocks' rows in the mask
template <class Key>
struct MeshKeyStage {
    Key key;
    int* nkey;                   // LDS, [8]
    __device__ __forceinline__ void operator()(int t, int2 b) const
    {
        if (t < 8) nkey[t] = key(b);
    }
};

template <class Scene, class Key>
__global__ __launch_bounds__(TFM_WG) void k_mesh_mark(Scene s, Key key, unsigned* __restrict__ mask)
{
    __shared__ unsigned tile[TFM_TILE3];
    __shared__ int nvoff[TFM_NVOFF(Scene, 8)];
    __shared__ int nkey[8];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ unsigned lmask[8 * TFM_EDGE_WORDS];
    const int t = threadIdx.x;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int n = mesh_live_list(g, s.n_total, live, &nlive, mesh_has_block(s, nullptr));    // (any order: OR commutes)
        for (int k = 0; k < n; ++k) {
            const int ei = live[k];
            mesh_stage(s, ei, s.v.hash[ei], tile, nvoff, MeshKeyStage<Key>{ key, nkey });        // (its leading barrier: the previous entry's flush is done)
            for (int i = t; i < 8 * TFM_EDGE_WORDS; i += TFM_WG) lmask[i] = 0u;
            __syncthreads();
            MeshMarker mk = { lmask };
            tfm_cube_mark(mesh_cube<TFM_TILE, 0>(tile), t & 7, t >> 3 & 7, t >> 6, mk);
            __syncthreads();
            for (int i = t; i < 8 * TFM_EDGE_WORDS; i += TFM_WG) {
                const unsigned w = lmask[i];
                if (w) {
                    // the owner holds a corner of a valid cube (w > 0), so its block exists; the guard only bounds the store
                    const int o = i / TFM_EDGE_WORDS, row = nkey[o];
                    if (row >= 0) atomicOr(&mask[(size_t)row * TFM_EDGE_WORDS + (i - o * TFM_EDGE_WORDS)], w);
                }
            }
        }
    }
}

// Per live entry (one wave each) the exclusive popcount prefix of its block's mask words and its vertex
// count; dead entries count 0; each 512-entry group's total beside, as k_mesh_count leaves them.
template <class Scene, class Key>
__global__ __launch_bounds__(TFM_WG) void k_mesh_vcount(Scene s, Key key, const unsigned* __restrict__ mask, unsigned* __restrict__ wpre,
                                                        long long* __restrict__ count, long long* __restrict__ groupTot)
{
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ int gsum;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        if (t == 0) gsum = 0;            // (thread 0 read the previous group's sum itself; the list's barriers stand before the adds)
        const int n = mesh_live_list(g, s.n_total, live, &nlive, mesh_has_block(s, count));
        for (int k = wave; k < n; k += TFM_WG / 64) {
            const int ei = live[k];
            const int row = key(make_int2(ei, s.v.hash[ei].ptr * TF_BLK3));
            int total = 0;
            if (row >= 0) {
                const size_t at = (size_t)row * TFM_EDGE_WORDS;
                const int ca = __popc(mask[at + lane]);
                const int cb = lane < TFM_EDGE_WORDS - 64 ? __popc(mask[at + 64 + lane]) : 0;
                const int ia = mesh_wave_scan(ca), ib = mesh_wave_scan(cb);
                const int ta = __shfl(ia, 63, 64);
                total = ta + __shfl(ib, 63, 64);
                wpre[at + lane] = (unsigned)(ia - ca);
                if (lane < TFM_EDGE_WORDS - 64) wpre[at + 64 + lane] = (unsigned)(ta + ib - cb);
            }
            if (lane == 0) {
                count[ei] = total;
                atomicAdd(&gsum, total);             // (an integer sum: any order)
            }
        }
        __syncthreads();
        if (t == 0) groupTot[g] = gsum;
    }
}

// The vertex table: positions (may be nullptr), normals, colours (one RGBA word per vertex), each clipped
// at `capacity` vertices.  The tile is the attributed kernel's; a block's vertices are contiguous.
template <bool NORMALS, bool COLOURS, class Scene, class Key>
__global__ __launch_bounds__(TFM_WG) void k_mesh_emit_vertices(Scene s, Key key, const unsigned* __restrict__ rgb, const unsigned* __restrict__ mask,
                                                               const unsigned* __restrict__ wpre, const long long* __restrict__ vcount,
                                                               const long long* __restrict__ vbase, float* __restrict__ outPos,
                                                               float* __restrict__ outNrm, unsigned* __restrict__ outCol, long long capacity,
                                                               float voxelSize)
{
    __shared__ unsigned tile[TFM_ATILE3];
    __shared__ int grad3[NORMALS ? 3 * TFM_TILE3 : 1];
    __shared__ unsigned ctile[COLOURS ? TFM_TILE3 : 1];
    __shared__ int nvoff[TFM_NVOFF(Scene, 27)];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ unsigned lm[TFM_EDGE_WORDS + 1], lpre[TFM_EDGE_WORDS];
    const int t = threadIdx.x;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    if (t == 0) lm[TFM_EDGE_WORDS] = 0u;     // (the zero word behind the mask; published by the first list's barriers)
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int n = mesh_live_list(g, s.n_total, live, &nlive, MeshHasOutput{ vcount, vbase, capacity });
        for (int k = 0; k < n; ++k) {
            const int ei = live[k];
            const TfHashEntry e = s.v.hash[ei];
            mesh_stage_attr<NORMALS, COLOURS>(s, rgb, ei, e, tile, ctile, nvoff);
            if (t < TFM_EDGE_WORDS) {                // (vcount > 0: the entry is live and has a row, k_mesh_vcount)
                const size_t own = (size_t)key(make_int2(ei, e.ptr * TF_BLK3)) * TFM_EDGE_WORDS;
                lm[t] = mask[own + t];
                lpre[t] = wpre[own + t];
            }
            if (NORMALS) mesh_grad_fill(tile, grad3);
            __syncthreads();         // the mask words, and the gradients
            // this voxel's seven bits, t * 7 .. t * 7 + 6: in one word or across two (lm has a zero word behind)
            const unsigned b0 = (unsigned)t * 7u, w0 = b0 >> 5;
            const unsigned bits = (unsigned)((((unsigned long long)lm[w0 + 1] << 32 | lm[w0]) >> (b0 & 31u)) & 127u);
            if (bits) {
                const int x = t & 7, y = t >> 3 & 7, z = t >> 6;
                const int c = (x + 1) + TFM_ATILE * (y + 1) + TFM_ATILE * TFM_ATILE * (z + 1);
                const int sp = (int)(short)(tile[c] & 0xffffu);
                const MeshAttrSrc<NORMALS, COLOURS> src = { grad3, ctile, x + TFM_TILE * y + TFM_TILE * TFM_TILE * z };
                const long long base = vbase[ei];
#pragma unroll
                for (unsigned dc = 1; dc < 8; ++dc) {
                    if (!(bits >> (dc - 1) & 1u)) continue;
                    const unsigned bit = b0 + dc - 1;
                    const long long vi = base + tfm_edge_rank(lm[bit >> 5], lpre[bit >> 5], bit);
                    if (vi >= capacity) continue;
                    const int sq = (int)(short)(tile[c + (int)(dc & 1) + TFM_ATILE * (int)(dc >> 1 & 1) + TFM_ATILE * TFM_ATILE * (int)(dc >> 2)] & 0xffffu);
                    if (outPos) {
                        float p[3];
                        tfm_edge_vertex(dc, sp, sq, e.x * TF_BLK + x, e.y * TF_BLK + y, e.z * TF_BLK + z, voxelSize, p);
                        mesh_store3(outPos + vi * 3, p);
                    }
                    const float et = tfm_edge_t(sp, sq);
                    if (NORMALS) {
                        int gp[3], gq[3];
                        float nr[3];
                        src.grad(0u, gp);
                        src.grad(dc, gq);
                        tfm_normal(et, gp, gq, nr);
                        mesh_store3(outNrm + vi * 3, nr);
                    }
                    if (COLOURS) outCol[vi] = tfm_colour(et, src.colour(0u), src.colour(dc));
                }
            }
        }
    }
}

// the index of one triangle vertex: its edge's owner among the entry's eight blocks, the bit, the rank
struct MeshIndexWriter {
    const unsigned* lm;          // LDS: the entry's own mask words and prefixes
    const unsigned* lpre;
    const int* nkey;             // LDS: the eight blocks' rows in the mask
    const long long* nbase;      // LDS: ... and their entries' vertex bases
    const unsigned* mask;
    const unsigned* wpre;
    unsigned* out;
    int x, y, z;
    long long idx;               // the next triangle's index
    long long capacity;
    __device__ __forceinline__ void operator()(const unsigned* lo, const unsigned* hi)
    {
        if (idx < capacity) {
            tfm_u3 tri;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const TfmEdgeRef r = tfm_edge_ref(x + (int)(lo[v] & 1), y + (int)(lo[v] >> 1 & 1), z + (int)(lo[v] >> 2), hi[v] & ~lo[v]);
                const unsigned w = r.bit >> 5;
                unsigned m = 0u, pre = 0u;
                if (r.owner == 0u) {
                    m = lm[w]; pre = lpre[w];
                } else if (nkey[r.owner] >= 0) {         // (always: the owner holds a corner of this valid cube)
                    const size_t at = (size_t)nkey[r.owner] * TFM_EDGE_WORDS + w;
                    m = mask[at]; pre = wpre[at];
                }
                tri[v] = (unsigned)(nbase[r.owner] + tfm_edge_rank(m, pre, r.bit));
            }
            *reinterpret_cast<tfm_u3*>(out + idx * 3) = tri;
        }
        ++idx;
    }
};

// mesh_stage's hook of k_mesh_emit_indices: the eight blocks' rows in the mask and their entries' vertex
// bases (a missing block owns nothing), and threads 64 .. 175 bring the entry's own mask words and prefixes
template <class Key>
struct MeshIndexStage {
    Key key;
    const long long* vbase;
    const unsigned* mask;        // the entry's block's words
    const unsigned* wpre;
    int* nkey;                   // LDS
    long long* nbase;
    unsigned* lm;
    unsigned* lpre;
    __device__ __forceinline__ void operator()(int t, int2 b) const
    {
        if (t < 8) {
            const int row = key(b);
            nkey[t] = row;
            nbase[t] = row >= 0 ? vbase[b.x] : 0;
        }
        if (t >= 64 && t < 64 + TFM_EDGE_WORDS) {
            lm[t - 64] = mask[t - 64];
            lpre[t - 64] = wpre[t - 64];
        }
    }
};

template <class Scene, class Key>
__global__ __launch_bounds__(TFM_WG) void k_mesh_emit_indices(Scene s, Key key, const unsigned* __restrict__ mask, const unsigned* __restrict__ wpre,
                                                              const long long* __restrict__ count, const long long* __restrict__ base,
                                                              const long long* __restrict__ vbase, unsigned* __restrict__ out, long long capacity)
{
    __shared__ unsigned tile[TFM_TILE3];
    __shared__ int nvoff[TFM_NVOFF(Scene, 8)];
    __shared__ int nkey[8];
    __shared__ long long nbase[8];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ int wsum[TFM_WG / 64];
    __shared__ unsigned lm[TFM_EDGE_WORDS], lpre[TFM_EDGE_WORDS];
    const int t = threadIdx.x;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int n = mesh_live_list(g, s.n_total, live, &nlive, MeshHasOutput{ count, base, capacity });
        for (int k = 0; k < n; ++k) {
            const int ei = live[k];
            const TfHashEntry e = s.v.hash[ei];
            // (count > 0: a valid cube of the entry's own, so it is live and has a row unless its block lies outside the scratch)
            const int row = key(make_int2(ei, e.ptr * TF_BLK3));
            const size_t own = (size_t)(row < 0 ? 0 : row) * TFM_EDGE_WORDS;
            mesh_stage(s, ei, e, tile, nvoff, MeshIndexStage<Key>{ key, vbase, mask + own, wpre + own, nkey, nbase, lm, lpre });
            const TfmCube q = mesh_cube<TFM_TILE, 0>(tile);
            const int mine = tfm_cube_count(q);
            const int off = mesh_scan(mine, wsum);
            if (mine) {
                MeshIndexWriter wr = { lm, lpre, nkey, nbase, mask, wpre, out, t & 7, t >> 3 & 7, t >> 6, base[ei] + off, capacity };
                tfm_cube_emit_edges(q, wr);
            }
        }
    }
}

// ---- the host side ----------------------------------------------------------------------------------------
static hipError_t mesh_prefix(tf_ctx* c, const long long* count, const long long* groupTot, long long* base)
{
    hipLaunchKernelGGL(k_mesh_prefix, dim3((mesh_groups(c) + TFM_SCAN_GROUPS - 1) / TFM_SCAN_GROUPS), dim3(256), 0, c->stream, count, groupTot,
                       base, c->n_total);
    return hipGetLastError();
}

// Does this extraction read the GlobalCache?  Only a swapping context has one: on any other, every entry is in
// the first or the last row of the resolution table and the whole reading IS the resident one (the same kernels).
static inline bool mesh_reads_store(const tf_ctx* c, bool whole) { return whole && c->p.use_swapping && c->swapStore; }

// count + prefix; the scratch (counts, bases + total, group totals behind the counts) is the
// context's from the first call on.  whole: the reading over both tiers (here and in the emit passes).
static hipError_t tfk_mesh_count(tf_ctx* c, bool whole = false)
{
    if (!c->meshCount) {
        const hipError_t e = tf_mem_hip(c->mem.alloc_group({
            TfCtxMem::dev(&c->meshCount, sizeof(long long) * ((size_t)c->n_total + (size_t)mesh_groups(c))),
            TfCtxMem::dev(&c->meshBase, sizeof(long long) * ((size_t)c->n_total + 1)) }));
        if (e != hipSuccess) return e;
    }
    long long* groupTot = c->meshCount + c->n_total;
    if (mesh_reads_store(c, whole))
        hipLaunchKernelGGL(k_mesh_count<MeshSceneWhole>, mesh_grid(c), dim3(TFM_WG), 0, c->stream, mesh_scene_whole(c), c->meshCount, groupTot);
    else
        hipLaunchKernelGGL(k_mesh_count<MeshScene>, mesh_grid(c), dim3(TFM_WG), 0, c->stream, mesh_scene(c), c->meshCount, groupTot);
    return mesh_prefix(c, c->meshCount, groupTot, c->meshBase);
}

// after tfk_mesh_count on the same stream
static hipError_t tfk_mesh_emit(tf_ctx* c, float* triangles, long long capacity, bool whole = false)
{
    if (mesh_reads_store(c, whole))
        hipLaunchKernelGGL(k_mesh_emit<MeshSceneWhole>, mesh_grid(c), dim3(TFM_WG), 0, c->stream, mesh_scene_whole(c), c->meshCount, c->meshBase,
                           triangles, capacity, c->p.voxelSize);
    else
        hipLaunchKernelGGL(k_mesh_emit<MeshScene>, mesh_grid(c), dim3(TFM_WG), 0, c->stream, mesh_scene(c), c->meshCount, c->meshBase, triangles,
                           capacity, c->p.voxelSize);
    return hipGetLastError();
}

// after tfk_mesh_count on the same stream: positions (may be nullptr), normals and / or colours (at
// least one of the two; colours need the colour plane), all clipped at the same capacity.  whole: normals
// only (a swapping scene has no colour plane; the callers refuse the pair).
static hipError_t tfk_mesh_emit_attr(tf_ctx* c, float* triangles, float* normals, unsigned char* colours, long long capacity, bool whole = false)
{
    if (mesh_reads_store(c, whole)) {
        hipLaunchKernelGGL((k_mesh_emit_attr<true, false, MeshSceneWhole>), mesh_grid(c), dim3(TFM_WG), 0, c->stream, mesh_scene_whole(c), nullptr,
                           c->meshCount, c->meshBase, triangles, normals, nullptr, capacity, c->p.voxelSize);
        return hipGetLastError();
    }
    mesh_dispatch_attr(normals != nullptr, colours != nullptr, [&](auto N, auto C) {
        if constexpr (N() || C())
            hipLaunchKernelGGL((k_mesh_emit_attr<N(), C(), MeshScene>), mesh_grid(c), dim3(TFM_WG), 0, c->stream, mesh_scene(c), c->vba_rgb_guard, c->meshCount,
                               c->meshBase, triangles, normals, reinterpret_cast<unsigned*>(colours), capacity, c->p.voxelSize);
    });
    return hipGetLastError();
}

// The vertex counts and bases per hash entry (both readings'), the context's from the first indexed call on
static hipError_t mesh_vcount_scratch(tf_ctx* c)
{
    if (c->meshVCount) return hipSuccess;
    const size_t counts = sizeof(long long) * ((size_t)c->n_total + (size_t)mesh_groups(c));
    return tf_mem_hip(c->mem.alloc_group({ TfCtxMem::dev(&c->meshVCount, counts),
                                           TfCtxMem::dev(&c->meshVBase, sizeof(long long) * ((size_t)c->n_total + 1)) }));
}

// mark, count and the vertex prefix over masks already cleared
template <class Scene, class Key>
static hipError_t mesh_mark_count(tf_ctx* c, const Scene& s, Key key, unsigned* mask, unsigned* wpre)
{
    long long* groupTot = c->meshVCount + c->n_total;
    hipLaunchKernelGGL((k_mesh_mark<Scene, Key>), mesh_grid(c), dim3(TFM_WG), 0, c->stream, s, key, mask);
    hipLaunchKernelGGL((k_mesh_vcount<Scene, Key>), mesh_grid(c), dim3(TFM_WG), 0, c->stream, s, key, mask, wpre, c->meshVCount, groupTot);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? mesh_prefix(c, c->meshVCount, groupTot, c->meshVBase) : e;
}

// Triangle count + prefix (tfk_mesh_count), then the edge masks cleared (blocks are freed and reused: a
// stale mask is a wrong mesh), marked and counted, and the vertex prefix: the totals land in
// meshBase[n_total] and meshVBase[n_total].  The scratch is the context's from the first call on.
static hipError_t tfk_mesh_index_count(tf_ctx* c)
{
    hipError_t e = tfk_mesh_count(c);
    if (e != hipSuccess) return e;
    const size_t words = (size_t)c->p.n_blocks * TFM_EDGE_WORDS;
    if ((e = mesh_vcount_scratch(c)) != hipSuccess) return e;
    if (!c->meshMask) {
        e = tf_mem_hip(c->mem.alloc_group({ TfCtxMem::dev(&c->meshMask, sizeof(unsigned) * words), TfCtxMem::dev(&c->meshWPre, sizeof(unsigned) * words) }));
        if (e != hipSuccess) return e;
    }
    e = hipMemsetAsync(c->meshMask, 0, sizeof(unsigned) * words, c->stream);
    if (e != hipSuccess) return e;
    return mesh_mark_count(c, mesh_scene(c), MeshKeyBlock{ c->p.n_blocks }, c->meshMask, c->meshWPre);
}

// ... of the whole reading (a swapping context with a GlobalCache).  The entries that resolve are numbered
// first, and their number R comes to the host (one wait): the edge masks and prefixes are R rows of
// TFM_EDGE_WORDS words, a scratch of their own beside the resident form's, grown geometrically when R
// exceeds what is held and cleared every time, since the slots are numbered anew by every extraction.
static hipError_t tfk_mesh_index_count_whole(tf_ctx* c)
{
    hipError_t e = tfk_mesh_count(c, true);
    if (e != hipSuccess) return e;
    if ((e = mesh_vcount_scratch(c)) != hipSuccess) return e;
    const int ng = mesh_groups(c);
    if (!c->meshSlot) {
        e = tf_mem_hip(c->mem.alloc(&c->meshSlot, sizeof(int) * ((size_t)c->n_total + (size_t)ng + 1)));
        if (e != hipSuccess) return e;
    }
    const MeshSceneWhole s = mesh_scene_whole(c);
    int* gcount = c->meshSlot + c->n_total;
    hipLaunchKernelGGL(k_mesh_slot_count, mesh_grid(c), dim3(TFM_WG), 0, c->stream, s, gcount);
    hipLaunchKernelGGL(k_mesh_slot_assign, mesh_grid(c), dim3(TFM_WG), 0, c->stream, s, gcount, c->meshSlot, gcount + ng);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    int R = 0;
    e = hipMemcpyAsync(&R, gcount + ng, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return e;
    const long long need = R < 1 ? 1 : R;
    if (need > c->meshSlotCap) {
        const long long cap = need > 2 * c->meshSlotCap ? need : 2 * c->meshSlotCap;
        (void)c->mem.release(c->meshSlotMask);
        (void)c->mem.release(c->meshSlotWPre);
        c->meshSlotCap = 0;
        const size_t bytes = sizeof(unsigned) * TFM_EDGE_WORDS * (size_t)cap;
        e = tf_mem_hip(c->mem.alloc_group({ TfCtxMem::dev(&c->meshSlotMask, bytes), TfCtxMem::dev(&c->meshSlotWPre, bytes) }));
        if (e != hipSuccess) return e;
        c->meshSlotCap = cap;
    }
    e = hipMemsetAsync(c->meshSlotMask, 0, sizeof(unsigned) * TFM_EDGE_WORDS * (size_t)need, c->stream);
    if (e != hipSuccess) return e;
    return mesh_mark_count(c, s, MeshKeySlot{ c->meshSlot }, c->meshSlotMask, c->meshSlotWPre);
}

// after tfk_mesh_index_count[_whole] on the same stream: the vertex table's columns (each may be nullptr, one at
// least is not; colours need the colour plane and the resident reading), clipped at the same capacity
static hipError_t tfk_mesh_emit_vertices(tf_ctx* c, float* vertices, float* normals, unsigned char* colours, long long capacity, bool whole = false)
{
    mesh_dispatch_attr(normals != nullptr, colours != nullptr && !whole, [&](auto N, auto C) {
        if (whole) {
            if constexpr (!C())
                hipLaunchKernelGGL((k_mesh_emit_vertices<N(), false, MeshSceneWhole, MeshKeySlot>), mesh_grid(c), dim3(TFM_WG), 0, c->stream,
                                   mesh_scene_whole(c), MeshKeySlot{ c->meshSlot }, nullptr, c->meshSlotMask, c->meshSlotWPre, c->meshVCount,
                                   c->meshVBase, vertices, normals, nullptr, capacity, c->p.voxelSize);
        } else {
            hipLaunchKernelGGL((k_mesh_emit_vertices<N(), C(), MeshScene, MeshKeyBlock>), mesh_grid(c), dim3(TFM_WG), 0, c->stream, mesh_scene(c),
                               MeshKeyBlock{ c->p.n_blocks }, c->vba_rgb_guard, c->meshMask, c->meshWPre, c->meshVCount, c->meshVBase, vertices,
                               normals, reinterpret_cast<unsigned*>(colours), capacity, c->p.voxelSize);
        }
    });
    return hipGetLastError();
}

// after tfk_mesh_index_count[_whole] on the same stream: three vertex numbers per triangle, the first `capacity` triangles
static hipError_t tfk_mesh_emit_indices(tf_ctx* c, unsigned* indices, long long capacity, bool whole = false)
{
    if (whole)
        hipLaunchKernelGGL((k_mesh_emit_indices<MeshSceneWhole, MeshKeySlot>), mesh_grid(c), dim3(TFM_WG), 0, c->stream, mesh_scene_whole(c),
                           MeshKeySlot{ c->meshSlot }, c->meshSlotMask, c->meshSlotWPre, c->meshCount, c->meshBase, c->meshVBase, indices, capacity);
    else
        hipLaunchKernelGGL((k_mesh_emit_indices<MeshScene, MeshKeyBlock>), mesh_grid(c), dim3(TFM_WG), 0, c->stream, mesh_scene(c),
                           MeshKeyBlock{ c->p.n_blocks }, c->meshMask, c->meshWPre, c->meshCount, c->meshBase, c->meshVBase, indices, capacity);
    return hipGetLastError();
}

// ---- the entry points (additions: the reference has no mesher; DESIGN.md §Mesh extraction) -----------
// The PLY writers (tf_mesh_write_ply*) are host code of their own in tf_mesh_ply.cpp.
// count + prefix on the stream, then the total
static tf_status mesh_count(tf_ctx* c, long long* n, bool whole = false)
{
    TF_CHECK(tfk_mesh_count(c, whole));
    TF_CHECK(hipMemcpyAsync(n, c->meshBase + c->n_total, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    return sync_checked(c);
}

// tf_mesh_extract, tf_mesh_extract_attr and tf_mesh_extract_whole (no colours), after the flush
static tf_status mesh_extract(tf_ctx* c, float* dev_triangles, float* dev_normals, uint8_t* dev_colours, long long capacity, long long* n_triangles,
                              bool whole = false)
{
    const bool any = dev_triangles || dev_normals || dev_colours;
    if (!c || !n_triangles || capacity < 0 || (capacity > 0 && !any)) return TF_INVALID_ARG;
    if (dev_colours && !c->p.voxel_rgb) return TF_INVALID_ARG;
    long long n = 0;
    tf_status s = mesh_count(c, &n, whole);
    if (s != TF_OK) return s;
    *n_triangles = n;
    if (capacity == 0 || !any || n == 0) return TF_OK;
    TF_CHECK(order_after_caller(c));                      // the caller may still use the buffers on stream 0
    if (dev_normals || dev_colours) {
        TF_CHECK(tfk_mesh_emit_attr(c, dev_triangles, dev_normals, dev_colours, capacity, whole));
    } else {
        TF_CHECK(tfk_mesh_emit(c, dev_triangles, capacity, whole));
    }
    return sync_checked(c);
}

extern "C" tf_status tf_mesh_extract(tf_ctx* c, float* dev_triangles, long long capacity, long long* n_triangles)
{
    TF_FLUSH(c);
    return mesh_extract(c, dev_triangles, nullptr, nullptr, capacity, n_triangles);
}

extern "C" tf_status tf_mesh_extract_attr(tf_ctx* c, float* dev_triangles, float* dev_normals, uint8_t* dev_colours, long long capacity,
                                          long long* n_triangles)
{
    TF_FLUSH(c);
    return mesh_extract(c, dev_triangles, dev_normals, dev_colours, capacity, n_triangles);
}

extern "C" tf_status tf_mesh_extract_whole(tf_ctx* c, float* dev_triangles, float* dev_normals, long long capacity, long long* n_triangles)
{
    TF_FLUSH(c);
    return mesh_extract(c, dev_triangles, dev_normals, nullptr, capacity, n_triangles, true);
}

// What the tf_mesh_save_ply* share: `bytes` of output, written by emit(dev) on the context stream into a
// temporary device buffer, brought to *host (malloc'd, the caller frees; nullptr when bytes == 0)
template <class Emit>
static tf_status mesh_download(tf_ctx* c, size_t bytes, char** host, Emit emit)
{
    *host = nullptr;
    if (bytes == 0) return TF_OK;
    char* dev = nullptr;
    TfCtxMem tmp(c->mem.fns());                         // the device buffer, freed when this returns
    *host = (char*)malloc(bytes);
    if (!*host) return TF_OOM;
    if (tmp.alloc(&dev, bytes) != 0) { (void)hipGetLastError(); free(*host); *host = nullptr; return TF_OOM; }
    hipError_t e = emit(dev);
    if (e == hipSuccess) e = hipMemcpyAsync(*host, dev, bytes, hipMemcpyDeviceToHost, c->stream);
    tf_status s = tf_from_hip(e);
    const tf_status s2 = sync_checked(c);              // (the stream is idle before the buffer goes)
    if (s == TF_OK) s = s2;
    return s;
}

// The attribute column at `off` of the downloaded buffer when `want`ed, else nullptr.  An empty mesh has no
// buffer: its columns are still declared in the file (a non-null dummy, never read).
template <class T>
static const T* mesh_column(const char* host, size_t off, bool want)
{
    static const float none = 0.0f;
    return !want ? nullptr : host ? (const T*)(host + off) : (const T*)&none;
}

// tf_mesh_save_ply (attrs 0) and tf_mesh_save_ply_attr, after the flush.  TF_MESH_WHOLE: the whole map through
// the same writer -- one device buffer, one host buffer, one weld, so the caller's memory bounds the mesh.
static tf_status mesh_save_ply(tf_ctx* c, const char* path, int attrs)
{
    if (!c || !path || (attrs & ~(TF_MESH_NORMALS | TF_MESH_COLOURS | TF_MESH_WHOLE))) return TF_INVALID_ARG;
    if ((attrs & TF_MESH_COLOURS) && (!c->p.voxel_rgb || (attrs & TF_MESH_WHOLE))) return TF_INVALID_ARG;
    const bool whole = attrs & TF_MESH_WHOLE;
    long long n = 0;
    tf_status s = mesh_count(c, &n, whole);
    if (s != TF_OK) return s;
    const bool nrm = attrs & TF_MESH_NORMALS, col = attrs & TF_MESH_COLOURS;
    // one allocation each side: positions, then normals, then colours
    const size_t bt = sizeof(float) * 9 * (size_t)n, bn = nrm ? bt : 0, bc = col ? 12 * (size_t)n : 0;
    char* host = nullptr;
    s = mesh_download(c, bt + bn + bc, &host, [&](char* dev) {
        if (!nrm && !col) return tfk_mesh_emit(c, (float*)dev, n, whole);
        return tfk_mesh_emit_attr(c, (float*)dev, nrm ? (float*)(dev + bt) : nullptr, col ? (unsigned char*)(dev + bt + bn) : nullptr, n, whole);
    });
    if (s == TF_OK)
        s = tf_mesh_write_ply_attr(path, (const float*)host, mesh_column<float>(host, bt, nrm), mesh_column<uint8_t>(host, bt + bn, col), n);
    free(host);
    return s;
}

extern "C" tf_status tf_mesh_save_ply(tf_ctx* c, const char* path)
{
    TF_FLUSH(c);
    return mesh_save_ply(c, path, 0);
}

extern "C" tf_status tf_mesh_save_ply_attr(tf_ctx* c, const char* path, int attrs)
{
    TF_FLUSH(c);
    return mesh_save_ply(c, path, attrs);
}

// ---- indexed mesh extraction (additions; DESIGN.md §Mesh extraction, indexed) ---------------------------
// triangle and vertex totals after the count passes.  whole: the reading over both tiers, by the slot-keyed
// kernels where the context has a GlobalCache and by the resident ones where it has none
static tf_status mesh_index_count(tf_ctx* c, long long* nv, long long* nt, bool whole = false)
{
    const hipError_t e = mesh_reads_store(c, whole) ? tfk_mesh_index_count_whole(c) : tfk_mesh_index_count(c);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return TF_OOM; }
    TF_CHECK(e);
    TF_CHECK(hipMemcpyAsync(nt, c->meshBase + c->n_total, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    TF_CHECK(hipMemcpyAsync(nv, c->meshVBase + c->n_total, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    return sync_checked(c);
}

// tf_mesh_extract_indexed and tf_mesh_extract_indexed_whole (no colours), after the flush
static tf_status mesh_extract_indexed(tf_ctx* c, float* dev_vertices, float* dev_normals, uint8_t* dev_colours, long long vertex_capacity,
                                      uint32_t* dev_indices, long long triangle_capacity, long long* n_vertices, long long* n_triangles,
                                      bool whole = false)
{
    const bool any = dev_vertices || dev_normals || dev_colours;
    if (!c || !n_vertices || !n_triangles || vertex_capacity < 0 || triangle_capacity < 0) return TF_INVALID_ARG;
    if ((vertex_capacity > 0 && !any) || (triangle_capacity > 0 && !dev_indices)) return TF_INVALID_ARG;
    if (dev_colours && !c->p.voxel_rgb) return TF_INVALID_ARG;
    long long nv = 0, nt = 0;
    tf_status s = mesh_index_count(c, &nv, &nt, whole);
    if (s != TF_OK) return s;
    *n_vertices = nv;
    *n_triangles = nt;
    if (nv > 0xffffffffLL) return TF_INDEX_RANGE;
    const bool verts = any && vertex_capacity > 0 && nv > 0, tris = dev_indices && triangle_capacity > 0 && nt > 0;
    if (!verts && !tris) return TF_OK;
    const bool store = mesh_reads_store(c, whole);
    TF_CHECK(order_after_caller(c));                      // the caller may still use the buffers on stream 0
    if (verts) TF_CHECK(tfk_mesh_emit_vertices(c, dev_vertices, dev_normals, dev_colours, vertex_capacity, store));
    if (tris) TF_CHECK(tfk_mesh_emit_indices(c, dev_indices, triangle_capacity, store));
    return sync_checked(c);
}

extern "C" tf_status tf_mesh_extract_indexed(tf_ctx* c, float* dev_vertices, float* dev_normals, uint8_t* dev_colours,
                                             long long vertex_capacity, uint32_t* dev_indices, long long triangle_capacity,
                                             long long* n_vertices, long long* n_triangles)
{
    TF_FLUSH(c);
    return mesh_extract_indexed(c, dev_vertices, dev_normals, dev_colours, vertex_capacity, dev_indices, triangle_capacity, n_vertices, n_triangles);
}

extern "C" tf_status tf_mesh_extract_indexed_whole(tf_ctx* c, float* dev_vertices, float* dev_normals, long long vertex_capacity,
                                                   uint32_t* dev_indices, long long triangle_capacity, long long* n_vertices,
                                                   long long* n_triangles)
{
    TF_FLUSH(c);
    return mesh_extract_indexed(c, dev_vertices, dev_normals, nullptr, vertex_capacity, dev_indices, triangle_capacity, n_vertices, n_triangles,
                                true);
}

// The whole map as an indexed PLY in bounded pieces.  The device holds the columns (positions, normals,
// indices: a quarter to a third of the soup's bytes); they come to the host through a pinned staging buffer of
// mesh_chunk_bytes (TFUSION_MESH_CHUNK_BYTES), the context's from the first call on, a chunk of vertices
// (position and normal rows side by side) or of faces at a time, and the streaming writer (tf_mesh_ply.cpp)
// interleaves each chunk into the file's records.  Host memory is the chunk, whatever the mesh.
extern "C" tf_status tf_mesh_save_ply_indexed_whole(tf_ctx* c, const char* path, int attrs)
{
    TF_FLUSH(c);
    if (!c || !path || (attrs & ~TF_MESH_NORMALS)) return TF_INVALID_ARG;
    long long nv = 0, nt = 0;
    tf_status s = mesh_index_count(c, &nv, &nt, true);
    if (s != TF_OK) return s;
    if (nv > 0x7fffffffLL) return TF_INDEX_RANGE;       // (the PLY's indices are int)
    const bool nrm = attrs & TF_MESH_NORMALS, store = mesh_reads_store(c, true);
    if (nt == 0) nv = 0;                                 // (no vertex is unreferenced)
    if (!c->meshPinned) {
        const hipError_t e = tf_mem_hip(c->mem.alloc(TfCtxMem::pin(&c->meshPinned, (size_t)c->mesh_chunk_bytes, hipHostMallocDefault)));
        if (e != hipSuccess) { (void)hipGetLastError(); return TF_OOM; }
    }
    const size_t bp = 12 * (size_t)nv, bn = nrm ? bp : 0, bi = 12 * (size_t)nt;
    char* dev = nullptr;
    TfCtxMem tmp(c->mem.fns());                         // the device columns, freed when this returns
    if (nt > 0) {
        if (tmp.alloc(&dev, bp + bn + bi) != 0) { (void)hipGetLastError(); return TF_OOM; }
        TF_CHECK(tfk_mesh_emit_vertices(c, (float*)dev, nrm ? (float*)(dev + bp) : nullptr, nullptr, nv, store));
        TF_CHECK(tfk_mesh_emit_indices(c, (unsigned*)(dev + bp + bn), nt, store));
    }
    tf_ply_stream* ps = nullptr;
    s = tf_mesh_ply_begin(path, nv, nt, attrs, &ps);
    if (s != TF_OK) { (void)sync_checked(c); return s; }
    unsigned char* pin = c->meshPinned;
    const long long vrows = c->mesh_chunk_bytes / (nrm ? 24 : 12), frows = c->mesh_chunk_bytes / 12;
    hipError_t e = hipSuccess;
    for (long long v0 = 0; v0 < nv && s == TF_OK && e == hipSuccess; v0 += vrows) {
        const long long k = nv - v0 < vrows ? nv - v0 : vrows;
        e = hipMemcpyAsync(pin, dev + 12 * v0, 12 * (size_t)k, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && nrm) e = hipMemcpyAsync(pin + 12 * k, dev + bp + 12 * v0, 12 * (size_t)k, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) s = tf_mesh_ply_vertices(ps, (const float*)pin, nrm ? (const float*)(pin + 12 * k) : nullptr, nullptr, k);
    }
    for (long long t0 = 0; t0 < nt && s == TF_OK && e == hipSuccess; t0 += frows) {
        const long long k = nt - t0 < frows ? nt - t0 : frows;
        e = hipMemcpyAsync(pin, dev + bp + bn + 12 * t0, 12 * (size_t)k, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) s = tf_mesh_ply_faces(ps, (const uint32_t*)pin, k);
    }
    if (s == TF_OK && e != hipSuccess) s = tf_from_hip(e);
    const tf_status s2 = sync_checked(c);               // (the stream is idle before the device buffer goes)
    if (s == TF_OK) s = s2;
    const tf_status s3 = tf_mesh_ply_end(ps, s == TF_OK);     // (a failure so far: the file is removed)
    return s == TF_OK ? s3 : s;
}

extern "C" tf_status tf_mesh_save_ply_indexed(tf_ctx* c, const char* path, int attrs)
{
    TF_FLUSH(c);
    if (!c || !path || (attrs & ~(TF_MESH_NORMALS | TF_MESH_COLOURS | TF_MESH_INDEXED))) return TF_INVALID_ARG;
    if ((attrs & TF_MESH_COLOURS) && !c->p.voxel_rgb) return TF_INVALID_ARG;
    long long nv = 0, nt = 0;
    tf_status s = mesh_index_count(c, &nv, &nt);
    if (s != TF_OK) return s;
    if (nv > 0x7fffffffLL) return TF_INDEX_RANGE;       // (the PLY's indices are int)
    const bool nrm = attrs & TF_MESH_NORMALS, col = attrs & TF_MESH_COLOURS;
    // one allocation each side: positions, normals, colours, indices
    const size_t bp = 12 * (size_t)nv, bn = nrm ? bp : 0, bc = col ? 4 * (size_t)nv : 0, bi = 12 * (size_t)nt;
    char* host = nullptr;
    s = mesh_download(c, nt > 0 ? bp + bn + bc + bi : 0, &host, [&](char* dev) {
        const hipError_t e = tfk_mesh_emit_vertices(c, (float*)dev, nrm ? (float*)(dev + bp) : nullptr, col ? (unsigned char*)(dev + bp + bn) : nullptr, nv);
        return e == hipSuccess ? tfk_mesh_emit_indices(c, (unsigned*)(dev + bp + bn + bc), nt) : e;
    });
    if (s == TF_OK)
        s = tf_mesh_write_ply_indexed(path, (const float*)host, mesh_column<float>(host, bp, nrm), mesh_column<uint8_t>(host, bp + bn, col),
                                      nt > 0 ? nv : 0, host ? (const uint32_t*)(host + bp + bn + bc) : nullptr, nt);
    free(host);
    return s;
}
