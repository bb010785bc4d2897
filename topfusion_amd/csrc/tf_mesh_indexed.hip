// tf_mesh_indexed.hip -- the indexed form of mesh extraction for gfx950 (an addition, as tf_mesh.hip is):
// the triangles of tf_mesh_extract with shared vertices and u32 indices (DESIGN.md §Mesh extraction,
// indexed).  Its kernels live apart from tf_mesh.hip's so that those compile exactly as before.
//
// A vertex is its Kuhn edge (tf_mesh.h): per VBA block a mask of 512 x 7 edge bits (TFM_EDGE_WORDS words,
// indexed by the block number ptr) and the words' exclusive popcount prefixes; per hash entry its
// vertex count and base, by k_mesh_prefix on a second pair of arrays.
//
//   k_mesh_mark          : k_mesh_count's loop; every valid cube ORs its sign-changing Kuhn edges into the
//                          owners' masks -- gathered in LDS, flushed with one global atomicOr per non-zero
//                          word (integer OR: the result does not depend on the order of arrival)
//   k_mesh_vcount        : one wave per live entry: the 112 words' popcounts, scanned -> prefixes, count
//   k_mesh_emit_vertices : per live entry with vertices, each thread its voxel's seven edges; a set bit is
//                          the vertex base + prefix + popcount below
//   k_mesh_emit_indices  : k_mesh_emit's structure; a triangle vertex (lo, hi) -> owner block, bit, index
//
// No workgroup waits on another inside a grid.  The scene (hash, VBA, block grid) is only read.
#include "tf_mesh_dev.h"

typedef unsigned tfm_u3 __attribute__((ext_vector_type(3), aligned(4)));

// mesh_block_voff with the hash entry beside the offset: (entry, voff) or (-1, TF_VOFF_NONE)
__device__ __forceinline__ int2 mesh_block_look(const MeshScene& s, int bx, int by, int bz)
{
    if (tf_grid_in(bx, by, bz)) return s.v.grid[tf_grid_cell(bx, by, bz)];
    if (bx > 32767 || by > 32767 || bz > 32767) return make_int2(-1, TF_VOFF_NONE);
    return blk_walk(s.v, bx, by, bz);
}

struct MeshMarker {
    unsigned* lmask;             // LDS, [8][TFM_EDGE_WORDS]
    __device__ __forceinline__ void operator()(const TfmEdgeRef& r) { atomicOr(&lmask[r.owner * TFM_EDGE_WORDS + (r.bit >> 5)], 1u << (r.bit & 31u)); }
};

__global__ __launch_bounds__(TFM_WG) void k_mesh_mark(MeshScene s, unsigned* __restrict__ mask, int n_blocks)
{
    __shared__ unsigned tile[TFM_TILE3];
    __shared__ int nvoff[8];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ unsigned lmask[8 * TFM_EDGE_WORDS];
    const int t = threadIdx.x;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        __syncthreads();
        if (t == 0) nlive = 0;
        __syncthreads();
        const int idx = g * TFM_WG + t;
        if (idx < s.n_total && s.v.hash[idx].ptr >= 0) live[atomicAdd(&nlive, 1)] = idx;      // (any order: OR commutes)
        __syncthreads();
        const int n = nlive;
        for (int k = 0; k < n; ++k) {
            const TfHashEntry e = s.v.hash[live[k]];
            mesh_stage(s, e, tile, nvoff);           // (its first barrier: the previous entry's flush is done)
            for (int i = t; i < 8 * TFM_EDGE_WORDS; i += TFM_WG) lmask[i] = 0u;
            __syncthreads();
            MeshMarker mk = { lmask };
            tfm_cube_mark(mesh_cube(tile), t & 7, t >> 3 & 7, t >> 6, mk);
            __syncthreads();
            for (int i = t; i < 8 * TFM_EDGE_WORDS; i += TFM_WG) {
                const unsigned w = lmask[i];
                if (w) {
                    // the owner holds a corner of a valid cube (w > 0), so its block exists; the guards only bound the store
                    const int o = i / TFM_EDGE_WORDS, blk = nvoff[o] >> 9;
                    if (nvoff[o] >= 0 && blk < n_blocks) atomicOr(&mask[(size_t)blk * TFM_EDGE_WORDS + (i - o * TFM_EDGE_WORDS)], w);
                }
            }
        }
    }
}

// Per live entry (one wave each) the exclusive popcount prefix of its block's mask words and its vertex
// count; dead entries count 0; each 512-entry group's total beside, as k_mesh_count leaves them.
__global__ __launch_bounds__(TFM_WG) void k_mesh_vcount(MeshScene s, const unsigned* __restrict__ mask, unsigned* __restrict__ wpre, int n_blocks,
                                                        long long* __restrict__ count, long long* __restrict__ groupTot)
{
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ int gsum;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        __syncthreads();
        if (t == 0) { nlive = 0; gsum = 0; }
        __syncthreads();
        const int idx = g * TFM_WG + t;
        if (idx < s.n_total) {
            if (s.v.hash[idx].ptr >= 0) live[atomicAdd(&nlive, 1)] = idx;
            else count[idx] = 0;
        }
        __syncthreads();
        const int n = nlive;
        for (int k = wave; k < n; k += TFM_WG / 64) {
            const int ei = live[k];
            const int blk = s.v.hash[ei].ptr;
            int total = 0;
            if (blk < n_blocks) {
                const size_t at = (size_t)blk * TFM_EDGE_WORDS;
                const int ca = __popc(mask[at + lane]);
                const int cb = lane < TFM_EDGE_WORDS - 64 ? __popc(mask[at + 64 + lane]) : 0;
                int ia = ca, ib = cb;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
                    if (lane >= o) { ia += ua; ib += ub; }
                }
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

typedef float tfm_f3 __attribute__((ext_vector_type(3), aligned(4)));

__device__ __forceinline__ void mesh_store3(float* p, const float* v)
{
    tfm_f3 a;
    a.x = v[0]; a.y = v[1]; a.z = v[2];
    *reinterpret_cast<tfm_f3*>(p) = a;
}

// The vertex table: positions (may be nullptr), normals, colours (one RGBA word per vertex), each clipped
// at `capacity` vertices.  The tile is the attributed kernel's; a block's vertices are contiguous.
template <bool NORMALS, bool COLOURS>
__global__ __launch_bounds__(TFM_WG) void k_mesh_emit_vertices(MeshScene s, const unsigned* __restrict__ rgb, const unsigned* __restrict__ mask,
                                                               const unsigned* __restrict__ wpre, const long long* __restrict__ vcount,
                                                               const long long* __restrict__ vbase, float* __restrict__ outPos,
                                                               float* __restrict__ outNrm, unsigned* __restrict__ outCol, long long capacity,
                                                               float voxelSize)
{
    __shared__ unsigned tile[TFM_ATILE3];
    __shared__ int grad3[NORMALS ? 3 * TFM_TILE3 : 1];
    __shared__ unsigned ctile[COLOURS ? TFM_TILE3 : 1];
    __shared__ int nvoff[27];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ unsigned lm[TFM_EDGE_WORDS + 1], lpre[TFM_EDGE_WORDS];
    const int t = threadIdx.x;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        __syncthreads();
        if (t == 0) { nlive = 0; lm[TFM_EDGE_WORDS] = 0u; }
        __syncthreads();
        const int idx = g * TFM_WG + t;
        if (idx < s.n_total && vcount[idx] > 0 && vbase[idx] < capacity) live[atomicAdd(&nlive, 1)] = idx;
        __syncthreads();
        const int n = nlive;
        for (int k = 0; k < n; ++k) {
            const int ei = live[k];
            const TfHashEntry e = s.v.hash[ei];
            mesh_stage_attr<NORMALS, COLOURS>(s, rgb, e, tile, ctile, nvoff);
            if (t < TFM_EDGE_WORDS) {                // (vcount > 0: the entry is live and its block below n_blocks)
                lm[t] = mask[(size_t)e.ptr * TFM_EDGE_WORDS + t];
                lpre[t] = wpre[(size_t)e.ptr * TFM_EDGE_WORDS + t];
            }
            if (NORMALS) {
                for (int i = t; i < TFM_TILE3; i += TFM_WG) {
                    const int z = i / (TFM_TILE * TFM_TILE), r = i - z * (TFM_TILE * TFM_TILE), y = r / TFM_TILE, x = r - y * TFM_TILE;
                    const int c = (x + 1) + TFM_ATILE * (y + 1) + TFM_ATILE * TFM_ATILE * (z + 1);
                    const unsigned v0 = tile[c];
                    grad3[i] = tfm_grad_axis_packed(tile[c - 1], v0, tile[c + 1]);
                    grad3[TFM_TILE3 + i] = tfm_grad_axis_packed(tile[c - TFM_ATILE], v0, tile[c + TFM_ATILE]);
                    grad3[2 * TFM_TILE3 + i] = tfm_grad_axis_packed(tile[c - TFM_ATILE * TFM_ATILE], v0, tile[c + TFM_ATILE * TFM_ATILE]);
                }
            }
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
    const int* nvoff;            // LDS: the eight blocks' voxel offsets
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
                } else if (nvoff[r.owner] >= 0) {        // (always: the owner holds a corner of this valid cube)
                    const size_t at = (size_t)(nvoff[r.owner] >> 9) * TFM_EDGE_WORDS + w;
                    m = mask[at]; pre = wpre[at];
                }
                tri[v] = (unsigned)(nbase[r.owner] + tfm_edge_rank(m, pre, r.bit));
            }
            *reinterpret_cast<tfm_u3*>(out + idx * 3) = tri;
        }
        ++idx;
    }
};

__global__ __launch_bounds__(TFM_WG) void k_mesh_emit_indices(MeshScene s, const unsigned* __restrict__ mask, const unsigned* __restrict__ wpre,
                                                              const long long* __restrict__ count, const long long* __restrict__ base,
                                                              const long long* __restrict__ vbase, unsigned* __restrict__ out, long long capacity)
{
    __shared__ unsigned tile[TFM_TILE3];
    __shared__ int nvoff[8];
    __shared__ long long nbase[8];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ int wsum[TFM_WG / 64];
    __shared__ unsigned lm[TFM_EDGE_WORDS], lpre[TFM_EDGE_WORDS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        __syncthreads();
        if (t == 0) nlive = 0;
        __syncthreads();
        const int idx = g * TFM_WG + t;
        if (idx < s.n_total && count[idx] > 0 && base[idx] < capacity) live[atomicAdd(&nlive, 1)] = idx;
        __syncthreads();
        const int n = nlive;
        for (int k = 0; k < n; ++k) {
            const int ei = live[k];
            const TfHashEntry e = s.v.hash[ei];
            // mesh_stage with the eight blocks' entries: their vertex bases (a missing block owns nothing)
            __syncthreads();
            if (t < 8) {
                const int2 b = t == 0 ? make_int2(ei, e.ptr * TF_BLK3) : mesh_block_look(s, e.x + (t & 1), e.y + (t >> 1 & 1), e.z + (t >> 2));
                nvoff[t] = b.y;
                nbase[t] = b.y >= 0 ? vbase[b.x] : 0;
            }
            if (t >= 64 && t < 64 + TFM_EDGE_WORDS) {
                lm[t - 64] = mask[(size_t)e.ptr * TFM_EDGE_WORDS + (t - 64)];
                lpre[t - 64] = wpre[(size_t)e.ptr * TFM_EDGE_WORDS + (t - 64)];
            }
            __syncthreads();
            for (int i = t; i < TFM_TILE3; i += TFM_WG) {
                const int z = i / (TFM_TILE * TFM_TILE), r = i - z * (TFM_TILE * TFM_TILE), y = r / TFM_TILE, x = r - y * TFM_TILE;
                const int voff = nvoff[(x >> 3) | (y >> 3) << 1 | (z >> 3) << 2];
                const TfVoxel v = s.v.vba[TF_BLK3 + voff + (x & 7) + ((y & 7) << 3) + ((z & 7) << 6)];
                tile[i] = (unsigned)(unsigned short)v.sdf | (unsigned)v.w << 16;
            }
            __syncthreads();
            const TfmCube q = mesh_cube(tile);
            const int mine = tfm_cube_count(q);
            int inc = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(inc, o, 64);
                if (lane >= o) inc += up;
            }
            if (lane == 63) wsum[wave] = inc;
            __syncthreads();
            int off = inc - mine;
            for (int w = 0; w < wave; ++w) off += wsum[w];
            if (mine) {
                MeshIndexWriter wr = { lm, lpre, nvoff, nbase, mask, wpre, out, t & 7, t >> 3 & 7, t >> 6, base[ei] + off, capacity };
                tfm_cube_emit_edges(q, wr);
            }
        }
    }
}

// ---- indexed extraction: the host side ------------------------------------------------------------------
// Triangle count + prefix (tfk_mesh_count), then the edge masks cleared (blocks are freed and reused: a
// stale mask is a wrong mesh), marked and counted, and the vertex prefix: the totals land in
// meshBase[n_total] and meshVBase[n_total].  The scratch is the context's from the first call on.
hipError_t tfk_mesh_index_count(tf_ctx* c)
{
    hipError_t e = tfk_mesh_count(c);
    if (e != hipSuccess) return e;
    const int ng = mesh_groups(c);
    const size_t words = (size_t)c->p.n_blocks * TFM_EDGE_WORDS;
    if (!c->meshMask) {
        void* b[4] = { nullptr, nullptr, nullptr, nullptr };
        const size_t bytes[4] = { sizeof(unsigned) * words, sizeof(unsigned) * words, sizeof(long long) * ((size_t)c->n_total + (size_t)ng),
                                  sizeof(long long) * ((size_t)c->n_total + 1) };
        for (int i = 0; i < 4; ++i) {
            e = hipMalloc(&b[i], bytes[i]);
            if (e != hipSuccess) {
                for (int j = 0; j < i; ++j) (void)hipFree(b[j]);
                return e;
            }
        }
        c->meshMask = (unsigned*)b[0]; c->meshWPre = (unsigned*)b[1]; c->meshVCount = (long long*)b[2]; c->meshVBase = (long long*)b[3];
    }
    e = hipMemsetAsync(c->meshMask, 0, sizeof(unsigned) * words, c->stream);
    if (e != hipSuccess) return e;
    long long* groupTot = c->meshVCount + c->n_total;
    const dim3 grid(ng < TFM_GRID ? ng : TFM_GRID), wg(TFM_WG);
    hipLaunchKernelGGL(k_mesh_mark, grid, wg, 0, c->stream, mesh_scene(c), c->meshMask, c->p.n_blocks);
    hipLaunchKernelGGL(k_mesh_vcount, grid, wg, 0, c->stream, mesh_scene(c), c->meshMask, c->meshWPre, c->p.n_blocks, c->meshVCount, groupTot);
    e = hipGetLastError();
    return e == hipSuccess ? tfk_mesh_prefix(c, c->meshVCount, groupTot, c->meshVBase) : e;
}

// after tfk_mesh_index_count on the same stream: the vertex table's columns (each may be nullptr, one at
// least is not; colours need the colour plane), clipped at the same capacity
hipError_t tfk_mesh_emit_vertices(tf_ctx* c, float* vertices, float* normals, unsigned char* colours, long long capacity)
{
    const int ng = mesh_groups(c);
    const dim3 grid(ng < TFM_GRID ? ng : TFM_GRID), wg(TFM_WG);
    unsigned* col = reinterpret_cast<unsigned*>(colours);
#define TFM_LAUNCH_VERTICES(N, C)                                                                                                      \
    hipLaunchKernelGGL((k_mesh_emit_vertices<N, C>), grid, wg, 0, c->stream, mesh_scene(c), c->vba_rgb_guard, c->meshMask, c->meshWPre, \
                       c->meshVCount, c->meshVBase, vertices, normals, col, capacity, c->p.voxelSize)
    if (normals && colours) TFM_LAUNCH_VERTICES(true, true);
    else if (normals) TFM_LAUNCH_VERTICES(true, false);
    else if (colours) TFM_LAUNCH_VERTICES(false, true);
    else TFM_LAUNCH_VERTICES(false, false);
#undef TFM_LAUNCH_VERTICES
    return hipGetLastError();
}

// after tfk_mesh_index_count on the same stream: three vertex numbers per triangle, the first `capacity` triangles
hipError_t tfk_mesh_emit_indices(tf_ctx* c, unsigned* indices, long long capacity)
{
    const int ng = mesh_groups(c);
    hipLaunchKernelGGL(k_mesh_emit_indices, dim3(ng < TFM_GRID ? ng : TFM_GRID), dim3(TFM_WG), 0, c->stream, mesh_scene(c), c->meshMask,
                       c->meshWPre, c->meshCount, c->meshBase, c->meshVBase, indices, capacity);
    return hipGetLastError();
}
