// tf_mesh.hip -- mesh extraction from the voxel block hash for gfx950 (an addition: the reference has no
// mesher).  Marching tetrahedra on the Kuhn split of every voxel cube (tf_mesh.h, DESIGN.md §Mesh
// extraction), as three plain launches on the context stream:
//
//   k_mesh_count  : per live hash entry (ptr >= 0) the 9 x 9 x 9 corner voxels of its 512 cubes staged in
//                   LDS (own block + up to seven neighbours, found through the block grid, outside it by
//                   the hash walk), every cube classified, the entry's triangle count (64-bit) written;
//                   dead entries get 0; each 512-entry group's total written beside
//   k_mesh_prefix : exclusive scan of the counts in entry order -> every entry's base, and the total
//   k_mesh_emit   : the classification again, an exclusive scan over the 512 voxels inside the
//                   workgroup, triangles written at base + offset while below the caller's capacity
//
//   k_mesh_emit_attr<NORMALS, COLOURS> : k_mesh_emit with per-vertex normals (TSDF gradient) and / or colours
//                   (colour plane) beside the positions, from a larger LDS tile of its own
//
//   k_mesh_mark, k_mesh_vcount, k_mesh_emit_vertices<NORMALS, COLOURS>, k_mesh_emit_indices : the indexed
//                   form of the same mesh (shared vertices, u32 indices), in tf_mesh_indexed.hip
//
// No workgroup waits on another inside a grid.  The scene (hash, VBA, block grid) is only read.
#include "tf_mesh_dev.h"

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(TFM_WG) void k_mesh_count(MeshScene s, long long* __restrict__ count, long long* __restrict__ groupTot)
{
    __shared__ unsigned tile[TFM_TILE3];
    __shared__ int nvoff[8];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ int wsum[TFM_WG / 64];
    const int t = threadIdx.x;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        __syncthreads();
        if (t == 0) nlive = 0;
        __syncthreads();
        const int idx = g * TFM_WG + t;
        if (idx < s.n_total) {
            if (s.v.hash[idx].ptr >= 0) live[atomicAdd(&nlive, 1)] = idx;      // (any order: each entry's count stands alone)
            else count[idx] = 0;
        }
        __syncthreads();
        const int n = nlive;
        long long tot = 0;
        for (int k = 0; k < n; ++k) {
            const int ei = live[k];
            const TfHashEntry e = s.v.hash[ei];
            mesh_stage(s, e, tile, nvoff);
            const int c = wave_sum(tfm_cube_count(mesh_cube(tile)));
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

// 4-byte aligned 16-byte store: a triangle is 36 bytes, so its address is only dword aligned
typedef float tfm_f4 __attribute__((ext_vector_type(4), aligned(4)));

struct MeshWriter {
    float* out;
    long long idx;           // the next triangle's index
    long long capacity;
    __device__ __forceinline__ void operator()(const float* tri)
    {
        if (idx < capacity) {
            float* p = out + idx * 9;
            tfm_f4 a, b;
            a.x = tri[0]; a.y = tri[1]; a.z = tri[2]; a.w = tri[3];
            b.x = tri[4]; b.y = tri[5]; b.z = tri[6]; b.w = tri[7];
            *reinterpret_cast<tfm_f4*>(p) = a;
            *reinterpret_cast<tfm_f4*>(p + 4) = b;
            p[8] = tri[8];
        }
        ++idx;
    }
};

__global__ __launch_bounds__(TFM_WG) void k_mesh_emit(MeshScene s, const long long* __restrict__ count, const long long* __restrict__ base,
                                                      float* __restrict__ out, long long capacity, float voxelSize)
{
    __shared__ unsigned tile[TFM_TILE3];
    __shared__ int nvoff[8];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ int wsum[TFM_WG / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ngroups = (s.n_total + TFM_WG - 1) / TFM_WG;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        __syncthreads();
        if (t == 0) nlive = 0;
        __syncthreads();
        const int idx = g * TFM_WG + t;
        // entries with triangles below the capacity (count and base are uniform per entry)
        if (idx < s.n_total && count[idx] > 0 && base[idx] < capacity) live[atomicAdd(&nlive, 1)] = idx;
        __syncthreads();
        const int n = nlive;
        for (int k = 0; k < n; ++k) {
            const int ei = live[k];
            const TfHashEntry e = s.v.hash[ei];
            mesh_stage(s, e, tile, nvoff);
            const TfmCube q = mesh_cube(tile);
            const int mine = tfm_cube_count(q);
            // exclusive scan over the 512 voxels: inclusive within the wave, then the lower waves' sums
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
                MeshWriter wr = { out, base[ei] + off, capacity };
                tfm_cube_emit(q, e.x * TF_BLK + (t & 7), e.y * TF_BLK + (t >> 3 & 7), e.z * TF_BLK + (t >> 6), voxelSize, wr);
            }
        }
    }
}

// ---- the emit pass with per-vertex attributes (normals, colours) -------------------------------------
// Its own kernel beside k_mesh_emit: the larger tile, the gradients and the colour words live in its
// LDS alone.  Per entry: the 11 x 11 x 11 voxels around the block (local coordinates -1 .. 9; only points
// with at most one coordinate outside 0 .. 8 are read, the others never are) from the block and up to 19
// neighbours, the 9 x 9 x 9 integer gradients formed once from it, the colour words of the same 9 x 9 x 9
// corners; then k_mesh_emit's classification and scan, and per triangle vertex two LDS gradient / colour
// reads per end.  (The tile itself -- mesh_stage_attr, MeshAttrSrc -- is in tf_mesh_dev.h: the indexed
// form's vertex pass stages the same one.)
__device__ __forceinline__ void mesh_store9(float* p, const float* v)
{
    tfm_f4 a, b;
    a.x = v[0]; a.y = v[1]; a.z = v[2]; a.w = v[3];
    b.x = v[4]; b.y = v[5]; b.z = v[6]; b.w = v[7];
    *reinterpret_cast<tfm_f4*>(p) = a;
    *reinterpret_cast<tfm_f4*>(p + 4) = b;
    p[8] = v[8];
}

typedef unsigned tfm_u3 __attribute__((ext_vector_type(3), aligned(4)));

template <bool NORMALS, bool COLOURS>
struct MeshAttrWriter {
    float* tri;                  // may be nullptr (uniform)
    float* nrm;
    unsigned* col;
    long long idx;
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

template <bool NORMALS, bool COLOURS>
__global__ __launch_bounds__(TFM_WG) void k_mesh_emit_attr(MeshScene s, const unsigned* __restrict__ rgb, const long long* __restrict__ count,
                                                           const long long* __restrict__ base, float* __restrict__ outTri,
                                                           float* __restrict__ outNrm, unsigned* __restrict__ outCol, long long capacity,
                                                           float voxelSize)
{
    __shared__ unsigned tile[TFM_ATILE3];
    __shared__ int grad3[NORMALS ? 3 * TFM_TILE3 : 1];
    __shared__ unsigned ctile[COLOURS ? TFM_TILE3 : 1];
    __shared__ int nvoff[27];
    __shared__ int live[TFM_WG];
    __shared__ int nlive;
    __shared__ int wsum[TFM_WG / 64];
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
            mesh_stage_attr<NORMALS, COLOURS>(s, rgb, e, tile, ctile, nvoff);
            if (NORMALS) {
                // the 9^3 lattice gradients, once per entry (the tile is complete: mesh_stage_attr ends in a barrier)
                for (int i = t; i < TFM_TILE3; i += TFM_WG) {
                    const int z = i / (TFM_TILE * TFM_TILE), r = i - z * (TFM_TILE * TFM_TILE), y = r / TFM_TILE, x = r - y * TFM_TILE;
                    const int c = (x + 1) + TFM_ATILE * (y + 1) + TFM_ATILE * TFM_ATILE * (z + 1);
                    const unsigned v0 = tile[c];
                    grad3[i] = tfm_grad_axis_packed(tile[c - 1], v0, tile[c + 1]);
                    grad3[TFM_TILE3 + i] = tfm_grad_axis_packed(tile[c - TFM_ATILE], v0, tile[c + TFM_ATILE]);
                    grad3[2 * TFM_TILE3 + i] = tfm_grad_axis_packed(tile[c - TFM_ATILE * TFM_ATILE], v0, tile[c + TFM_ATILE * TFM_ATILE]);
                }
            }
            const TfmCube q = mesh_cube_attr(tile);
            const int mine = tfm_cube_count(q);
            int inc = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(inc, o, 64);
                if (lane >= o) inc += up;
            }
            if (lane == 63) wsum[wave] = inc;
            __syncthreads();         // wsum, and the gradients
            int off = inc - mine;
            for (int w = 0; w < wave; ++w) off += wsum[w];
            if (mine) {
                const MeshAttrSrc<NORMALS, COLOURS> src = { grad3, ctile, (t & 7) + TFM_TILE * (t >> 3 & 7) + TFM_TILE * TFM_TILE * (t >> 6) };
                MeshAttrWriter<NORMALS, COLOURS> wr = { outTri, outNrm, outCol, base[ei] + off, capacity };
                tfm_cube_emit_attr(q, e.x * TF_BLK + (t & 7), e.y * TF_BLK + (t >> 3 & 7), e.z * TF_BLK + (t >> 6), voxelSize, src, wr);
            }
        }
    }
}

// count + prefix; the scratch (counts, bases + total, group totals behind the counts) is the
// context's from the first call on
hipError_t tfk_mesh_count(tf_ctx* c)
{
    const int ng = mesh_groups(c);
    if (!c->meshCount) {
        hipError_t e = hipMalloc((void**)&c->meshCount, sizeof(long long) * ((size_t)c->n_total + (size_t)ng));
        if (e != hipSuccess) { c->meshCount = nullptr; return e; }
        e = hipMalloc((void**)&c->meshBase, sizeof(long long) * ((size_t)c->n_total + 1));
        if (e != hipSuccess) { (void)hipFree(c->meshCount); c->meshCount = nullptr; c->meshBase = nullptr; return e; }
    }
    long long* groupTot = c->meshCount + c->n_total;
    hipLaunchKernelGGL(k_mesh_count, dim3(ng < TFM_GRID ? ng : TFM_GRID), dim3(TFM_WG), 0, c->stream, mesh_scene(c), c->meshCount,
                       groupTot);
    hipLaunchKernelGGL(k_mesh_prefix, dim3((ng + TFM_SCAN_GROUPS - 1) / TFM_SCAN_GROUPS), dim3(256), 0, c->stream, c->meshCount,
                       groupTot, c->meshBase, c->n_total);
    return hipGetLastError();
}

// after tfk_mesh_count on the same stream
hipError_t tfk_mesh_emit(tf_ctx* c, float* triangles, long long capacity)
{
    const int ng = mesh_groups(c);
    hipLaunchKernelGGL(k_mesh_emit, dim3(ng < TFM_GRID ? ng : TFM_GRID), dim3(TFM_WG), 0, c->stream, mesh_scene(c), c->meshCount,
                       c->meshBase, triangles, capacity, c->p.voxelSize);
    return hipGetLastError();
}

// after tfk_mesh_count on the same stream: positions (may be nullptr), normals and / or colours (at
// least one of the two; colours need the colour plane), all clipped at the same capacity
hipError_t tfk_mesh_emit_attr(tf_ctx* c, float* triangles, float* normals, unsigned char* colours, long long capacity)
{
    const int ng = mesh_groups(c);
    const dim3 grid(ng < TFM_GRID ? ng : TFM_GRID), wg(TFM_WG);
    unsigned* col = reinterpret_cast<unsigned*>(colours);
    if (normals && colours)
        hipLaunchKernelGGL((k_mesh_emit_attr<true, true>), grid, wg, 0, c->stream, mesh_scene(c), c->vba_rgb_guard, c->meshCount, c->meshBase,
                           triangles, normals, col, capacity, c->p.voxelSize);
    else if (normals)
        hipLaunchKernelGGL((k_mesh_emit_attr<true, false>), grid, wg, 0, c->stream, mesh_scene(c), c->vba_rgb_guard, c->meshCount, c->meshBase,
                           triangles, normals, col, capacity, c->p.voxelSize);
    else
        hipLaunchKernelGGL((k_mesh_emit_attr<false, true>), grid, wg, 0, c->stream, mesh_scene(c), c->vba_rgb_guard, c->meshCount, c->meshBase,
                           triangles, normals, col, capacity, c->p.voxelSize);
    return hipGetLastError();
}

// the exclusive scan alone (tf_mesh_indexed.hip scans its vertex counts with it)
hipError_t tfk_mesh_prefix(tf_ctx* c, const long long* count, const long long* groupTot, long long* base)
{
    const int ng = mesh_groups(c);
    hipLaunchKernelGGL(k_mesh_prefix, dim3((ng + TFM_SCAN_GROUPS - 1) / TFM_SCAN_GROUPS), dim3(256), 0, c->stream, count, groupTot, base,
                       c->n_total);
    return hipGetLastError();
}
