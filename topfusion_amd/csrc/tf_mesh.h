// tf_mesh.h -- the per-cube part of mesh extraction (DESIGN.md §Mesh extraction): marching tetrahedra on
// the Kuhn split of a voxel cube.  No reference counterpart (the reference has no mesher).  Plain
// functions of eight corner voxels, shared by every kernel of tf_mesh.hip; also compilable as host C++
// (the case rules can then be checked without a GPU).  Each rule is written once: the case table is
// decoded by tfm_tet_emit_edges alone, the six tetrahedra are driven by tfm_cube_emit_edges alone, a
// corner's sdf is selected by tfm_corner_sdf, an edge's weight is tfm_edge_t; positions, attributes
// and indices are emit functors over that walk.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define TFM_HD __host__ __device__ __forceinline__
#define TFM_TABLE static __constant__ const
#define TFM_UNROLL _Pragma("unroll")        // on the three-vertex loops: their small arrays must never be indexed at run time
#else
#define TFM_HD inline
#define TFM_TABLE static constexpr
#define TFM_UNROLL
#endif

// Tetrahedron k of the cube, axis permutation (a, b, c) in the order xyz xzy yxz yzx zxy zyx: corners
// c0 = 0, c1 = e_a, c2 = e_a + e_b, c3 = (1,1,1), as cube corner ids (bit 0 x, bit 1 y, bit 2 z), 3 bits
// each.  det[c1 - c0, c2 - c0, c3 - c0] = det[e_a, e_b, e_c]: the permutation's sign is the
// tetrahedron's handedness.
constexpr unsigned tfm_perm_a(int k) { return (unsigned)(k >> 1); }
constexpr unsigned tfm_perm_b(int k) { return k == 0 ? 1u : k == 1 ? 2u : k == 2 ? 0u : k == 3 ? 2u : k == 4 ? 0u : 1u; }
constexpr unsigned tfm_tet_corners(int k)
{
    return (0u) | ((1u << tfm_perm_a(k)) << 3) | (((1u << tfm_perm_a(k)) | (1u << tfm_perm_b(k))) << 6) | (7u << 9);
}
// odd permutations: xzy, yxz, zyx
constexpr bool tfm_tet_negative(int k) { return k == 1 || k == 2 || k == 5; }

// A case of a tetrahedron, from the inside set m (bit i: corner i has sdf < 0), by rule:
//   bits 0-1  triangles (0, 1, 2)
//   bit  2    swap each triangle's last two vertices in a POSITIVE tetrahedron (a negative one: the opposite)
//   bits 4-19 the vertices v0..v3, 4 bits each: the edge's lower corner | upper corner << 2
// One inside corner i: the edges (i, j), j ascending; the listed order's normal points away from i
// iff (-1)^i det > 0 [(p1 - ci) . ((p2 - p1) x (p3 - p1)) = t1 t2 t3 det[cj1 - ci, cj2 - ci, cj3 - ci], and
// moving ci to the front of (c0..c3) takes i transpositions].  One outside corner i: the same
// vertices, the normal must point towards i.  Two and two (i < j inside, k < l outside): the quad
// v_ik v_il v_jl v_jk; at the edge midpoints its normal is (cl - ck) x (cj - ci) / 4 and n . (outside
// centroid - inside centroid) = det[cj - ci, ck - ci, cl - ci] / 4, so the listed order is right iff
// the permutation (i, j, k, l) is even (times the handedness).
constexpr unsigned tfm_edge(int u, int v) { return u < v ? (unsigned)(u | v << 2) : (unsigned)(v | u << 2); }
constexpr int tfm_popc4(unsigned m) { return (int)((m & 1) + (m >> 1 & 1) + (m >> 2 & 1) + (m >> 3 & 1)); }
constexpr int tfm_nth_set(unsigned m, int n)    // index of the n-th set bit of m (n from 0)
{
    return (m & 1) ? (n == 0 ? 0 : 1 + tfm_nth_set(m >> 1, n - 1)) : 1 + tfm_nth_set(m >> 1, n);
}
constexpr int tfm_inversions(int a, int b, int c, int d)
{
    return (a > b) + (a > c) + (a > d) + (b > c) + (b > d) + (c > d);
}
constexpr unsigned tfm_case(unsigned m)
{
    const int n = tfm_popc4(m);
    if (n == 0 || n == 4) return 0u;
    if (n == 1 || n == 3) {
        const unsigned one = n == 1 ? m : (~m & 15u), rest = ~one & 15u;
        const int i = tfm_nth_set(one, 0);
        const unsigned v = tfm_edge(i, tfm_nth_set(rest, 0)) | tfm_edge(i, tfm_nth_set(rest, 1)) << 4 |
                           tfm_edge(i, tfm_nth_set(rest, 2)) << 8;
        const bool ok_pos = n == 1 ? (i % 2 == 0) : (i % 2 == 1);
        return 1u | (ok_pos ? 0u : 4u) | v << 4;
    }
    const unsigned out = ~m & 15u;
    const int i = tfm_nth_set(m, 0), j = tfm_nth_set(m, 1), k = tfm_nth_set(out, 0), l = tfm_nth_set(out, 1);
    const unsigned v = tfm_edge(i, k) | tfm_edge(i, l) << 4 | tfm_edge(j, l) << 8 | tfm_edge(j, k) << 12;
    return 2u | (tfm_inversions(i, j, k, l) % 2 == 0 ? 0u : 4u) | v << 4;
}
TFM_TABLE unsigned tfm_cases[16] = { tfm_case(0), tfm_case(1), tfm_case(2), tfm_case(3), tfm_case(4), tfm_case(5),
                                     tfm_case(6), tfm_case(7), tfm_case(8), tfm_case(9), tfm_case(10), tfm_case(11),
                                     tfm_case(12), tfm_case(13), tfm_case(14), tfm_case(15) };

// triangles of a 4-bit case: 0 for none / all inside, 2 for two and two, else 1
TFM_HD int tfm_case_tris(unsigned m)
{
    // 2 bits per case, from the rule: |S| = 1, 3 -> 1; |S| = 2 -> 2
    constexpr unsigned long long packed =
        (unsigned long long)(tfm_case(0) & 3) | (unsigned long long)(tfm_case(1) & 3) << 2 | (unsigned long long)(tfm_case(2) & 3) << 4 |
        (unsigned long long)(tfm_case(3) & 3) << 6 | (unsigned long long)(tfm_case(4) & 3) << 8 | (unsigned long long)(tfm_case(5) & 3) << 10 |
        (unsigned long long)(tfm_case(6) & 3) << 12 | (unsigned long long)(tfm_case(7) & 3) << 14 | (unsigned long long)(tfm_case(8) & 3) << 16 |
        (unsigned long long)(tfm_case(9) & 3) << 18 | (unsigned long long)(tfm_case(10) & 3) << 20 | (unsigned long long)(tfm_case(11) & 3) << 22 |
        (unsigned long long)(tfm_case(12) & 3) << 24 | (unsigned long long)(tfm_case(13) & 3) << 26 | (unsigned long long)(tfm_case(14) & 3) << 28 |
        (unsigned long long)(tfm_case(15) & 3) << 30;
    return (int)(packed >> (2 * m) & 3);
}

// The cube's eight corner voxels, corner id = dx | dy << 1 | dz << 2: sdf shorts and "all eight exist
// with w > 0".
struct TfmCube {
    int sdf[8];
    bool valid;
};

// the case of tetrahedron K from the cube's 8-bit inside mask (bit = corner id)
template <int K>
TFM_HD unsigned tfm_tet_case(unsigned inside8)
{
    constexpr unsigned c = tfm_tet_corners(K);
    return (inside8 >> (c & 7) & 1) | (inside8 >> (c >> 3 & 7) & 1) << 1 | (inside8 >> (c >> 6 & 7) & 1) << 2 |
           (inside8 >> (c >> 9 & 7) & 1) << 3;
}
TFM_HD unsigned tfm_inside_mask(const TfmCube& q)
{
    unsigned m = 0;
    for (int i = 0; i < 8; ++i) m |= (q.sdf[i] < 0 ? 1u : 0u) << i;
    return m;
}
// triangles of the cube
TFM_HD int tfm_cube_count(const TfmCube& q)
{
    if (!q.valid) return 0;
    const unsigned m = tfm_inside_mask(q);
    return tfm_case_tris(tfm_tet_case<0>(m)) + tfm_case_tris(tfm_tet_case<1>(m)) + tfm_case_tris(tfm_tet_case<2>(m)) +
           tfm_case_tris(tfm_tet_case<3>(m)) + tfm_case_tris(tfm_tet_case<4>(m)) + tfm_case_tris(tfm_tet_case<5>(m));
}

// ---- the triangle walk (the only decoder of tfm_cases) ------------------------------------------------
// Tetrahedron K's triangles through emit(const unsigned lo[3], const unsigned hi[3]) -- per triangle
// vertex the cube corners its edge joins (lo a subset of hi) -- in case order; returns their number.
// Every emission (positions, attributes, indices) is a functor over this walk.
template <int K, class Emit>
TFM_HD int tfm_tet_emit_edges(unsigned inside8, Emit& emit)
{
    constexpr unsigned corners = tfm_tet_corners(K);
    const unsigned info = tfm_cases[tfm_tet_case<K>(inside8)];
    const int n = (int)(info & 3);
    const bool flip = ((info >> 2 & 1) != 0) != tfm_tet_negative(K);
    for (int tr = 0; tr < n; ++tr) {
        unsigned lo[3], hi[3];
        TFM_UNROLL               // (lo / hi stay registers only while v is a constant)
        for (int v = 0; v < 3; ++v) {
            // triangle 0: v0 v1 v2, triangle 1: v0 v2 v3; flipped: the last two swapped
            const int w = v == 0 ? 0 : (flip ? 3 - v : v) + tr;
            const unsigned e = info >> (4 + 4 * w) & 15u;
            lo[v] = corners >> (3 * (e & 3)) & 7u;
            hi[v] = corners >> (3 * (e >> 2)) & 7u;
        }
        emit(lo, hi);
    }
    return n;
}

// the six tetrahedra of a cube; 0 triangles when the cube is not valid
template <class Emit>
TFM_HD int tfm_cube_emit_edges(const TfmCube& q, Emit& emit)
{
    if (!q.valid) return 0;
    const unsigned m = tfm_inside_mask(q);
    int n = tfm_tet_emit_edges<0>(m, emit);
    n += tfm_tet_emit_edges<1>(m, emit);
    n += tfm_tet_emit_edges<2>(m, emit);
    n += tfm_tet_emit_edges<3>(m, emit);
    n += tfm_tet_emit_edges<4>(m, emit);
    n += tfm_tet_emit_edges<5>(m, emit);
    return n;
}

// The sdf at the cube corners lo and hi (0 .. 7, run-time values) by select chains: q.sdf[] is never
// indexed with a run-time value, so it stays in registers.  (Both chains read each q.sdf[i] once, in one
// loop: a load with a single select behind it is what a compiler turns back into an indexed load.)
TFM_HD void tfm_corner_sdf(const TfmCube& q, unsigned lo, unsigned hi, int& sp, int& sq)
{
    sp = sq = q.sdf[0];
    for (int i = 1; i < 8; ++i) { sp = lo == (unsigned)i ? q.sdf[i] : sp; sq = hi == (unsigned)i ? q.sdf[i] : sq; }
}

// the interpolation weight of an edge whose ends have the sdf sp and sq (the difference in int, exact in
// float): the one float that places the vertex and weighs its attributes
TFM_HD float tfm_edge_t(int sp, int sq) { return (float)sp / (float)(sp - sq); }

// The vertex on the edge from the cube corner `lo` (sdf sp, global voxel gx, gy, gz of the cube's
// corner 0) to `hi` (sdf sq): t = tfm_edge_t, then per axis RN(RN(g + t) * voxelSize) where the edge
// moves, RN(g * voxelSize) where it does not.  Both cubes (and all tetrahedra) that share the edge
// compute the same three floats.
TFM_HD void tfm_vertex(unsigned lo, unsigned hi, int sp, int sq, int gx, int gy, int gz, float vs, float* out)
{
    const float t = tfm_edge_t(sp, sq);
    const unsigned d = hi & ~lo;
    const float px = (float)(gx + (int)(lo & 1)), py = (float)(gy + (int)(lo >> 1 & 1)), pz = (float)(gz + (int)(lo >> 2 & 1));
    const float ax = px + t, ay = py + t, az = pz + t;
    out[0] = ((d & 1) ? ax : px) * vs;
    out[1] = ((d & 2) ? ay : py) * vs;
    out[2] = ((d & 4) ? az : pz) * vs;
}

// ---- per-vertex attributes (DESIGN.md §Mesh extraction, attributes) ---------------------------------
// A vertex lies on the edge from the lattice voxel p (the cube corner `lo`) to q (`hi`); its normal and
// colour are functions of the edge alone (t, and the gradients / colour words at p and q), so every
// cube and tetrahedron that shares the edge computes the same bits.

// One axis of the integer gradient at a voxel with sdf s0: sm / sp the sdf of the voxel one step down
// / up the axis, um / up whether that voxel is usable (its block in the hash with ptr >= 0, w > 0).
// Central where both are, one-sided and doubled where one is, 0 where neither is.  |result| <= 131070.
TFM_HD int tfm_grad_axis(int sm, int s0, int sp, bool um, bool up)
{
    return um ? (up ? sp - sm : 2 * (s0 - sm)) : (up ? 2 * (sp - s0) : 0);
}

// the same from packed voxels (sdf | w << 16, as the kernels stage them)
TFM_HD int tfm_grad_axis_packed(unsigned vm, unsigned v0, unsigned vp)
{
    return tfm_grad_axis((int)(short)(vm & 0xffffu), (int)(short)(v0 & 0xffffu), (int)(short)(vp & 0xffffu), (vm >> 16) != 0,
                         (vp >> 16) != 0);
}

// N_a = RN(Gp_a + RN(t (Gq_a - Gp_a))) (the difference in int, exact in float), normalised by
// L = sqrt(RN(RN(Nx Nx + Ny Ny) + Nz Nz)) with IEEE sqrt and division; (0, 0, 0) when L == 0
TFM_HD void tfm_normal(float t, const int* gp, const int* gq, float* out)
{
    const float nx = (float)gp[0] + t * (float)(gq[0] - gp[0]);
    const float ny = (float)gp[1] + t * (float)(gq[1] - gp[1]);
    const float nz = (float)gp[2] + t * (float)(gq[2] - gp[2]);
    const float l2 = (nx * nx + ny * ny) + nz * nz;
    const float l = sqrtf(l2);
    const bool zero = l == 0.0f;
    out[0] = zero ? 0.0f : nx / l;
    out[1] = zero ? 0.0f : ny / l;
    out[2] = zero ? 0.0f : nz / l;
}

// one channel: RN(cp + RN(t (cq - cp))), then + 0.5 and truncated (the value lies in [0, 255])
TFM_HD unsigned tfm_colour_channel(float t, int cp, int cq)
{
    const float f = (float)cp + t * (float)(cq - cp);
    return (unsigned)(unsigned char)(int)(f + 0.5f);
}

// The vertex's RGBA (r | g << 8 | b << 16 | a << 24) from the colour words of the edge's ends
// (r | g << 8 | b << 16 | w_color << 24; an unusable end is passed as 0).  An end has colour when its
// w_color > 0: both -> interpolated channels, one -> that end's, none -> 0; alpha 255 unless none.
TFM_HD unsigned tfm_colour(float t, unsigned wp, unsigned wq)
{
    const bool hp = (wp >> 24) != 0, hq = (wq >> 24) != 0;
    if (hp && hq) {
        return tfm_colour_channel(t, (int)(wp & 255u), (int)(wq & 255u)) |
               tfm_colour_channel(t, (int)(wp >> 8 & 255u), (int)(wq >> 8 & 255u)) << 8 |
               tfm_colour_channel(t, (int)(wp >> 16 & 255u), (int)(wq >> 16 & 255u)) << 16 | 0xff000000u;
    }
    if (hp) return (wp & 0xffffffu) | 0xff000000u;
    if (hq) return (wq & 0xffffffu) | 0xff000000u;
    return 0u;
}

// ---- triangles as floats: an emit functor over the edge walk --------------------------------------------
// Src gives the lattice data at a cube corner (0 .. 7):
//   static constexpr bool normals, colours;  void grad(unsigned corner, int g[3]) const;
//   unsigned colour(unsigned corner) const
// and emit receives (const float tri[9], const float nrm[9], const unsigned rgba[3]); what Src does not
// provide is passed as zeros.  TfmNoAttr provides nothing: positions only.
struct TfmNoAttr {
    static constexpr bool normals = false, colours = false;
    TFM_HD void grad(unsigned, int*) const {}
    TFM_HD unsigned colour(unsigned) const { return 0u; }
};

template <class Src, class Emit>
struct TfmVertexEmit {
    const TfmCube& q;
    int gx, gy, gz;              // the global voxel of the cube's corner 0
    float vs;
    const Src& src;
    Emit& emit;
    TFM_HD void operator()(const unsigned* lo, const unsigned* hi)
    {
        float tri[9], nrm[9];
        unsigned rgba[3];
        TFM_UNROLL               // (a rolled loop indexes tri / nrm / rgba with a run-time value: they leave the registers)
        for (int v = 0; v < 3; ++v) {
            int sp, sq;
            tfm_corner_sdf(q, lo[v], hi[v], sp, sq);
            tfm_vertex(lo[v], hi[v], sp, sq, gx, gy, gz, vs, tri + 3 * v);
            const float t = tfm_edge_t(sp, sq);
            if (Src::normals) {
                int gp[3], gq[3];
                src.grad(lo[v], gp);
                src.grad(hi[v], gq);
                tfm_normal(t, gp, gq, nrm + 3 * v);
            } else {
                nrm[3 * v] = nrm[3 * v + 1] = nrm[3 * v + 2] = 0.0f;
            }
            rgba[v] = Src::colours ? tfm_colour(t, src.colour(lo[v]), src.colour(hi[v])) : 0u;
        }
        emit(tri, nrm, rgba);
    }
};

// the cube's triangles with Src's attributes; order and count are tfm_cube_emit_edges'
template <class Src, class Emit>
TFM_HD int tfm_cube_emit_attr(const TfmCube& q, int gx, int gy, int gz, float vs, const Src& src, Emit& emit)
{
    TfmVertexEmit<Src, Emit> ve = { q, gx, gy, gz, vs, src, emit };
    return tfm_cube_emit_edges(q, ve);
}

// ---- indexed extraction (DESIGN.md §Mesh extraction, indexed) ----------------------------------------
// A vertex IS its Kuhn edge (p, d): p the edge's lower end (a lattice voxel), d in {0,1}^3 \ {0} with the
// direction code dc = dx | dy << 1 | dz << 2.  The edge belongs to the block of p (its owner); inside the
// owner it is bit lp * 7 + dc - 1 of a 512 x 7-bit mask (lp = p's voxel index x + 8 y + 64 z), and its
// vertex number is the owner's base plus the number of set bits below it.
#define TFM_EDGE_WORDS 112       // 512 * 7 / 32

struct TfmEdgeRef {
    unsigned owner;              // which of the entry's eight blocks holds p: (px >> 3) | (py >> 3) << 1 | (pz >> 3) << 2
    unsigned bit;                // the edge's bit in the owner's mask
};

TFM_HD unsigned tfm_edge_bit(unsigned lp, unsigned dc) { return lp * 7u + dc - 1u; }

// the edge whose lower end is the lattice point (px, py, pz) of an entry's tile, 0 .. 8 each
TFM_HD TfmEdgeRef tfm_edge_ref(int px, int py, int pz, unsigned dc)
{
    TfmEdgeRef r;
    r.owner = (unsigned)((px >> 3) | (py >> 3) << 1 | (pz >> 3) << 2);
    r.bit = tfm_edge_bit((unsigned)((px & 7) | (py & 7) << 3 | (pz & 7) << 6), dc);
    return r;
}

// the edge's rank inside its owner from the mask word that holds its bit and that word's exclusive
// popcount prefix
TFM_HD unsigned tfm_edge_rank(unsigned word, unsigned prefix, unsigned bit)
{
    return prefix + (unsigned)__builtin_popcount(word & ((1u << (bit & 31u)) - 1u));
}

// The sign-changing Kuhn edges of the cube whose corner 0 is the tile's lattice point (x, y, z), 0 .. 7
// each, through mark(TfmEdgeRef): the 19 corner pairs lo, hi = lo | dc with lo & dc == 0.  Each is an
// edge of one of the six tetrahedra at least, and a tetrahedron puts a triangle vertex on every edge
// of its own whose ends differ, so these are exactly the edges tfm_cube_emit_edges' triangles touch.
template <class Mark>
TFM_HD void tfm_cube_mark(const TfmCube& q, int x, int y, int z, Mark& mark)
{
    if (!q.valid) return;
    const unsigned m = tfm_inside_mask(q);
    if (m == 0u || m == 255u) return;
    for (unsigned lo = 0; lo < 7; ++lo)
        for (unsigned dc = 1; dc < 8; ++dc) {
            if (lo & dc) continue;
            if (((m >> lo) ^ (m >> (lo | dc))) & 1u) mark(tfm_edge_ref(x + (int)(lo & 1), y + (int)(lo >> 1 & 1), z + (int)(lo >> 2), dc));
        }
}


// The vertex of the edge (p, dc) from its lower end: p's global voxel coordinate, the sdf shorts at p and
// q = p + d.  tfm_vertex with the cube's corner 0 at p, so the bits every cube sharing the edge computes.
TFM_HD void tfm_edge_vertex(unsigned dc, int sp, int sq, int px, int py, int pz, float vs, float* out)
{
    tfm_vertex(0u, dc, sp, sq, px, py, pz, vs, out);
}