// tf_mesh_ply.cpp -- the PLY writers of mesh extraction (include/tfusion_hip.h: tf_mesh_write_ply,
// tf_mesh_write_ply_attr, tf_mesh_write_ply_indexed).  Host only, no HIP call (also built alone for a
// CPU, under sanitizers, by the tests).  A vertex is a record of 3 (+ 3) (+ 1) dwords -- position, normal,
// RGBA -- and the three writers share one record packer, one welder and one file emitter.
#include "../../include/tfusion_hip.h"

#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

namespace {

struct Columns {
    const float* pos;            // 3 floats per vertex
    const float* nrm;            // 3 floats per vertex, or nullptr
    const uint8_t* col;          // RGBA per vertex, or nullptr
    size_t nw() const { return 3 + (nrm ? 3 : 0) + (col ? 1 : 0); }      // dwords per record
    void pack(size_t i, uint32_t* k) const
    {
        memcpy(k, pos + 3 * i, 12);
        if (nrm) memcpy(k + 3, nrm + 3 * i, 12);
        if (col) memcpy(k + (nrm ? 6 : 3), col + 4 * i, 4);
    }
};

// The nv records welded by the exact bits of the whole record (-0.0f and 0.0f stay apart): verts gets the
// distinct ones in the order of their first appearance, face[i] record i's number among them.  Open
// addressing, slots hold vertex number + 1; the result does not depend on the hash function.
void weld(const Columns& c, size_t nv, std::vector<uint32_t>& verts, std::vector<uint32_t>& face)
{
    const size_t nw = c.nw();
    size_t cap = 16;
    while (cap < nv * 2) cap <<= 1;
    std::vector<int> slot(cap, 0);
    face.resize(nv);
    verts.reserve((nv / 4 + 16) * nw);
    for (size_t i = 0; i < nv; ++i) {
        uint32_t k[7];
        c.pack(i, k);
        size_t h = 0;
        for (size_t j = 0; j < nw; ++j) h = (h ^ k[j]) * 0x9e3779b1u;
        h ^= h >> 15;
        for (h &= cap - 1;; h = (h + 1) & (cap - 1)) {
            if (!slot[h]) { verts.insert(verts.end(), k, k + nw); slot[h] = (int)(verts.size() / nw); break; }
            if (!memcmp(&verts[((size_t)slot[h] - 1) * nw], k, 4 * nw)) break;
        }
        face[i] = (uint32_t)(slot[h] - 1);
    }
}

// binary little-endian PLY: the header with the property lines of the columns present, the vertex
// records, then nt faces of 13 bytes (uchar 3, three int indices)
tf_status emit_ply(const char* path, const Columns& c, const std::vector<uint32_t>& verts, const uint32_t* faces, size_t nt)
{
    std::vector<unsigned char> rec(nt * 13);
    for (size_t i = 0; i < nt; ++i) {
        rec[13 * i] = 3;
        memcpy(&rec[13 * i + 1], faces + 3 * i, 12);
    }
    FILE* f = fopen(path, "wb");
    if (!f) return TF_INVALID_ARG;
    bool ok = fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment topfusion mesh\nelement vertex %zu\n"
                         "property float x\nproperty float y\nproperty float z\n%s%selement face %zu\n"
                         "property list uchar int vertex_indices\nend_header\n", verts.size() / c.nw(),
                      c.nrm ? "property float nx\nproperty float ny\nproperty float nz\n" : "",
                      c.col ? "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n" : "", nt) > 0;
    ok = ok && (verts.empty() || fwrite(verts.data(), 4, verts.size(), f) == verts.size());
    ok = ok && (rec.empty() || fwrite(rec.data(), 1, rec.size(), f) == rec.size());
    ok = (fclose(f) == 0) && ok;
    return ok ? TF_OK : TF_INVALID_ARG;
}

}  // namespace

// vertices welded, faces of int indices in the input order
extern "C" tf_status tf_mesh_write_ply_attr(const char* path, const float* host_triangles, const float* host_normals,
                                            const uint8_t* host_colours, long long n)
{
    if (!path || n < 0 || (n > 0 && !host_triangles) || n > (long long)(INT_MAX / 3)) return TF_INVALID_ARG;
    const Columns c = { host_triangles, host_normals, host_colours };
    try {
        std::vector<uint32_t> verts, face;
        weld(c, (size_t)n * 3, verts, face);
        return emit_ply(path, c, verts, face.data(), (size_t)n);
    } catch (const std::bad_alloc&) { return TF_OOM; }
}

extern "C" tf_status tf_mesh_write_ply(const char* path, const float* host_triangles, long long n)
{
    return tf_mesh_write_ply_attr(path, host_triangles, nullptr, nullptr, n);
}

// the vertex table as given (no welding), then the same faces
extern "C" tf_status tf_mesh_write_ply_indexed(const char* path, const float* host_vertices, const float* host_normals,
                                               const uint8_t* host_colours, long long nv, const uint32_t* host_indices, long long nt)
{
    if (!path || nv < 0 || nt < 0 || (nv > 0 && !host_vertices) || (nt > 0 && !host_indices) || nv > (long long)INT_MAX) return TF_INVALID_ARG;
    for (long long i = 0; i < 3 * nt; ++i)
        if ((long long)host_indices[i] >= nv) return TF_INVALID_ARG;
    const Columns c = { host_vertices, host_normals, host_colours };
    try {
        std::vector<uint32_t> verts((size_t)nv * c.nw());
        for (size_t i = 0; i < (size_t)nv; ++i) c.pack(i, &verts[i * c.nw()]);
        return emit_ply(path, c, verts, host_indices, (size_t)nt);
    } catch (const std::bad_alloc&) { return TF_OOM; }
}
