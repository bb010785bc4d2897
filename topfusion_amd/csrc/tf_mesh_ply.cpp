// tf_mesh_ply.cpp -- the PLY writers of mesh extraction (include/tfusion_hip.h: tf_mesh_write_ply,
// tf_mesh_write_ply_attr, tf_mesh_write_ply_indexed).  Host only, no HIP call (also built alone for a
// CPU, under sanitizers, by the tests).  A vertex is a record of 3 (+ 3) (+ 1) dwords -- position, normal,
// RGBA -- and the three writers share one record packer, one welder and one file emitter: the streaming
// writer (tf_mesh_ply_begin / _vertices / _faces / _end), which takes the vertices and the faces in pieces
// and is what tf_mesh_save_ply_indexed_whole feeds chunk by chunk.  The one-call writers are callers of it.
#include "../../include/tfusion_hip.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
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

}  // namespace

// ---- the streaming writer: the one place the file's format stands ------------------------------------------
// binary little-endian PLY: the header with the property lines of the columns present, nv vertex records of
// 3 (+ 3) (+ 1) dwords, then nt faces of 13 bytes (uchar 3, three int indices).  Records are packed through a
// fixed buffer, so the writer's memory does not grow with the mesh.
struct tf_ply_stream {
    FILE* f;
    char* path;                  // (removed on a failure)
    long long nv, nt;            // as declared in the header
    long long vdone, fdone;
    bool nrm, col, ok;
    unsigned char buf[1 << 16];
    size_t nw() const { return 3 + (nrm ? 3 : 0) + (col ? 1 : 0); }
    bool put(size_t bytes) { return ok = ok && fwrite(buf, 1, bytes, f) == bytes; }
};

namespace {

// n records already packed (nw dwords each)
tf_status ply_records(tf_ply_stream* s, const uint32_t* rec, long long n)
{
    if (!s->ok || n < 0 || s->fdone > 0 || n > s->nv - s->vdone) { s->ok = false; return TF_INVALID_ARG; }
    const size_t words = (size_t)n * s->nw();
    s->ok = words == 0 || fwrite(rec, 4, words, s->f) == words;
    s->vdone += n;
    return s->ok ? TF_OK : TF_INVALID_ARG;
}

}  // namespace

extern "C" tf_status tf_mesh_ply_begin(const char* path, long long nv, long long nt, int attrs, tf_ply_stream** out)
{
    if (out) *out = nullptr;
    if (!path || !out || nv < 0 || nt < 0 || nv > (long long)INT_MAX || (attrs & ~(TF_MESH_NORMALS | TF_MESH_COLOURS))) return TF_INVALID_ARG;
    tf_ply_stream* s = new (std::nothrow) tf_ply_stream;
    char* name = s ? (char*)malloc(strlen(path) + 1) : nullptr;
    if (!name) { delete s; return TF_OOM; }
    strcpy(name, path);
    s->path = name;
    s->nv = nv; s->nt = nt; s->vdone = s->fdone = 0;
    s->nrm = attrs & TF_MESH_NORMALS; s->col = attrs & TF_MESH_COLOURS;
    s->f = fopen(path, "wb");
    if (!s->f) { free(name); delete s; return TF_INVALID_ARG; }
    s->ok = fprintf(s->f, "ply\nformat binary_little_endian 1.0\ncomment topfusion mesh\nelement vertex %lld\n"
                          "property float x\nproperty float y\nproperty float z\n%s%selement face %lld\n"
                          "property list uchar int vertex_indices\nend_header\n", nv,
                    s->nrm ? "property float nx\nproperty float ny\nproperty float nz\n" : "",
                    s->col ? "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n" : "", nt) > 0;
    *out = s;
    return TF_OK;                // (a header that could not be written fails the first append, or the end)
}

extern "C" tf_status tf_mesh_ply_vertices(tf_ply_stream* s, const float* pos, const float* nrm, const uint8_t* col, long long n)
{
    if (!s) return TF_INVALID_ARG;
    if (!s->ok || n < 0 || s->fdone > 0 || n > s->nv - s->vdone || (n > 0 && (!pos || (s->nrm && !nrm) || (s->col && !col)))) {
        s->ok = false;
        return TF_INVALID_ARG;
    }
    const Columns c = { pos, s->nrm ? nrm : nullptr, s->col ? col : nullptr };
    const size_t nw = s->nw(), per = sizeof s->buf / (4 * nw);
    for (size_t i0 = 0; i0 < (size_t)n && s->ok; i0 += per) {
        const size_t k = (size_t)n - i0 < per ? (size_t)n - i0 : per;
        for (size_t i = 0; i < k; ++i) {
            uint32_t rec[7];
            c.pack(i0 + i, rec);
            memcpy(s->buf + 4 * nw * i, rec, 4 * nw);
        }
        s->put(4 * nw * k);
    }
    s->vdone += n;
    return s->ok ? TF_OK : TF_INVALID_ARG;
}

extern "C" tf_status tf_mesh_ply_faces(tf_ply_stream* s, const uint32_t* indices, long long n)
{
    if (!s) return TF_INVALID_ARG;
    if (!s->ok || n < 0 || s->vdone != s->nv || n > s->nt - s->fdone || (n > 0 && !indices)) { s->ok = false; return TF_INVALID_ARG; }
    const size_t per = sizeof s->buf / 13;
    for (size_t i0 = 0; i0 < (size_t)n && s->ok; i0 += per) {
        const size_t k = (size_t)n - i0 < per ? (size_t)n - i0 : per;
        for (size_t i = 0; i < k; ++i) {
            const uint32_t* tri = indices + 3 * (i0 + i);
            if ((long long)tri[0] >= s->nv || (long long)tri[1] >= s->nv || (long long)tri[2] >= s->nv) s->ok = false;
            s->buf[13 * i] = 3;
            memcpy(s->buf + 13 * i + 1, tri, 12);
        }
        s->put(13 * k);
    }
    s->fdone += n;
    return s->ok ? TF_OK : TF_INVALID_ARG;
}

extern "C" tf_status tf_mesh_ply_end(tf_ply_stream* s, int commit)
{
    if (!s) return TF_INVALID_ARG;
    bool ok = commit && s->ok && s->vdone == s->nv && s->fdone == s->nt;
    ok = (fclose(s->f) == 0) && ok;
    if (!ok) remove(s->path);
    const bool quiet = !commit;
    free(s->path);
    delete s;
    return ok || quiet ? TF_OK : TF_INVALID_ARG;
}

namespace {

// the welded writers' file: records already packed, faces as given
tf_status emit_ply(const char* path, const Columns& c, const std::vector<uint32_t>& verts, const uint32_t* faces, size_t nt)
{
    tf_ply_stream* s = nullptr;
    const tf_status b = tf_mesh_ply_begin(path, (long long)(verts.size() / c.nw()), (long long)nt,
                                          (c.nrm ? TF_MESH_NORMALS : 0) | (c.col ? TF_MESH_COLOURS : 0), &s);
    if (b != TF_OK) return b;
    ply_records(s, verts.data(), (long long)(verts.size() / c.nw()));
    tf_mesh_ply_faces(s, faces, (long long)nt);
    return tf_mesh_ply_end(s, 1);
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

// the vertex table as given (no welding), then the same faces: the streaming writer in one piece
extern "C" tf_status tf_mesh_write_ply_indexed(const char* path, const float* host_vertices, const float* host_normals,
                                               const uint8_t* host_colours, long long nv, const uint32_t* host_indices, long long nt)
{
    if (!path || nv < 0 || nt < 0 || (nv > 0 && !host_vertices) || (nt > 0 && !host_indices) || nv > (long long)INT_MAX) return TF_INVALID_ARG;
    for (long long i = 0; i < 3 * nt; ++i)              // (before the file is touched: whatever lay at path survives bad input)
        if ((long long)host_indices[i] >= nv) return TF_INVALID_ARG;
    tf_ply_stream* s = nullptr;
    const tf_status b = tf_mesh_ply_begin(path, nv, nt, (host_normals ? TF_MESH_NORMALS : 0) | (host_colours ? TF_MESH_COLOURS : 0), &s);
    if (b != TF_OK) return b;
    tf_mesh_ply_vertices(s, host_vertices, host_normals, host_colours, nv);
    tf_mesh_ply_faces(s, host_indices, nt);
    return tf_mesh_ply_end(s, 1);
}
