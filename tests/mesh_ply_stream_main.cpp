// mesh_ply_stream_main.cpp -- drives the streaming PLY writer (tf_mesh_ply_begin / _vertices / _faces / _end,
// topfusion_amd/csrc/tf_mesh_ply.cpp) in one process; tests/test_mesh_indexed_whole_ref.py builds it for the CPU
// with -fsanitize=address,undefined.  Every piece is handed over in a heap buffer of exactly its size, so a
// read past the end of a chunk is a sanitizer report.
//
//   mesh_ply_stream_main DIR
//
// One vertex table (positions, normals, colours; more records than the writer's record buffer holds) and one
// index buffer, written by tf_mesh_write_ply_indexed and by the stream in chunks of 1 record, of 7 (a ragged
// last chunk), of 4096 (several buffer fills, ragged) and of everything, for every column combination: every
// stream file must equal the one-call file byte for byte.  Then nv = 0 (with and without faces declared), an
// out-of-range index in the last chunk, too many / too few records, faces before the vertices are complete, a
// missing column, the give-up end and the argument checks: each refused, and no file left.
// Prints "ok <files> compared, <calls> rejected" and returns 0 when all of that holds.
#include "../include/tfusion_hip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

static int g_compared = 0, g_rejected = 0, g_failures = 0;

static void fail(const char* what, long a)
{
    ++g_failures;
    fprintf(stderr, "failed: %s %ld\n", what, a);
}

// a heap copy of exactly n elements from p (a distinct non-null pointer even when empty)
template <class T>
static T* exact(const T* p, size_t n)
{
    T* q = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    if (!q) abort();
    if (n) memcpy(q, p, n * sizeof(T));
    return q;
}

static uint32_t g_rng = 2463534242u;
static uint32_t rnd(uint32_t n)
{
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

static bool slurp(const std::string& path, std::vector<unsigned char>& buf)
{
    buf.clear();
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    unsigned char chunk[4096];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    fclose(f);
    return true;
}

static bool exists(const std::string& path)
{
    if (FILE* f = fopen(path.c_str(), "rb")) { fclose(f); return true; }
    return false;
}

struct Mesh {
    std::vector<float> pos, nrm;
    std::vector<uint8_t> col;
    std::vector<uint32_t> idx;
    size_t nv() const { return pos.size() / 3; }
    size_t nt() const { return idx.size() / 3; }
};

// the mesh through the stream, `vchunk` vertices and `fchunk` faces per call; every chunk an exact heap copy
static tf_status stream(const std::string& path, const Mesh& m, int attrs, size_t vchunk, size_t fchunk)
{
    tf_ply_stream* s = nullptr;
    tf_status st = tf_mesh_ply_begin(path.c_str(), (long long)m.nv(), (long long)m.nt(), attrs, &s);
    if (st != TF_OK) return st;
    for (size_t v0 = 0; v0 < m.nv() && st == TF_OK; v0 += vchunk) {
        const size_t k = m.nv() - v0 < vchunk ? m.nv() - v0 : vchunk;
        float* p = exact(&m.pos[3 * v0], 3 * k);
        float* n = (attrs & TF_MESH_NORMALS) ? exact(&m.nrm[3 * v0], 3 * k) : nullptr;
        uint8_t* c = (attrs & TF_MESH_COLOURS) ? exact(&m.col[4 * v0], 4 * k) : nullptr;
        st = tf_mesh_ply_vertices(s, p, n, c, (long long)k);
        free(p); free(n); free(c);
    }
    for (size_t t0 = 0; t0 < m.nt() && st == TF_OK; t0 += fchunk) {
        const size_t k = m.nt() - t0 < fchunk ? m.nt() - t0 : fchunk;
        uint32_t* i = exact(&m.idx[3 * t0], 3 * k);
        st = tf_mesh_ply_faces(s, i, (long long)k);
        free(i);
    }
    const tf_status e = tf_mesh_ply_end(s, 1);
    return st == TF_OK ? e : st;
}

static void expect_rejected(tf_status s, const std::string& path, const char* what)
{
    ++g_rejected;
    if (s != TF_INVALID_ARG) fail(what, (long)s);
    if (exists(path)) { fail("a refused stream left a file:", g_rejected); remove(path.c_str()); }
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage\n"); return 2; }
    const std::string dir = std::string(argv[1]) + "/";

    // 9001 vertices and 12345 faces: the writer's record buffer (64 KiB) fills several times in one call
    Mesh m;
    const size_t nv = 9001, nt = 12345;
    m.pos.resize(nv * 3); m.nrm.resize(nv * 3); m.col.resize(nv * 4); m.idx.resize(nt * 3);
    for (float& v : m.pos) v = (float)rnd(100000) * 0.001f - 50.0f;
    for (float& v : m.nrm) v = (float)rnd(3) - 1.0f;
    for (uint8_t& v : m.col) v = (uint8_t)rnd(256);
    for (uint32_t& v : m.idx) v = rnd((uint32_t)nv);
    m.idx[0] = (uint32_t)nv - 1;
    m.idx[m.idx.size() - 1] = (uint32_t)nv - 1;

    const size_t chunks[4][2] = { { 1, 1 }, { 7, 7 }, { 4096, 5000 }, { nv, nt } };
    for (int k = 0; k < 4; ++k) {
        const int attrs = ((k & 1) ? TF_MESH_NORMALS : 0) | ((k & 2) ? TF_MESH_COLOURS : 0);
        const std::string one = dir + "one" + std::to_string(k) + ".ply";
        float* p = exact(m.pos.data(), m.pos.size());
        float* n = exact(m.nrm.data(), m.nrm.size());
        uint8_t* c = exact(m.col.data(), m.col.size());
        uint32_t* i = exact(m.idx.data(), m.idx.size());
        if (tf_mesh_write_ply_indexed(one.c_str(), p, (k & 1) ? n : nullptr, (k & 2) ? c : nullptr, (long long)nv, i, (long long)nt) != TF_OK)
            fail("tf_mesh_write_ply_indexed", k);
        free(p); free(n); free(c); free(i);
        std::vector<unsigned char> want, got;
        if (!slurp(one, want)) fail("one-call file", k);
        for (int q = 0; q < 4; ++q) {
            if (k != 1 && q == 0) continue;             // (1 record per call: once, with normals, is enough)
            const std::string path = dir + "stream" + std::to_string(k) + "_" + std::to_string(q) + ".ply";
            if (stream(path, m, attrs, chunks[q][0], chunks[q][1]) != TF_OK) fail("stream", k * 10 + q);
            ++g_compared;
            if (!slurp(path, got) || got != want) fail("stream file differs from the one-call file", k * 10 + q);
        }
    }

    // nv = 0: an empty mesh with and without a declared normal column; equal to the one-call writer's
    {
        Mesh e;
        const float none = 0.0f;
        std::vector<unsigned char> want, got;
        for (int k = 0; k < 2; ++k) {
            const std::string one = dir + "empty_one" + std::to_string(k) + ".ply", st = dir + "empty_stream" + std::to_string(k) + ".ply";
            if (tf_mesh_write_ply_indexed(one.c_str(), nullptr, k ? &none : nullptr, nullptr, 0, nullptr, 0) != TF_OK) fail("empty one-call", k);
            if (stream(st, e, k ? TF_MESH_NORMALS : 0, 1, 1) != TF_OK) fail("empty stream", k);
            ++g_compared;
            if (!slurp(one, want) || !slurp(st, got) || got != want) fail("empty stream file differs", k);
        }
        // ... and an empty append in the middle of a full mesh changes nothing
        tf_ply_stream* s = nullptr;
        const std::string path = dir + "empty_append.ply", one = dir + "one0.ply";
        if (tf_mesh_ply_begin(path.c_str(), (long long)nv, (long long)nt, 0, &s) != TF_OK) fail("begin", 0);
        if (tf_mesh_ply_vertices(s, nullptr, nullptr, nullptr, 0) != TF_OK) fail("empty vertex append", 0);
        if (tf_mesh_ply_vertices(s, m.pos.data(), nullptr, nullptr, (long long)nv) != TF_OK) fail("vertex append", 0);
        if (tf_mesh_ply_faces(s, nullptr, 0) != TF_OK) fail("empty face append", 0);
        if (tf_mesh_ply_faces(s, m.idx.data(), (long long)nt) != TF_OK) fail("face append", 0);
        if (tf_mesh_ply_end(s, 1) != TF_OK) fail("end", 0);
        ++g_compared;
        if (!slurp(one, want) || !slurp(path, got) || got != want) fail("empty appends changed the file", 0);
        // faces into an empty table
        Mesh f;
        f.idx = { 0, 0, 0 };
        expect_rejected(stream(dir + "bad.ply", f, 0, 1, 1), dir + "bad.ply", "an index into an empty table");
    }

    // refused, and no file left
    const std::string bad = dir + "bad.ply";
    {
        Mesh b = m;
        b.idx[b.idx.size() - 2] = (uint32_t)nv;         // in the last chunk, whatever the chunk size
        expect_rejected(stream(bad, b, TF_MESH_NORMALS, 4096, 5000), bad, "index == nv in a late chunk");
        expect_rejected(stream(bad, b, 0, 1, 1), bad, "index == nv in the last record");
        b.idx[b.idx.size() - 2] = 0xffffffffu;
        expect_rejected(stream(bad, b, 0, nv, nt), bad, "index 2^32 - 1");
    }
    {
        tf_ply_stream* s = nullptr;
        // more vertices than declared
        if (tf_mesh_ply_begin(bad.c_str(), 10, 1, 0, &s) != TF_OK) fail("begin", 1);
        if (tf_mesh_ply_vertices(s, m.pos.data(), nullptr, nullptr, 11) != TF_INVALID_ARG) fail("11 of 10 vertices", 0);
        if (tf_mesh_ply_faces(s, m.idx.data(), 0) != TF_INVALID_ARG) fail("an append after a failure", 0);
        expect_rejected(tf_mesh_ply_end(s, 1), bad, "too many vertices");
        // faces before the vertices are complete
        if (tf_mesh_ply_begin(bad.c_str(), 10, 1, 0, &s) != TF_OK) fail("begin", 2);
        tf_mesh_ply_vertices(s, m.pos.data(), nullptr, nullptr, 9);
        const uint32_t tri[3] = { 0, 1, 2 };
        if (tf_mesh_ply_faces(s, tri, 1) != TF_INVALID_ARG) fail("faces before the last vertex", 0);
        expect_rejected(tf_mesh_ply_end(s, 1), bad, "faces too early");
        // fewer faces than declared
        if (tf_mesh_ply_begin(bad.c_str(), 10, 2, 0, &s) != TF_OK) fail("begin", 3);
        tf_mesh_ply_vertices(s, m.pos.data(), nullptr, nullptr, 10);
        tf_mesh_ply_faces(s, tri, 1);
        expect_rejected(tf_mesh_ply_end(s, 1), bad, "too few faces");
        // more faces than declared
        if (tf_mesh_ply_begin(bad.c_str(), 10, 1, 0, &s) != TF_OK) fail("begin", 4);
        tf_mesh_ply_vertices(s, m.pos.data(), nullptr, nullptr, 10);
        const uint32_t two[6] = { 0, 1, 2, 3, 4, 5 };
        if (tf_mesh_ply_faces(s, two, 2) != TF_INVALID_ARG) fail("2 of 1 faces", 0);
        expect_rejected(tf_mesh_ply_end(s, 1), bad, "too many faces");
        // a declared column that does not come
        if (tf_mesh_ply_begin(bad.c_str(), 10, 0, TF_MESH_NORMALS, &s) != TF_OK) fail("begin", 5);
        if (tf_mesh_ply_vertices(s, m.pos.data(), nullptr, nullptr, 10) != TF_INVALID_ARG) fail("no normals", 0);
        expect_rejected(tf_mesh_ply_end(s, 1), bad, "a missing column");
        // the caller gives up on a stream that was fine: TF_OK, and no file
        if (tf_mesh_ply_begin(bad.c_str(), 10, 0, 0, &s) != TF_OK) fail("begin", 6);
        tf_mesh_ply_vertices(s, m.pos.data(), nullptr, nullptr, 10);
        if (tf_mesh_ply_end(s, 0) != TF_OK) fail("give-up end", 0);
        if (exists(bad)) fail("a given-up stream left a file", 0);
        // arguments
        expect_rejected(tf_mesh_ply_begin(nullptr, 1, 1, 0, &s), bad, "no path");
        expect_rejected(tf_mesh_ply_begin(bad.c_str(), 1, 1, 0, nullptr), bad, "no stream pointer");
        expect_rejected(tf_mesh_ply_begin(bad.c_str(), -1, 1, 0, &s), bad, "nv < 0");
        expect_rejected(tf_mesh_ply_begin(bad.c_str(), 1, -1, 0, &s), bad, "nt < 0");
        expect_rejected(tf_mesh_ply_begin(bad.c_str(), 0x80000000LL, 0, 0, &s), bad, "nv > INT_MAX");
        expect_rejected(tf_mesh_ply_begin(bad.c_str(), 1, 1, TF_MESH_WHOLE, &s), bad, "an attribute bit that names no column");
        expect_rejected(tf_mesh_ply_begin((dir + "no/such/dir/x.ply").c_str(), 1, 1, 0, &s), bad, "a path that cannot be written");
        if (s) fail("a refused begin left a stream", 0);
        expect_rejected(tf_mesh_ply_vertices(nullptr, m.pos.data(), nullptr, nullptr, 1), bad, "no stream");
        expect_rejected(tf_mesh_ply_faces(nullptr, tri, 1), bad, "no stream");
        expect_rejected(tf_mesh_ply_end(nullptr, 1), bad, "no stream");
    }

    if (g_failures) { fprintf(stderr, "%d failures\n", g_failures); return 1; }
    printf("ok %d compared, %d rejected\n", g_compared, g_rejected);
    return 0;
}
