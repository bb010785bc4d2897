// mesh_ply_main.cpp -- drives the mesh's PLY writers (topfusion_amd/csrc/tf_mesh_ply.cpp) in one process;
// tests/test_mesh_attr_ref.py builds it for the CPU with -fsanitize=address,undefined.  Every input is
// handed over in a heap buffer of exactly its size, so a read past the end is a sanitizer report.
//
//   mesh_ply_main DIR
//
// Writes its files into DIR.  Prints "ok <files> written, <calls> rejected" and returns 0 when every valid
// call succeeds with a file that expands back to its input bit for bit, and every invalid call is
// TF_INVALID_ARG.
#include "../include/tfusion_hip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

static int g_written = 0, g_rejected = 0, g_failures = 0;

static void fail(const char* what, long a)
{
    ++g_failures;
    fprintf(stderr, "failed: %s %ld\n", what, a);
}

// a heap copy of exactly v's bytes (a distinct non-null pointer even when empty)
template <class T>
static T* exact(const std::vector<T>& v)
{
    T* p = (T*)malloc(v.size() * sizeof(T) ? v.size() * sizeof(T) : 1);
    if (!p) abort();
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static uint32_t g_rng = 12345u;
static uint32_t rnd(uint32_t n)
{
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

// the file read back: nv records of nw dwords and nf faces; false when its length does not fit its header
static bool read_back(const std::string& path, size_t nw, std::vector<uint32_t>& verts, std::vector<int32_t>& faces)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<unsigned char> buf;
    unsigned char chunk[4096];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    fclose(f);
    const std::string text(buf.begin(), buf.end());
    const size_t end = text.find("end_header\n"), ev = text.find("element vertex "), ef = text.find("element face ");
    if (end == std::string::npos || ev == std::string::npos || ef == std::string::npos || ev > end || ef > end) return false;
    const size_t nv = (size_t)atoll(text.c_str() + ev + 15), nf = (size_t)atoll(text.c_str() + ef + 13), body = end + 11;
    if (buf.size() != body + nv * nw * 4 + nf * 13) return false;
    verts.resize(nv * nw);
    if (nv) memcpy(verts.data(), buf.data() + body, nv * nw * 4);
    faces.resize(nf * 3);
    for (size_t i = 0; i < nf; ++i) {
        if (buf[body + nv * nw * 4 + 13 * i] != 3) return false;
        memcpy(&faces[3 * i], buf.data() + body + nv * nw * 4 + 13 * i + 1, 12);
    }
    for (int32_t i : faces)
        if (i < 0 || (size_t)i >= nv) return false;
    return true;
}

// one record per input vertex, as the file should expand to
static std::vector<uint32_t> records(const std::vector<float>& pos, const std::vector<float>* nrm, const std::vector<uint8_t>* col)
{
    const size_t n = pos.size() / 3, nw = 3 + (nrm ? 3 : 0) + (col ? 1 : 0);
    std::vector<uint32_t> r(n * nw);
    for (size_t i = 0; i < n; ++i) {
        memcpy(&r[i * nw], &pos[3 * i], 12);
        if (nrm) memcpy(&r[i * nw + 3], &(*nrm)[3 * i], 12);
        if (col) memcpy(&r[i * nw + (nrm ? 6 : 3)], &(*col)[4 * i], 4);
    }
    return r;
}

// a welding writer's file: distinct records, `want_distinct` of them (0: not checked), expanding to the input
static void check_welded(const std::string& path, const std::vector<uint32_t>& want, size_t nw, size_t want_distinct, const char* what)
{
    std::vector<uint32_t> verts;
    std::vector<int32_t> faces;
    ++g_written;
    if (!read_back(path, nw, verts, faces) || faces.size() * nw != want.size()) { fail(what, 0); return; }
    for (size_t i = 0; i < faces.size(); ++i)
        if (memcmp(&verts[(size_t)faces[i] * nw], &want[i * nw], 4 * nw)) { fail(what, (long)i); return; }
    const size_t nv = verts.size() / nw;
    for (size_t a = 0; a < nv; ++a)
        for (size_t b = a + 1; b < nv; ++b)
            if (!memcmp(&verts[a * nw], &verts[b * nw], 4 * nw)) { fail("two equal records", (long)a); return; }
    if (want_distinct && nv != want_distinct) fail("distinct records", (long)nv);
}

static void expect_rejected(tf_status s, const char* what)
{
    ++g_rejected;
    if (s != TF_INVALID_ARG) fail(what, (long)s);
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage\n"); return 2; }
    const std::string dir = std::string(argv[1]) + "/";

    // 300 triangles over a pool of 40 positions, each with one of two normals and colours: duplicated
    // positions, duplicated whole records, and equal positions with different attributes
    const size_t n = 300;
    std::vector<float> pool(40 * 3), tri(n * 9), nrm(n * 9);
    std::vector<uint8_t> col(n * 12);
    for (float& v : pool) v = (float)rnd(1000) * 0.01f - 5.0f;
    for (size_t i = 0; i < n * 3; ++i) {
        const uint32_t p = rnd(40), a = rnd(2);
        memcpy(&tri[3 * i], &pool[3 * p], 12);
        nrm[3 * i] = a ? 1.0f : 0.0f; nrm[3 * i + 1] = 0.0f; nrm[3 * i + 2] = a ? 0.0f : -1.0f;
        col[4 * i] = (uint8_t)p; col[4 * i + 1] = (uint8_t)(a * 200); col[4 * i + 2] = 7; col[4 * i + 3] = 255;
    }
    float* ht = exact(tri);
    float* hn = exact(nrm);
    uint8_t* hc = exact(col);
    std::string path = dir + "plain.ply";
    if (tf_mesh_write_ply(path.c_str(), ht, (long long)n) != TF_OK) fail("tf_mesh_write_ply", 0);
    check_welded(path, records(tri, nullptr, nullptr), 3, 0, "plain");
    for (int k = 0; k < 4; ++k) {
        path = dir + "attr" + std::to_string(k) + ".ply";
        if (tf_mesh_write_ply_attr(path.c_str(), ht, (k & 1) ? hn : nullptr, (k & 2) ? hc : nullptr, (long long)n) != TF_OK)
            fail("tf_mesh_write_ply_attr", k);
        check_welded(path, records(tri, (k & 1) ? &nrm : nullptr, (k & 2) ? &col : nullptr), 3 + ((k & 1) ? 3 : 0) + ((k & 2) ? 1 : 0), 0, "attr");
    }

    // 0.0f and -0.0f stay apart: two triangles over (0, 0, 0), (-0, 0, 0) and (1, 0, 0) have three vertices
    {
        const std::vector<float> z = { 0.0f, 0.0f, 0.0f, -0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -0.0f, 0.0f, 0.0f };
        float* hz = exact(z);
        path = dir + "zeros.ply";
        if (tf_mesh_write_ply(path.c_str(), hz, 2) != TF_OK) fail("tf_mesh_write_ply zeros", 0);
        check_welded(path, records(z, nullptr, nullptr), 3, 3, "zeros");
        free(hz);
    }

    // the indexed writer: the pool as the vertex table (with a duplicated position), random indices
    const size_t nv = 41, nt = 250;
    std::vector<float> vp(pool), vn(nv * 3);
    vp.insert(vp.end(), pool.begin(), pool.begin() + 3);
    std::vector<uint8_t> vc(nv * 4);
    std::vector<uint32_t> idx(nt * 3);
    for (size_t i = 0; i < nv * 3; ++i) vn[i] = (float)rnd(3) - 1.0f;
    for (size_t i = 0; i < nv * 4; ++i) vc[i] = (uint8_t)rnd(256);
    for (uint32_t& i : idx) i = rnd((uint32_t)nv);
    idx[0] = (uint32_t)nv - 1;
    float* hvp = exact(vp);
    float* hvn = exact(vn);
    uint8_t* hvc = exact(vc);
    uint32_t* hi = exact(idx);
    for (int k = 0; k < 4; ++k) {
        path = dir + "indexed" + std::to_string(k) + ".ply";
        const size_t nw = 3 + ((k & 1) ? 3 : 0) + ((k & 2) ? 1 : 0);
        if (tf_mesh_write_ply_indexed(path.c_str(), hvp, (k & 1) ? hvn : nullptr, (k & 2) ? hvc : nullptr, (long long)nv, hi, (long long)nt) != TF_OK)
            fail("tf_mesh_write_ply_indexed", k);
        std::vector<uint32_t> verts;
        std::vector<int32_t> faces;
        ++g_written;
        if (!read_back(path, nw, verts, faces) || verts != records(vp, (k & 1) ? &vn : nullptr, (k & 2) ? &vc : nullptr) ||
            faces.size() != idx.size() || memcmp(faces.data(), idx.data(), 4 * idx.size()))
            fail("indexed file", k);
    }

    // empty meshes, without and with attribute columns (non-null, never read: one byte each)
    {
        const std::vector<float> none;
        float* d = exact(none);
        std::vector<uint32_t> verts;
        std::vector<int32_t> faces;
        const std::string e[5] = { dir + "e0.ply", dir + "e1.ply", dir + "e2.ply", dir + "e3.ply", dir + "e4.ply" };
        if (tf_mesh_write_ply(e[0].c_str(), nullptr, 0) != TF_OK || !read_back(e[0], 3, verts, faces) || !faces.empty()) fail("empty plain", 0);
        if (tf_mesh_write_ply_attr(e[1].c_str(), nullptr, nullptr, nullptr, 0) != TF_OK || !read_back(e[1], 3, verts, faces)) fail("empty attr", 0);
        if (tf_mesh_write_ply_attr(e[2].c_str(), nullptr, d, (const uint8_t*)d, 0) != TF_OK || !read_back(e[2], 7, verts, faces)) fail("empty attr", 1);
        if (tf_mesh_write_ply_indexed(e[3].c_str(), nullptr, nullptr, nullptr, 0, nullptr, 0) != TF_OK || !read_back(e[3], 3, verts, faces))
            fail("empty indexed", 0);
        if (tf_mesh_write_ply_indexed(e[4].c_str(), nullptr, d, (const uint8_t*)d, 0, nullptr, 0) != TF_OK || !read_back(e[4], 7, verts, faces))
            fail("empty indexed", 1);
        // vertices without faces are a valid table
        if (tf_mesh_write_ply_indexed(e[4].c_str(), hvp, hvn, nullptr, (long long)nv, nullptr, 0) != TF_OK || !read_back(e[4], 6, verts, faces) ||
            verts.size() != nv * 6 || !faces.empty())
            fail("vertices only", 0);
        g_written += 6;
        free(d);
    }

    // refused: an index equal to nv, and the null / negative argument set
    path = dir + "bad.ply";
    idx[idx.size() - 1] = (uint32_t)nv;
    uint32_t* hbad = exact(idx);
    expect_rejected(tf_mesh_write_ply_indexed(path.c_str(), hvp, hvn, hvc, (long long)nv, hbad, (long long)nt), "index == nv");
    expect_rejected(tf_mesh_write_ply_indexed(path.c_str(), nullptr, nullptr, nullptr, 0, hi, 1), "index into an empty table");
    expect_rejected(tf_mesh_write_ply_indexed(nullptr, hvp, hvn, hvc, (long long)nv, hi, (long long)nt), "indexed: no path");
    expect_rejected(tf_mesh_write_ply_indexed(path.c_str(), nullptr, hvn, hvc, (long long)nv, hi, (long long)nt), "indexed: no vertices");
    expect_rejected(tf_mesh_write_ply_indexed(path.c_str(), hvp, hvn, hvc, (long long)nv, nullptr, (long long)nt), "indexed: no indices");
    expect_rejected(tf_mesh_write_ply_indexed(path.c_str(), hvp, hvn, hvc, -1, hi, (long long)nt), "indexed: nv < 0");
    expect_rejected(tf_mesh_write_ply_indexed(path.c_str(), hvp, hvn, hvc, (long long)nv, hi, -1), "indexed: nt < 0");
    expect_rejected(tf_mesh_write_ply_indexed(path.c_str(), hvp, nullptr, nullptr, 0x80000000LL, nullptr, 0), "indexed: nv > INT_MAX");
    expect_rejected(tf_mesh_write_ply(nullptr, ht, (long long)n), "plain: no path");
    expect_rejected(tf_mesh_write_ply(path.c_str(), nullptr, (long long)n), "plain: no triangles");
    expect_rejected(tf_mesh_write_ply(path.c_str(), ht, -1), "plain: n < 0");
    expect_rejected(tf_mesh_write_ply(path.c_str(), ht, 0x7fffffffLL / 3 + 1), "plain: n > INT_MAX / 3");
    expect_rejected(tf_mesh_write_ply_attr(nullptr, ht, hn, hc, (long long)n), "attr: no path");
    expect_rejected(tf_mesh_write_ply_attr(path.c_str(), nullptr, hn, hc, (long long)n), "attr: no triangles");
    expect_rejected(tf_mesh_write_ply_attr(path.c_str(), ht, hn, hc, -1), "attr: n < 0");
    expect_rejected(tf_mesh_write_ply_attr(path.c_str(), ht, hn, hc, 0x7fffffffLL / 3 + 1), "attr: n > INT_MAX / 3");
    expect_rejected(tf_mesh_write_ply((dir + "no/such/dir/x.ply").c_str(), ht, (long long)n), "a path that cannot be written");
    if (FILE* f = fopen(path.c_str(), "rb")) { fclose(f); fail("a refused call left a file", 0); }

    free(ht); free(hn); free(hc); free(hvp); free(hvn); free(hvc); free(hi); free(hbad);
    if (g_failures) { fprintf(stderr, "%d failures\n", g_failures); return 1; }
    printf("ok %d written, %d rejected\n", g_written, g_rejected);
    return 0;
}
