// ctx_mem_main.cpp -- drives the context's memory registry (topfusion_amd/csrc/tf_ctx_mem.h) and the
// environment-switch helpers (topfusion_amd/csrc/tf_env.h) on the CPU; tests/test_capi.py builds it with
// -fsanitize=address,undefined and runs it.
//
// The registry gets a counting malloc / free pair that fails on its k-th call.  A scripted sequence -- single
// buffers, a group of four, an early release and regrow, a second group, a scoped temporary -- runs for every k
// from 1 to one past its number of allocations, stopping at its first failure as an entry point would; after
// destruction nothing may be live.  The blocks are the C library's, so a block freed twice is a sanitizer report.
//
// Prints "ok <runs> runs, <allocations> allocations" and returns 0.
#include "../topfusion_amd/csrc/tf_ctx_mem.h"
#include "../topfusion_amd/csrc/tf_env.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static long g_calls, g_fail_at, g_allocs, g_frees, g_live, g_smallest_dev, g_failures;
enum { ERR_DEV = 2, ERR_PIN = 3, ERR_OOM = 4 };

#define EXPECT(cond)                                                                         \
    do {                                                                                     \
        if (!(cond)) { ++g_failures; fprintf(stderr, "line %d (k = %ld): %s\n", __LINE__, g_fail_at, #cond); } \
    } while (0)

static int count_alloc(void** p, size_t bytes, int err)
{
    if (++g_calls == g_fail_at) return err;
    *p = malloc(bytes);
    if (!*p) abort();
    ++g_allocs;
    ++g_live;
    return 0;
}
static int dev_alloc(void** p, size_t bytes)
{
    if ((long)bytes < g_smallest_dev) g_smallest_dev = (long)bytes;
    return count_alloc(p, bytes, ERR_DEV);
}
static int pin_alloc(void** p, size_t bytes, unsigned flags)
{
    EXPECT(flags == 7u);
    return count_alloc(p, bytes, ERR_PIN);
}
static int count_free(void* p)
{
    EXPECT(p != nullptr);
    free(p);
    ++g_frees;
    --g_live;
    return 0;
}
static const TfMemFns fns = { dev_alloc, count_free, pin_alloc, count_free, ERR_OOM };

// the scripted sequence; returns the first error, as the library's entry points do
static int script()
{
    TfCtxMem m(fns);
    float* a = nullptr; char* b = nullptr; int* pinned = nullptr;
    int e = m.alloc(&a, 100);
    if (e) { EXPECT(!a && e == ERR_DEV); return e; }
    if ((e = m.alloc(&b, 3)) != 0) { EXPECT(!b); return e; }                 // (16 bytes are asked for)
    if ((e = m.alloc(TfCtxMem::pin(&pinned, 64, 7u))) != 0) { EXPECT(!pinned && e == ERR_PIN); return e; }
    memset(b, 1, 16);
    {   // a group of four, all or none
        void* g[4] = { (void*)1, (void*)1, (void*)1, (void*)1 };
        const long live = g_live;
        e = m.alloc_group({ TfCtxMem::dev(&g[0], 40), TfCtxMem::dev(&g[1], 8), TfCtxMem::pin(&g[2], 24, 7u), TfCtxMem::dev(&g[3], 1000) });
        if (e) { EXPECT(!g[0] && !g[1] && !g[2] && !g[3] && g_live == live); return e; }
        EXPECT(g[0] && g[1] && g[2] && g[3] && g_live == live + 4);
    }
    {   // an early release and regrow; pointer values, not addresses, are what is recorded
        float* moved = a;
        a = nullptr;
        const long live = g_live;
        EXPECT(m.release(moved) == 0 && !moved && g_live == live - 1);
        EXPECT(m.release(moved) == 0 && g_live == live - 1);             // nullptr: nothing
        if ((e = m.alloc(&a, 400)) != 0) { EXPECT(!a); return e; }
        EXPECT(g_live == live);
    }
    {   // a second group
        long long* c0 = nullptr; long long* c1 = nullptr;
        const long live = g_live;
        e = m.alloc_group({ TfCtxMem::dev(&c0, 64), TfCtxMem::dev(&c1, 72) });
        if (e) { EXPECT(!c0 && !c1 && g_live == live); return e; }
    }
    {   // a scoped temporary of the same functions
        const long live = g_live;
        {
            TfCtxMem tmp(m.fns());
            char* t = nullptr;
            if ((e = tmp.alloc(&t, 12)) != 0) { EXPECT(!t); return e; }
            EXPECT(g_live == live + 1);
        }
        EXPECT(g_live == live);
    }
    return 0;
}

static void set_or_unset(const char* name, const char* value)
{
    if (value) setenv(name, value, 1);
    else unsetenv(name);
}

// (value, default) -> result, the expected column written from the expressions tf_create used:
//   default-on flags   !(env && env[0] == '0')          default-off flags   env && env[0] == '1'
//   integers           v = env ? atoi(env) : def; if (v < lo || v > hi) v = fallback
static void env_tables()
{
    static const struct { const char* v; int on, off; } flags[] = {
        { nullptr, 1, 0 }, { "", 1, 0 }, { "0", 0, 0 }, { "1", 1, 1 }, { "00", 0, 0 }, { "2", 1, 0 }, { "abc", 1, 0 }, { "01", 0, 0 }, { "10", 1, 1 },
    };
    for (const auto& f : flags) {
        set_or_unset("TF_TEST_SWITCH", f.v);
        EXPECT(tf_env_flag("TF_TEST_SWITCH", 1) == f.on);
        EXPECT(tf_env_flag("TF_TEST_SWITCH", 0) == f.off);
    }
    // wg: TFUSION_INTEG_WG_FRAME (768, [64, 2560], falls back to 2560); ck: TFUSION_CKPT_CHUNK_BLOCKS (4096, [1, 2^18], falls
    // back to its default); ed: TFUSION_ED_LDS_MAX_N's part of the helper (16384, negative -> 0; tf_read_env clamps the top)
    static const struct { const char* v; int wg, ck, ed; } ints[] = {
        { nullptr, 768, 4096, 16384 }, { "", 2560, 4096, 0 }, { "0", 2560, 4096, 0 }, { "1", 2560, 1, 1 }, { "00", 2560, 4096, 0 },
        { "2", 2560, 2, 2 }, { "abc", 2560, 4096, 0 }, { "-5", 2560, 4096, 0 }, { "63", 2560, 63, 63 }, { "64", 64, 64, 64 },
        { "1000", 1000, 1000, 1000 }, { "2560", 2560, 2560, 2560 }, { "2561", 2560, 2561, 2561 }, { "262144", 2560, 262144, 262144 },
        { "262145", 2560, 4096, 262145 },
    };
    for (const auto& i : ints) {
        set_or_unset("TF_TEST_SWITCH", i.v);
        EXPECT(tf_env_int("TF_TEST_SWITCH", 768, 64, 2560, 2560) == i.wg);
        EXPECT(tf_env_int("TF_TEST_SWITCH", 4096, 1, 1 << 18, 4096) == i.ck);
        EXPECT(tf_env_int("TF_TEST_SWITCH", 16384, 0, INT_MAX, 0) == i.ed);
    }
    static const struct { const char* v; long long n; } counts[] = { { nullptr, 0 }, { "", 0 }, { "0", 0 }, { "7", 7 }, { "abc", 0 }, { "5000000000", 5000000000LL } };
    for (const auto& n : counts) {
        set_or_unset("TF_TEST_SWITCH", n.v);
        EXPECT(tf_env_count("TF_TEST_SWITCH") == n.n);
    }
}

int main()
{
    // the sequence without a failure: how many allocations it makes
    g_fail_at = 0;
    g_smallest_dev = LONG_MAX;
    EXPECT(script() == 0);
    const long n = g_calls;
    EXPECT(n == 11 && g_allocs == n && g_frees == g_allocs && g_live == 0);
    EXPECT(g_smallest_dev == 16);                                            // alloc(&b, 3), the group's 8 and the temporary's 12
    long runs = 1;
    for (long k = 1; k <= n + 1; ++k, ++runs) {
        g_calls = g_allocs = g_frees = g_live = 0;
        g_fail_at = k;
        const int e = script();
        EXPECT((e != 0) == (k <= n));
        EXPECT(g_live == 0 && g_frees == g_allocs);
        EXPECT(g_allocs == (k <= n ? k - 1 : n));
    }
    g_fail_at = 0;
    env_tables();
    if (g_failures) return 1;
    printf("ok %ld runs, %ld allocations\n", runs, n);
    return 0;
}
