// tf_env.h -- how an environment switch is read (host only).  The switches themselves, their defaults and
// what they mean are listed in one place: tf_read_env, tf_capi.hip.
#pragma once
#include <stdlib.h>

// A flag decided by the value's first character alone: a default-on flag goes off on "0...", a default-off
// flag goes on on "1..."; everything else (unset, "", "2", "abc") leaves the default.
static inline int tf_env_flag(const char* name, int def)
{
    const char* e = getenv(name);
    return def ? !(e && e[0] == '0') : (e && e[0] == '1');
}

// An integer (atoi: "" and "abc" read as 0), `def` when unset; a value outside [lo, hi] becomes `fallback`.
static inline int tf_env_int(const char* name, int def, int lo, int hi, int fallback)
{
    const char* e = getenv(name);
    const int v = e ? atoi(e) : def;
    return v < lo || v > hi ? fallback : v;
}

// A launch number of the fault-injection switches (atoll), 0 = never when unset.
static inline long long tf_env_count(const char* name)
{
    const char* e = getenv(name);
    return e ? atoll(e) : 0;
}
