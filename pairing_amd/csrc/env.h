// The PA_* tuning knobs and regime bounds (INTEGRATION.md lists them): one
// parser for the integer and boolean ones.  Nothing is cached here; a call
// site reads its knob once, into a function-local static.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdlib.h>

namespace pa {

// unset: dflt; set: the value, clamped to [lo, hi] (text that is no number reads as 0)
inline long long env_clamp(const char* name, long long dflt, long long lo, long long hi) {
    const char* e = getenv(name);
    if (!e) return dflt;
    const long long v = strtoll(e, nullptr, 10);
    return v < lo ? lo : (v > hi ? hi : v);
}

// a count or size bound: any value from 0 up
inline size_t env_count(const char* name, size_t dflt) {
    return (size_t)env_clamp(name, (long long)dflt, 0, LLONG_MAX);
}

// unset, or set to a value outside [lo, hi]: dflt
inline long long env_within(const char* name, long long dflt, long long lo, long long hi) {
    const char* e = getenv(name);
    if (!e) return dflt;
    const long long v = strtoll(e, nullptr, 10);
    return v < lo || v > hi ? dflt : v;
}

// unset: dflt; set: whether the value is a nonzero number
inline bool env_flag(const char* name, bool dflt) {
    const char* e = getenv(name);
    return e ? strtoll(e, nullptr, 10) != 0 : dflt;
}

}  // namespace pa
