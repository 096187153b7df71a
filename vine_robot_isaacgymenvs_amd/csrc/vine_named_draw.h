// vine_named_draw.h — the named draw, stated once for every translation unit that draws per-env values from
// VineEnvRedrawName slots: vine_env_redraw.hip and vine_env_adr.hip (through vine_env_redraw_draw.h), vine_env_sensor.hip,
// vine_env_push.hip and vine_env_target.hip.  utils/named_draw.py is the same statement in numpy.
//
// A name is a number, a range or a value list (include/vine_env_redraw.h, VineEnvRedrawForm); what global env g gets in
// episode k is a pure function of (seed, key, g, k).  Here: the value (`redraw_value`, host and device), the host's check of
// one name (`named_check`, the eight refusals every *_spec entry point makes, in one order), the text of a refusal
// (`named_refusal`) and the device's per-episode tail (`VINE_NAMED_REDRAW_ROWS`).
//
// EVERY INCLUDING UNIT IS COMPILED WITHOUT FLOATING-POINT CONTRACTION (native.py, and the pragma in front of the unit's
// includes): `lo + (hi - lo) * u` must stay a multiply and an add, each rounded, as numpy forms it.
//
// Besides include/vine_env_redraw.h this needs vine_observer.h, for the error text a refusal sets (vine_invalid_arg).
//
// A NEW FEATURE supplies: its names (an enum of slots, a table of their draw names, the Python NAMES / DRAW_NAMES), which of
// them are integers, a `bad_value(slot, v)` for what a single value may be, its own checks over the envelope `named_check`
// returns, and its kernel body, which ends in `VINE_NAMED_REDRAW_ROWS`.
#ifndef VINE_NAMED_DRAW_H
#define VINE_NAMED_DRAW_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/vine_env_redraw.h"
#include "vine_observer.h"

namespace {

__host__ __device__ inline unsigned long long mix64(unsigned long long x) {      // splitmix64's finaliser
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// u in [0, 1) of (seed, key, global env id g, episode k); k == 0 gives utils/env_params.py uniform01
__host__ __device__ inline double redraw_u(unsigned long long seed, unsigned long long key, unsigned long long g,
                                           unsigned long long k) {
    const unsigned long long pre = mix64(seed ^ key) + g * 0x9E3779B97F4A7C15ull;
    const unsigned long long h = mix64(pre ^ mix64(k));
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

// the value of one name (present: form != ABSENT) for env g in episode k
__host__ __device__ inline double redraw_value(const VineEnvRedrawName& nm, bool integer, const double* values,
                                               unsigned long long seed, unsigned long long g, unsigned long long k) {
    if (nm.form == VINE_REDRAW_NUMBER) return nm.lo;
    if (nm.form == VINE_REDRAW_VALUES) {
        const unsigned long long count = (unsigned long long)nm.values_count;
        unsigned long long i;
        if (k == 0ull) {
            i = (g / nm.radix) % count;
        } else {
            const double u = redraw_u(seed, nm.key, g, k);
            i = (unsigned long long)floor(u * (double)nm.values_count);
            if (i > count - 1ull) i = count - 1ull;
        }
        return values[(size_t)nm.values_first + i];
    }
    const double u = redraw_u(seed, nm.key, g, k);
    const double lo = nm.lo, hi = nm.hi;
    if (integer) return fmin(lo + floor(u * (hi - lo + 1.0)), hi);
    return lo + (hi - lo) * u;
}

// The tail of a kernel whose table holds NAMES rows of named draws: env e (flagged for a reset by the step) enters its next
// episode and gets that episode's values.  `integer_mask`: bit q set where name q ranges over the integers.
//
// A macro, not a function, because the kernels must compile to what they compiled to with the tail written out in each.  As
// a function -- __forceinline__ or not, the slots passed by pointer, by reference or as the whole spec, the count a template
// parameter or an argument -- the loop is unrolled before the body reaches the kernel, and the compiler then fetches the
// whole kernel-argument struct in front of the reset branch instead of reading each slot where the tail uses it
// (profiles/named_draw/kernel_resources.txt has both tables).
#define VINE_NAMED_REDRAW_ROWS(NAMES, name, integer_mask, values, seed, env_off, e, n, table, episode_index)                   \
    do {                                                                                                                        \
        const int k_ = (episode_index)[e] + 1;                                                                                  \
        (episode_index)[e] = k_;                                                                                                \
        const unsigned long long g_ = (unsigned long long)(env_off) + (unsigned long long)(e);                                  \
        _Pragma("unroll") for (int q_ = 0; q_ < (NAMES); ++q_)                                                                  \
            (table)[(size_t)q_ * (n) + (e)] = (float)redraw_value((name)[q_], (((integer_mask) >> q_) & 1u) != 0u, values, seed, g_, \
                                                                  (unsigned long long)(long long)k_);                           \
    } while (0)

// What the host's check of one name finds: why it is refused (nullptr: it is not) and the envelope [lo, hi] of what the name
// can give an env (0, 0 for an absent name).
struct NamedCheck {
    const char* why;
    double lo, hi;
};

inline const char* any_value(double) { return nullptr; }      // the `bad_value` of a unit without a word on single values

// One name of a spec against the host copy of the value lists.  `bad_value(v)`: the unit's own word on a single value the
// name can take -- a reason, or nullptr.  `absent_ok`: the unit keeps a name that is ABSENT (then {nullptr, 0, 0}).  The
// refusals, in this order: reserved, a number that is not finite, a range without finite lo <= hi, the extent of a value
// list, its radix, a listed value that is not finite, an absent name, an unknown form; a value's own refusal follows the
// finiteness of that value.
template <class BadValue>
inline NamedCheck named_check(const VineEnvRedrawName& nm, const double* host_values, int num_values, bool absent_ok,
                              BadValue bad_value) {
    if (nm.reserved != 0) return {"reserved must be 0", 0.0, 0.0};
    if (nm.form == VINE_REDRAW_NUMBER) {
        if (!std::isfinite(nm.lo)) return {"the number is not finite", 0.0, 0.0};
        return {bad_value(nm.lo), nm.lo, nm.lo};
    }
    if (nm.form == VINE_REDRAW_RANGE) {
        if (!std::isfinite(nm.lo) || !std::isfinite(nm.hi) || nm.lo > nm.hi) return {"a range needs finite lo <= hi", 0.0, 0.0};
        const char* why = bad_value(nm.lo);
        return {why ? why : bad_value(nm.hi), nm.lo, nm.hi};
    }
    if (nm.form == VINE_REDRAW_VALUES) {
        if (nm.values_count < 1 || nm.values_first < 0 || (long long)nm.values_first + nm.values_count > num_values)
            return {"the extent of the value list lies outside the values array", 0.0, 0.0};
        if (nm.radix < 1) return {"radix must be at least 1", 0.0, 0.0};
        double lo = host_values[nm.values_first], hi = lo;
        for (int i = 0; i < nm.values_count; ++i) {
            const double v = host_values[nm.values_first + i];
            if (!std::isfinite(v)) return {"a listed value is not finite", 0.0, 0.0};
            if (const char* why = bad_value(v)) return {why, 0.0, 0.0};
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
        return {nullptr, lo, hi};
    }
    if (nm.form == VINE_REDRAW_ABSENT)
        return {absent_ok ? nullptr : "absent: every name needs a number, a range or a value list", 0.0, 0.0};
    return {"unknown form", 0.0, 0.0};
}

// "<unit>: <NAME>: <why>" as the library's error text; returns VINE_ERR_INVALID_ARG
inline int named_refusal(const char* unit, const char* name, const char* why) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s: %s: %s", unit, name, why);
    return vine_invalid_arg(msg);
}

}  // namespace

#endif
