// vine_env_redraw_draw.h — the draw of ENV_PARAMS_PER_EPISODE, stated once for the two translation units that form table
// columns on the device: vine_env_redraw.hip (include/vine_env_redraw.h) and vine_env_adr.hip (include/vine_env_adr.h).
//
// BOTH ARE COMPILED WITHOUT FLOATING-POINT CONTRACTION (native.py): `a + b * c` must stay a multiply and an add, each rounded,
// as numpy and the host pass form it.
//
// `redraw_value` and `redraw_column` are host and device functions: the spec functions form the candidates they check with
// the statements the kernels form their columns with.
#ifndef VINE_ENV_REDRAW_DRAW_H
#define VINE_ENV_REDRAW_DRAW_H

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/vine_env_redraw.h"
#include "vine_inertia_composites.h"

namespace {

constexpr int NL = VINE_NUM_LINKS;
static_assert(VR_NAMES == 15 && VR_FPAM_K == 8 && VR_CART_MASS == 12, "slots 0..7 are rows 0..7, 8..11 the FPAM vectors");
static_assert(VP_FPAM_K0 == 8 && VP_FPAM_C0 == 13 && VP_FPAM_b0 == 18 && VP_FPAM_B0 == 23 && VP_COUNT == 28, "FPAM rows");

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

// the two columns of an env from the per-name values v (read where the name is present): pcol = the parameter table's 28
// rows (the base's where a name is absent), icol = the inertia table's 31, the derived rows from the primary ones
__host__ __device__ inline void redraw_column(const VineEnvRedrawSpec& S, const double v[VR_NAMES], float pcol[VP_COUNT],
                                              float icol[VI_COUNT]) {
#pragma unroll
    for (int p = 0; p < VP_COUNT; ++p) pcol[p] = S.base_params[p];
#pragma unroll
    for (int s = 0; s < VR_FPAM_K; ++s)
        if (S.name[s].form != VINE_REDRAW_ABSENT) pcol[s] = (float)v[s];
#pragma unroll
    for (int s = VR_FPAM_K; s <= VR_FPAM_B; ++s)
        if (S.name[s].form != VINE_REDRAW_ABSENT) {
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int p = VP_FPAM_K0 + (s - VR_FPAM_K) * NL + j;
                pcol[p] = (float)((double)S.base_params[p] * v[s]);
            }
        }
    icol[VI_CART_MASS] = S.name[VR_CART_MASS].form != VINE_REDRAW_ABSENT ? (float)v[VR_CART_MASS] : S.base_inertia[VI_CART_MASS];
    const double link = S.name[VR_LINK_MASS].form != VINE_REDRAW_ABSENT ? v[VR_LINK_MASS] : 1.0;
    const double tip = S.name[VR_TIP_LINK_MASS].form != VINE_REDRAW_ABSENT ? v[VR_TIP_LINK_MASS] : 1.0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const double f = i == NL - 1 ? link * tip : link;
        icol[VI_LINK_MASS0 + i] = (float)((double)S.base_inertia[VI_LINK_MASS0 + i] * f);
        icol[VI_LINK_INERTIA0 + i] = (float)((double)S.base_inertia[VI_LINK_INERTIA0 + i] * f);
    }
    InertiaComposites ic;
    inertia_composites(icol[VI_CART_MASS], icol + VI_LINK_MASS0, icol + VI_LINK_INERTIA0, S.link_length, S.link_com, S.gravity, ic);
    icol[VI_MTOT] = (float)ic.mtot;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        icol[VI_B0 + i] = (float)ic.b[i];
        icol[VI_GB0 + i] = (float)ic.gb[i];
        icol[VI_ADIAG0 + i] = (float)ic.adiag[i];
        if (i > 0) icol[VI_AOFF1 + i - 1] = (float)ic.aoff[i];
    }
}

__host__ __device__ inline bool names_inertia(const VineEnvRedrawSpec& S) {
    return S.name[VR_CART_MASS].form != VINE_REDRAW_ABSENT || S.name[VR_LINK_MASS].form != VINE_REDRAW_ABSENT ||
           S.name[VR_TIP_LINK_MASS].form != VINE_REDRAW_ABSENT;
}

}  // namespace

#endif
