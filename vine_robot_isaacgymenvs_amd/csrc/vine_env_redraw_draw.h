// vine_env_redraw_draw.h — what the two translation units that form table COLUMNS on the device share beyond the named draw
// itself (vine_named_draw.h, which this includes): vine_env_redraw.hip (include/vine_env_redraw.h) and vine_env_adr.hip
// (include/vine_env_adr.h).
//
// BOTH ARE COMPILED WITHOUT FLOATING-POINT CONTRACTION (native.py): `a + b * c` must stay a multiply and an add, each rounded,
// as numpy and the host pass form it.
//
// `redraw_column` is a host and device function, as `redraw_value` is: the spec functions form the candidates they check with
// the statements the kernels form their columns with.
#ifndef VINE_ENV_REDRAW_DRAW_H
#define VINE_ENV_REDRAW_DRAW_H

#include "vine_inertia_composites.h"
#include "vine_named_draw.h"

namespace {

constexpr int NL = VINE_NUM_LINKS;
static_assert(VR_NAMES == 15 && VR_FPAM_K == 8 && VR_CART_MASS == 12, "slots 0..7 are rows 0..7, 8..11 the FPAM vectors");
static_assert(VP_FPAM_K0 == 8 && VP_FPAM_C0 == 13 && VP_FPAM_b0 == 18 && VP_FPAM_B0 == 23 && VP_COUNT == 28, "FPAM rows");

// the names of a spec's slots (VineEnvRedrawSlot), as a refusal words them
const char* const kRedrawNames[VR_NAMES] = {
    "DAMPING", "SMOOTHING_ALPHA_INFLATE", "SMOOTHING_ALPHA_DEFLATE", "RAIL_VELOCITY_SCALE", "RAIL_P_GAIN", "RAIL_D_GAIN",
    "RAIL_ACCELERATION", "ACTION_DELAY", "FPAM_K", "FPAM_C", "FPAM_b", "FPAM_B", "CART_MASS", "LINK_MASS", "TIP_LINK_MASS"};

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
