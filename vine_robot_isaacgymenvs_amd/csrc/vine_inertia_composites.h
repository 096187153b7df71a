// vine_inertia_composites.h — the constant coefficients of the absolute-angle Lagrangian from the masses: the one statement of
// them, for the host (vine_hip.hip: make_params, vine_env_inertia_derive) and for the device (vine_env_redraw.hip, which
// re-derives a column it has just redrawn).  Accumulated in double and rounded once by whoever stores them, so a uniform
// handle, a host-derived column and a device-derived column of the same float32 masses hold the same bits -- PROVIDED the
// translation unit that runs this on the device is compiled without floating-point contraction (native.py gives
// vine_env_redraw.hip -ffp-contract=off; the host pass targets baseline x86-64, which has no fused multiply-add).
// Not part of the C ABI.
#ifndef VINE_INERTIA_COMPOSITES_H
#define VINE_INERTIA_COMPOSITES_H

#include <hip/hip_runtime.h>

#include "../../include/vine.h"

struct InertiaComposites {
    double mtot, b[VINE_NUM_LINKS], gb[VINE_NUM_LINKS], adiag[VINE_NUM_LINKS], aoff[VINE_NUM_LINKS];   // aoff[i] = L b_i = a_ij, j < i
};

__host__ __device__ inline void inertia_composites(float cart_mass, const float* link_mass, const float* link_inertia,
                                                   float link_length, float link_com, float gravity, InertiaComposites& o) {
    constexpr int NLINKS = VINE_NUM_LINKS;
    double m[NLINKS], mt = cart_mass, L = link_length, l = link_com;
    for (int i = 0; i < NLINKS; ++i) { m[i] = link_mass[i]; mt += m[i]; }
    o.mtot = mt;
    for (int i = 0; i < NLINKS; ++i) {
        double distal = 0;
        for (int k = i + 1; k < NLINKS; ++k) distal += m[k];
        o.b[i] = m[i] * l + L * distal;
        o.gb[i] = (double)gravity * o.b[i];
        o.adiag[i] = m[i] * l * l + L * L * distal + (double)link_inertia[i];
        o.aoff[i] = L * o.b[i];
    }
}

#endif
