// vine_target_path.h — a moving target's path, stated once: the control step along an axis (step 4 of
// include/vine_env_target.h) and the words a point of the path puts into the state block (step 5).  vine_env_target.hip walks
// it one step behind every step of an env; vine_mpc_track.hip walks it H - 1 steps ahead for the predictive controller's
// samples.  Not part of the C ABI.
//
// Everything is float32, and every multiply, add, subtract and compare is its own rounded operation: both units switch
// contraction off by a pragma in front of everything they include, this header too.
#ifndef VINE_TARGET_PATH_H
#define VINE_TARGET_PATH_H

#include <hip/hip_runtime.h>

#include "../../include/vine_env_target.h"

// one control step along an axis of half-length S, reflected at its ends (one reflection suffices: the spec check)
__device__ __forceinline__ void target_path_advance(float& off, float& vel, const float S, const float cdt) {
    const float step = vel * cdt;
    float nx = off + step;
    if (nx > S) {
        nx = S - (nx - S);
        vel = -vel;
    } else if (nx < -S) {
        nx = -S - (nx + S);
        vel = -vel;
    }
    off = nx;
}

// The words of the offsets (oa, oc) about the anchor (ay, az, d0) along the axis (c, s).  A word the mode does not write
// keeps what the caller put there.
template <int MODE>
__device__ __forceinline__ void target_path_words(const float ay, const float az, const float d0, const float c, const float s,
                                                  const float oa, const float oc, float& ty, float& tz, float& depth) {
    if (MODE == VINE_TARGET_FREE) {
        ty = ay + oa;
        tz = az + oc;
    } else if (MODE == VINE_TARGET_SHELF) {
        ty = ay - oa;
        depth = d0 + oa;
    } else {
        const float py = oa * c, pz = oa * s;
        ty = ay - py;
        tz = az - pz;
        depth = d0 + oa;
    }
}

inline int target_path_mode_of(unsigned flags) {
    return (flags & VINE_FLAG_CREATE_PIPE) ? VINE_TARGET_PIPE : (flags & VINE_FLAG_CREATE_SHELF) ? VINE_TARGET_SHELF : VINE_TARGET_FREE;
}

#endif
