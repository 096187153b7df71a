// vine_adr_shared.h — what the two ADR units state alike, once: vine_env_adr.hip (ENV_PARAMS_ADR, the plant's ranges) and
// vine_env_draw_adr.hip (ENV_DRAW_ADR, the ranges of the sensor's, the push's and the target's named draws).
//
// Here: a boundary after w steps outward (`adr_bound_lo`, `adr_bound_hi`) and the decide launch's lane (`adr_decide_lane`):
// the rule that judges one boundary, the ballot-ordered history rows and the cursor update.  include/vine_env_adr.h states
// the semantics; utils/env_params.py adr_ranges and adr_decide are the same statements in numpy.
//
// EVERY INCLUDING UNIT IS COMPILED WITHOUT FLOATING-POINT CONTRACTION (the pragma in front of the unit's includes):
// `start - w * step` must stay a multiply and an add, each rounded, as numpy forms it.
//
// Besides <hip/hip_runtime.h> this needs vine_observer.h, for the step count a history row carries.
#ifndef VINE_ADR_SHARED_H
#define VINE_ADR_SHARED_H

#include <hip/hip_runtime.h>

#include "vine_observer.h"

namespace {

constexpr int ADR_HISTORY_WORDS = 4;      // (step index, boundary, new widen, 0)

// the lo / hi boundary after w steps outward from START, never past the limit
__host__ __device__ inline double adr_bound_lo(double limit_lo, double start_lo, double step, int w) {
    return fmax(limit_lo, start_lo - (double)w * step);
}
__host__ __device__ inline double adr_bound_hi(double limit_hi, double start_hi, double step, int w) {
    return fmin(limit_hi, start_hi + (double)w * step);
}

// Lane b of the decide launch (one wave; every lane of the workgroup calls this, the lanes past `boundaries` judge nothing).
// `on(b)`: is boundary b's name under ADR; `max_widen(b)`: the steps between START and the limit.  Both are read only where
// the rule needs them.
template <class On, class MaxWiden>
__device__ __forceinline__ void adr_decide_lane(const int b, const int boundaries, const int queue, const double widen_at,
                                                const double narrow_at, const int history_capacity, On on, MaxWiden max_widen,
                                                const unsigned long long* __restrict__ counters, const int glog,
                                                int* __restrict__ widen, int* __restrict__ counts, int* __restrict__ history,
                                                unsigned long long* __restrict__ cursor) {
    bool changed = false;
    int w_new = 0;
    if (b < boundaries && on(b)) {
        const int n = counts[2 * b], r = counts[2 * b + 1];
        if (n >= queue) {
            const int w = widen[b];
            w_new = w;
            if ((double)r >= widen_at * (double)n) w_new = min(w + 1, max_widen(b));
            else if ((double)r <= narrow_at * (double)n) w_new = max(w - 1, 0);
            changed = w_new != w;
            if (changed) widen[b] = w_new;
            counts[2 * b] = 0;
            counts[2 * b + 1] = 0;
        }
    }
    const unsigned long long ballot = __ballot(changed);
    if (ballot == 0ull) return;
    const unsigned long long base = cursor[0];
    if (changed) {
        const unsigned long long k = base + (unsigned long long)__popcll(ballot & ((1ull << b) - 1ull));
        int* row = history + (size_t)(k % (unsigned long long)history_capacity) * ADR_HISTORY_WORDS;
        row[0] = (int)(long long)vine_steps_completed(counters, glog) - 1;
        row[1] = b;
        row[2] = w_new;
        row[3] = 0;
    }
    __syncthreads();      // every lane has read the cursor
    if (b == 0) cursor[0] = base + (unsigned long long)__popcll(ballot);
}

}  // namespace

#endif
