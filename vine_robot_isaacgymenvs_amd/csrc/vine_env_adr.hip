// vine_env_adr.hip — automatic domain randomisation of the per-episode plant (ENV_PARAMS_ADR) for MI355X (gfx950):
// include/vine_env_adr.h.
//
// Two launches behind every step.  decide: one wave, one lane per boundary, a ballot for the history slots.  redraw: one lane
// per env, VINE_ENV_ADR_THREADS envs per workgroup; every lane loads one word of its reward-matrix row, its reached word and
// its reset flag; a workgroup without a flagged lane leaves there.  The finished probing episodes of a workgroup are counted
// in LDS (integer atomics: order-free sums) and added to the global counts by at most 60 integer atomics per workgroup; the
// flagged lanes then draw and store their columns as vine_env_redraw_kernel does, from the range in force.
//
// THIS TRANSLATION UNIT IS COMPILED WITHOUT FLOATING-POINT CONTRACTION, as vine_env_redraw.hip is and for its reason: the
// range in force `start - widen * step` and a value `lo + (hi - lo) * u` must stay a multiply and an add, each rounded, as
// utils/env_params.py adr_replay forms them.  The pragma below says so for everything that follows, the shared draw
// included; native.py compiles this file with -ffp-contract=fast-honor-pragmas, under which the compiler obeys it.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/vine_env_adr.h"
#include "vine_adr_shared.h"
#include "vine_env_redraw_draw.h"
#include "vine_observer.h"

namespace {

constexpr int THREADS = VINE_ENV_ADR_THREADS;
constexpr int BOUNDARIES = 2 * VR_NAMES;
static_assert(ADR_HISTORY_WORDS == VINE_ENV_ADR_HISTORY_WORDS, "the history row of vine_adr_shared.h is the header's");
static_assert(BOUNDARIES <= 64, "decide is one wave, one lane per boundary");
static_assert(2 * BOUNDARIES <= THREADS, "the workgroup's counts are flushed by its first 2 * BOUNDARIES lanes");

// the boundary of slot s, side 0 = lo / 1 = hi, after w steps outward
__host__ __device__ inline double adr_bound(const VineEnvAdrSpec& A, int s, int side, int w) {
    const VineEnvAdrName& a = A.name[s];
    const VineEnvRedrawName& lim = A.redraw.name[s];
    if (side == 0) return adr_bound_lo(lim.lo, a.start_lo, a.step, w);
    return adr_bound_hi(lim.hi, a.start_hi, a.step, w);
}

__global__ __launch_bounds__(64) void vine_env_adr_decide_kernel(const VineEnvAdrSpec A, const unsigned long long* __restrict__ counters,
                                                                 const int glog, int* __restrict__ widen, int* __restrict__ counts,
                                                                 int* __restrict__ history, unsigned long long* __restrict__ cursor) {
    adr_decide_lane((int)threadIdx.x, BOUNDARIES, A.queue, A.widen_at, A.narrow_at, A.history_capacity,
                    [&A](int b) { return A.name[b >> 1].on != 0; }, [&A](int b) { return A.max_widen[b >> 1][b & 1]; }, counters, glog,
                    widen, counts, history, cursor);
}

__global__ __launch_bounds__(THREADS) void vine_env_adr_redraw_kernel(const VineEnvAdrSpec A, const int n, const unsigned env_off,
                                                                      const long long* __restrict__ reset,
                                                                      const float* __restrict__ rmat, float* __restrict__ st,
                                                                      float* __restrict__ ptab, float* __restrict__ itab,
                                                                      int* __restrict__ episode_index, const int* __restrict__ widen,
                                                                      int* __restrict__ counts, int* __restrict__ reached,
                                                                      int* __restrict__ probe) {
    __shared__ int wg_counts[2 * BOUNDARIES];
    const int e = blockIdx.x * THREADS + (int)threadIdx.x;
    if (threadIdx.x < 2 * BOUNDARIES) wg_counts[threadIdx.x] = 0;
    bool flagged = false;
    int r = 0;
    if (e < n) {
        const bool now = rmat[(size_t)e * VINE_NUM_REWARDS + 2] != 0.0f;
        r = reached[e] | (now ? 1 : 0);
        flagged = reset[e] != 0;
        if (!flagged && now) reached[e] = 1;
    }
    if (!__syncthreads_or(flagged)) return;       // nobody in this workgroup finished an episode (uniform); also the barrier
    if (flagged) {                                // behind the zeroing of wg_counts
        const int p = probe[e];
        if (p >= 0 && p < BOUNDARIES) {
            atomicAdd(&wg_counts[2 * p], 1);
            if (r) atomicAdd(&wg_counts[2 * p + 1], 1);
        }
        reached[e] = 0;
    }
    __syncthreads();
    if (threadIdx.x < 2 * BOUNDARIES && wg_counts[threadIdx.x] != 0) atomicAdd(&counts[threadIdx.x], wg_counts[threadIdx.x]);
    if (!flagged) return;

    const VineEnvRedrawSpec& S = A.redraw;
    const int k = episode_index[e] + 1;
    episode_index[e] = k;
    const unsigned long long g = (unsigned long long)env_off + (unsigned long long)e, kk = (unsigned long long)(long long)k;

    // which boundary, if any, this episode probes
    int pick = -1;
    if (redraw_u(S.seed, VINE_ENV_ADR_KEY_PROBE, g, kk) < A.boundary_fraction) {
        const double u_w = redraw_u(S.seed, VINE_ENV_ADR_KEY_WHICH, g, kk);
        const int j = min((int)floor(u_w * (double)(2 * A.num_adr)), 2 * A.num_adr - 1);
        pick = 2 * A.adr_slot[j >> 1] + (j & 1);
    }
    probe[e] = pick;

    double v[VR_NAMES];
#pragma unroll
    for (int s = 0; s < VR_NAMES; ++s) {
        v[s] = 0.0;
        if (S.name[s].form == VINE_REDRAW_ABSENT) continue;
        if (!A.name[s].on) {
            v[s] = redraw_value(S.name[s], s == VR_ACTION_DELAY, S.values, S.seed, g, kk);
            continue;
        }
        VineEnvRedrawName nm = S.name[s];         // the range in force in the place of the limits
        nm.lo = adr_bound(A, s, 0, widen[2 * s]);
        nm.hi = adr_bound(A, s, 1, widen[2 * s + 1]);
        v[s] = redraw_value(nm, s == VR_ACTION_DELAY, S.values, S.seed, g, kk);
        if (pick == 2 * s) v[s] = nm.lo;
        if (pick == 2 * s + 1) v[s] = nm.hi;
    }
    float pcol[VP_COUNT], icol[VI_COUNT];
    redraw_column(S, v, pcol, icol);

    if (S.name[VR_ACTION_DELAY].form != VINE_REDRAW_ABSENT) {
        const float old_delay = ptab[(size_t)VP_ACTION_DELAY * n + e];
        if (old_delay != pcol[VP_ACTION_DELAY]) {
#pragma unroll
            for (int j = 0; j < 2 * VINE_MAX_DELAY; ++j) st[(size_t)(VF_FIFO0 + j) * n + e] = 0.0f;
        }
    }
#pragma unroll
    for (int s = 0; s < VR_FPAM_K; ++s)
        if (S.name[s].form != VINE_REDRAW_ABSENT) ptab[(size_t)s * n + e] = pcol[s];
#pragma unroll
    for (int s = VR_FPAM_K; s <= VR_FPAM_B; ++s)
        if (S.name[s].form != VINE_REDRAW_ABSENT) {
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int p = VP_FPAM_K0 + (s - VR_FPAM_K) * NL + j;
                ptab[(size_t)p * n + e] = pcol[p];
            }
        }
    if (itab) {
#pragma unroll
        for (int r2 = 0; r2 < VI_COUNT; ++r2) itab[(size_t)r2 * n + e] = icol[r2];
    }
}

int bad_name(int s, const char* why) { return named_refusal("env adr spec", kRedrawNames[s], why); }

}  // namespace

extern "C" {

int vine_env_adr_spec_size(void) { return (int)sizeof(VineEnvAdrSpec); }

int vine_env_adr_spec(const VineConfig* cfg, const VineEnvRedrawSpec* redraw, const VineEnvAdrName names[VR_NAMES],
                      double boundary_fraction, int queue, double widen_at, double narrow_at, int history_capacity,
                      VineEnvAdrSpec* out) {
    if (!cfg || !redraw || !names || !out) return vine_invalid_arg("null argument to vine_env_adr_spec");
    if (redraw->abi_version != VINE_ENV_REDRAW_ABI_VERSION) return vine_invalid_arg("VineEnvRedrawSpec.abi_version mismatch");
    if (redraw->checked != 1u) return vine_invalid_arg("env adr spec: the VineEnvRedrawSpec was not filled by vine_env_redraw_spec");
    if (!(boundary_fraction >= 0.0 && boundary_fraction < 1.0)) return vine_invalid_arg("env adr spec: BOUNDARY_FRACTION must lie in [0, 1)");
    if (queue < 1) return vine_invalid_arg("env adr spec: QUEUE must be at least 1");
    if (!std::isfinite(widen_at) || !std::isfinite(narrow_at) || !(narrow_at < widen_at))
        return vine_invalid_arg("env adr spec: NARROW_AT must be below WIDEN_AT");
    if (history_capacity < 1) return vine_invalid_arg("env adr spec: the history capacity must be at least 1");
    VineEnvAdrSpec A;
    memset(&A, 0, sizeof A);
    A.abi_version = VINE_ENV_ADR_ABI_VERSION;
    A.queue = queue;
    A.history_capacity = history_capacity;
    A.boundary_fraction = boundary_fraction;
    A.widen_at = widen_at;
    A.narrow_at = narrow_at;
    A.redraw = *redraw;
    for (int s = 0; s < VR_NAMES; ++s) A.adr_slot[s] = -1;
    for (int s = 0; s < VR_NAMES; ++s) {
        const VineEnvAdrName& a = names[s];
        const VineEnvRedrawName& lim = redraw->name[s];
        if (a.reserved != 0) return bad_name(s, "reserved must be 0");
        if (!a.on) {
            if (a.start_lo != 0.0 || a.start_hi != 0.0 || a.step != 0.0) return bad_name(s, "START and STEP of a name that is not under ADR must be 0");
            continue;
        }
        if (lim.form != VINE_REDRAW_RANGE) return bad_name(s, "a name under ADR must be a [lo, hi] range of ENV_PARAMS");
        if (!std::isfinite(a.start_lo) || !std::isfinite(a.start_hi) || a.start_lo > a.start_hi)
            return bad_name(s, "START needs finite lo <= hi");
        if (a.start_lo < lim.lo || a.start_hi > lim.hi) return bad_name(s, "START lies outside the limits, the name's ENV_PARAMS range");
        if (!std::isfinite(a.step) || !(a.step > 0.0)) return bad_name(s, "STEP must be positive");
        if (s == VR_ACTION_DELAY && (a.start_lo != std::floor(a.start_lo) || a.start_hi != std::floor(a.start_hi) || a.step != std::floor(a.step)))
            return bad_name(s, "an integer parameter takes an integer START and STEP");
        double m_lo = std::ceil((a.start_lo - lim.lo) / a.step), m_hi = std::ceil((lim.hi - a.start_hi) / a.step);
        if (a.start_lo - m_lo * a.step > lim.lo) m_lo += 1.0;      // the quotient was rounded down to a whole number: the last
        if (a.start_hi + m_hi * a.step < lim.hi) m_hi += 1.0;      // step must arrive AT the limit, not an ulp inside it
        if (m_lo > 1073741824.0 || m_hi > 1073741824.0) return bad_name(s, "more than 2^30 STEPs between START and a limit");
        A.name[s] = a;
        A.name[s].on = 1;
        A.max_widen[s][0] = (int32_t)m_lo;
        A.max_widen[s][1] = (int32_t)m_hi;
        A.adr_slot[A.num_adr++] = s;
    }
    if (A.num_adr == 0) return vine_invalid_arg("env adr spec: no name is under ADR, there is no range to move");
    A.checked = 1u;
    *out = A;
    return VINE_OK;
}

int vine_env_adr_scheduled(VineHandle* h, const VineEnvAdrSpec* spec, const int64_t* reset, float* params_table,
                           float* inertia_table, int32_t* episode_index, int32_t* widen, int32_t* counts, int32_t* reached,
                           int32_t* probe, int32_t* history, int64_t* cursor, void* stream) {
    if (!h || !spec || !reset || !params_table || !episode_index || !widen || !counts || !reached || !probe || !history || !cursor)
        return vine_invalid_arg("null argument to vine_env_adr_scheduled");
    if (spec->abi_version != VINE_ENV_ADR_ABI_VERSION) return vine_invalid_arg("VineEnvAdrSpec.abi_version mismatch");
    if (spec->redraw.abi_version != VINE_ENV_REDRAW_ABI_VERSION) return vine_invalid_arg("VineEnvRedrawSpec.abi_version mismatch");
    if (spec->checked != 1u || spec->redraw.checked != 1u) return vine_invalid_arg("VineEnvAdrSpec was not filled by vine_env_adr_spec");
    const VineEnvRedrawSpec& S = spec->redraw;
    if (S.num_values > 0 && !S.values) return vine_invalid_arg("VineEnvRedrawSpec.values is NULL");
    VineHandleInfo info;
    int rc = vine_handle_info(h, &info);
    if (rc) return rc;
    const float *bound_params = nullptr, *bound_inertia = nullptr;
    unsigned env_off = 0;
    rc = vine_env_tables_of(h, &bound_params, &bound_inertia, &env_off);
    if (rc) return rc;
    if (!bound_params)
        return vine_invalid_arg("vine_env_adr_scheduled needs a parameter table bound to the handle (vine_bind_env_params)");
    if (bound_params != params_table)
        return vine_invalid_arg("vine_env_adr_scheduled: params_table is not the table bound to the handle");
    if (names_inertia(S) && (!bound_inertia || !inertia_table))
        return vine_invalid_arg("vine_env_adr_scheduled: the spec names masses and needs an inertia table bound to the handle "
                                "(vine_bind_env_inertia)");
    if (inertia_table && bound_inertia != inertia_table)
        return vine_invalid_arg("vine_env_adr_scheduled: inertia_table is not the table bound to the handle");
    const float* rmat = vine_reward_matrix_of(h);
    if (!rmat)
        return vine_invalid_arg("vine_env_adr_scheduled needs a reward matrix bound to the handle (vine_bind_reward_matrix) "
                                "before the step it rides behind");
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vine_env_adr_decide_kernel, dim3(1), dim3(64), 0, s, *spec, info.counters, info.glog, widen, counts, history,
                       (unsigned long long*)cursor);
    rc = vine_launch_status("vine_env_adr_decide");
    if (rc) return rc;
    const int blocks = (info.n + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(vine_env_adr_redraw_kernel, dim3(blocks), dim3(THREADS), 0, s, *spec, info.n, env_off, (const long long*)reset,
                       rmat, info.state, params_table, names_inertia(S) ? inertia_table : nullptr, episode_index, (const int*)widen,
                       counts, reached, probe);
    return vine_launch_status("vine_env_adr_redraw");
}

}  // extern "C"
