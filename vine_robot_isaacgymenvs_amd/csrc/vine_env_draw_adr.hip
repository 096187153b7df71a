// vine_env_draw_adr.hip — automatic domain randomisation of the sensor's, the push's and the target's named draws
// (ENV_DRAW_ADR) for MI355X (gfx950): include/vine_env_draw_adr.h states the semantics, utils/env_draw_adr.py
// draw_adr_replay is the same statement in numpy.
//
// Two launches behind every step, behind the three observers' launches of that step.  decide: one wave, one lane per
// boundary (vine_adr_shared.h, the lane vine_env_adr.hip runs).  redraw: one lane per env, VINE_ENV_DRAW_ADR_THREADS envs per
// workgroup; every lane loads one word of its reward-matrix row, its reached word and its reset flag; a workgroup without a
// flagged lane leaves there.  The finished probing episodes of a workgroup are counted in LDS (integer atomics: order-free
// sums) and added to the global counts by at most 36 integer atomics per workgroup; a flagged lane then hashes twice for the
// probe and once per name under ADR, and stores one float per name under ADR: the row its observer's tail has just drawn from
// the limits, drawn again from the range in force with the same u.
//
// CONTRACTION IS OFF FOR THIS WHOLE TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it
// with -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): the range in force `start - widen * step` and a
// value `lo + (hi - lo) * u` must stay a multiply and an add, each rounded, as numpy forms them.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/vine_env_draw_adr.h"
#include "vine_adr_shared.h"
#include "vine_named_draw.h"
#include "vine_observer.h"

namespace {

constexpr int THREADS = VINE_ENV_DRAW_ADR_THREADS;
constexpr int BOUNDARIES = 2 * VDA_NAMES;
static_assert(ADR_HISTORY_WORDS == VINE_ENV_DRAW_ADR_HISTORY_WORDS, "the history row of vine_adr_shared.h is the header's");
static_assert(BOUNDARIES <= 64, "decide is one wave, one lane per boundary");
static_assert(2 * BOUNDARIES <= THREADS, "the workgroup's counts are flushed by its first 2 * BOUNDARIES lanes");
static_assert(VDA_NAMES == VSN_NAMES + VPU_NAMES + VTG_NAMES, "the slots are the three observers' names, one behind the other");

// where slot s lies: its group, its row in that group's table, and whether its range is over the integers
__host__ __device__ constexpr int group_of(int s) { return s < VSN_NAMES ? VDA_SENSOR : s < VSN_NAMES + VPU_NAMES ? VDA_PUSH : VDA_TARGET; }
__host__ __device__ constexpr int row_of(int s) { return s < VSN_NAMES ? s : s < VSN_NAMES + VPU_NAMES ? s - VSN_NAMES : s - VSN_NAMES - VPU_NAMES; }
__host__ __device__ constexpr bool integer_of(int s) { return s == VDA_SENSOR_DELAY; }

__global__ __launch_bounds__(64) void vine_env_draw_adr_decide_kernel(const VineEnvDrawAdrSpec A,
                                                                      const unsigned long long* __restrict__ counters, const int glog,
                                                                      int* __restrict__ widen, int* __restrict__ counts,
                                                                      int* __restrict__ history, unsigned long long* __restrict__ cursor) {
    adr_decide_lane((int)threadIdx.x, BOUNDARIES, A.queue, A.widen_at, A.narrow_at, A.history_capacity,
                    [&A](int b) { return A.slot[b >> 1].adr.on != 0; }, [&A](int b) { return A.slot[b >> 1].max_widen[b & 1]; },
                    counters, glog, widen, counts, history, cursor);
}

__global__ __launch_bounds__(THREADS) void vine_env_draw_adr_redraw_kernel(const VineEnvDrawAdrSpec A, const int n, const unsigned env_off,
                                                                           const long long* __restrict__ reset,
                                                                           const float* __restrict__ rmat, float* __restrict__ table0,
                                                                           float* __restrict__ table1, float* __restrict__ table2,
                                                                           const double* __restrict__ values,
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

    const int k = episode_index[e] + 1;
    episode_index[e] = k;
    const unsigned long long g = (unsigned long long)env_off + (unsigned long long)e, kk = (unsigned long long)(long long)k;

    // which boundary, if any, this episode probes
    int pick = -1;
    if (redraw_u(A.seed, VINE_ENV_DRAW_ADR_KEY_PROBE, g, kk) < A.boundary_fraction) {
        const double u_w = redraw_u(A.seed, VINE_ENV_DRAW_ADR_KEY_WHICH, g, kk);
        const int j = min((int)floor(u_w * (double)(2 * A.num_adr)), 2 * A.num_adr - 1);
        pick = 2 * A.adr_slot[j >> 1] + (j & 1);
    }
    probe[e] = pick;

#pragma unroll
    for (int s = 0; s < VDA_NAMES; ++s) {
        const VineEnvDrawAdrSlot& sl = A.slot[s];
        if (!sl.adr.on) continue;
        VineEnvRedrawName nm = sl.limits;         // the range in force in the place of the limits; the key is the observer's
        nm.lo = adr_bound_lo(sl.limits.lo, sl.adr.start_lo, sl.adr.step, widen[2 * s]);
        nm.hi = adr_bound_hi(sl.limits.hi, sl.adr.start_hi, sl.adr.step, widen[2 * s + 1]);
        double v = redraw_value(nm, integer_of(s), values, A.seed, g, kk);
        if (pick == 2 * s) v = nm.lo;
        if (pick == 2 * s + 1) v = nm.hi;
        float* const table = group_of(s) == VDA_SENSOR ? table0 : group_of(s) == VDA_PUSH ? table1 : table2;
        table[(size_t)row_of(s) * n + e] = (float)v;
    }
}

const char* const kNames[VDA_NAMES] = {"SENSOR_DELAY",     "SENSOR_HOLD",       "SENSOR_NOISE_STD",  "PUSH_RATE",         "PUSH_IMPULSE",
                                       "TARGET_VEL_ALONG", "TARGET_VEL_ACROSS", "TARGET_SPAN_ALONG", "TARGET_SPAN_ACROSS"};
const char* const kGroups[VDA_GROUPS] = {"ENV_SENSOR", "ENV_PUSH", "ENV_TARGET"};

int bad_name(int s, const char* why) { return named_refusal("env draw adr spec", kNames[s], why); }

}  // namespace

extern "C" {

int vine_env_draw_adr_spec_size(void) { return (int)sizeof(VineEnvDrawAdrSpec); }

int vine_env_draw_adr_spec(const VineConfig* cfg, const VineEnvSensorSpec* sensor, const VineEnvPushSpec* push,
                           const VineEnvTargetSpec* target, const VineEnvAdrName names[VDA_NAMES], double boundary_fraction,
                           int queue, double widen_at, double narrow_at, int history_capacity, VineEnvDrawAdrSpec* out) {
    if (!cfg || !names || !out) return vine_invalid_arg("null argument to vine_env_draw_adr_spec");
    if (cfg->abi_version != VINE_ABI_VERSION) return vine_invalid_arg("VineConfig.abi_version mismatch");
    if (sensor && sensor->abi_version != VINE_ENV_SENSOR_ABI_VERSION) return vine_invalid_arg("VineEnvSensorSpec.abi_version mismatch");
    if (push && push->abi_version != VINE_ENV_PUSH_ABI_VERSION) return vine_invalid_arg("VineEnvPushSpec.abi_version mismatch");
    if (target && target->abi_version != VINE_ENV_TARGET_ABI_VERSION) return vine_invalid_arg("VineEnvTargetSpec.abi_version mismatch");
    if (sensor && sensor->checked != 1u) return vine_invalid_arg("env draw adr spec: the VineEnvSensorSpec was not filled by vine_env_sensor_spec");
    if (push && push->checked != 1u) return vine_invalid_arg("env draw adr spec: the VineEnvPushSpec was not filled by vine_env_push_spec");
    if (target && target->checked != 1u) return vine_invalid_arg("env draw adr spec: the VineEnvTargetSpec was not filled by vine_env_target_spec");
    if ((sensor && sensor->seed != cfg->seed) || (push && push->seed != cfg->seed) || (target && target->seed != cfg->seed))
        return vine_invalid_arg("env draw adr spec: an observer spec's seed is not the configuration's: the draw would not be the observer's");
    if (!(boundary_fraction >= 0.0 && boundary_fraction < 1.0)) return vine_invalid_arg("env draw adr spec: BOUNDARY_FRACTION must lie in [0, 1)");
    if (queue < 1) return vine_invalid_arg("env draw adr spec: QUEUE must be at least 1");
    if (!std::isfinite(widen_at) || !std::isfinite(narrow_at) || !(narrow_at < widen_at))
        return vine_invalid_arg("env draw adr spec: NARROW_AT must be below WIDEN_AT");
    if (history_capacity < 1) return vine_invalid_arg("env draw adr spec: the history capacity must be at least 1");
    VineEnvDrawAdrSpec A;
    memset(&A, 0, sizeof A);
    A.abi_version = VINE_ENV_DRAW_ADR_ABI_VERSION;
    A.queue = queue;
    A.history_capacity = history_capacity;
    A.boundary_fraction = boundary_fraction;
    A.widen_at = widen_at;
    A.narrow_at = narrow_at;
    A.seed = cfg->seed;
    const VineEnvRedrawName* const group_names[VDA_GROUPS] = {sensor ? sensor->name : nullptr, push ? push->name : nullptr,
                                                              target ? target->name : nullptr};
    const int group_per_episode[VDA_GROUPS] = {sensor ? sensor->per_episode : 0, push ? push->per_episode : 0,
                                               target ? target->per_episode : 0};
    for (int s = 0; s < VDA_NAMES; ++s) A.adr_slot[s] = -1;
    for (int s = 0; s < VDA_NAMES; ++s) {
        const VineEnvAdrName& a = names[s];
        VineEnvDrawAdrSlot& sl = A.slot[s];
        sl.group = group_of(s);
        sl.row = row_of(s);
        sl.integer = integer_of(s) ? 1 : 0;
        if (group_names[sl.group]) sl.limits = group_names[sl.group][sl.row];
        if (a.reserved != 0) return bad_name(s, "reserved must be 0");
        if (!a.on) {
            if (a.start_lo != 0.0 || a.start_hi != 0.0 || a.step != 0.0) return bad_name(s, "START and STEP of a name that is not under ADR must be 0");
            continue;
        }
        if (!group_names[sl.group]) return bad_name(s, "a name under ADR needs its observer's spec: the observer is off");
        if (!group_per_episode[sl.group]) return bad_name(s, "a name under ADR needs PER_EPISODE of its observer: its values are never redrawn");
        const VineEnvRedrawName& lim = sl.limits;
        if (lim.form != VINE_REDRAW_RANGE) return bad_name(s, "a name under ADR must be a [lo, hi] range of its observer");
        if (!std::isfinite(a.start_lo) || !std::isfinite(a.start_hi) || a.start_lo > a.start_hi)
            return bad_name(s, "START needs finite lo <= hi");
        if (a.start_lo < lim.lo || a.start_hi > lim.hi) return bad_name(s, "START lies outside the limits, the name's range of its observer");
        if (!std::isfinite(a.step) || !(a.step > 0.0)) return bad_name(s, "STEP must be positive");
        if (integer_of(s) && (a.start_lo != std::floor(a.start_lo) || a.start_hi != std::floor(a.start_hi) || a.step != std::floor(a.step)))
            return bad_name(s, "an integer parameter takes an integer START and STEP");
        double m_lo = std::ceil((a.start_lo - lim.lo) / a.step), m_hi = std::ceil((lim.hi - a.start_hi) / a.step);
        if (a.start_lo - m_lo * a.step > lim.lo) m_lo += 1.0;      // the quotient was rounded down to a whole number: the last
        if (a.start_hi + m_hi * a.step < lim.hi) m_hi += 1.0;      // step must arrive AT the limit, not an ulp inside it
        if (m_lo > 1073741824.0 || m_hi > 1073741824.0) return bad_name(s, "more than 2^30 STEPs between START and a limit");
        sl.adr = a;
        sl.adr.on = 1;
        sl.max_widen[0] = (int32_t)m_lo;
        sl.max_widen[1] = (int32_t)m_hi;
        A.adr_slot[A.num_adr++] = s;
    }
    if (A.num_adr == 0) return vine_invalid_arg("env draw adr spec: no name is under ADR, there is no range to move");
    A.checked = 1u;
    *out = A;
    return VINE_OK;
}

int vine_env_draw_adr_scheduled(VineHandle* h, const VineEnvDrawAdrSpec* spec, const int64_t* reset,
                                float* const tables[VDA_GROUPS], const double* values, int32_t* widen, int32_t* counts,
                                int32_t* reached, int32_t* probe, int32_t* episode_index, int32_t* history, int64_t* cursor,
                                void* stream) {
    if (!h || !spec || !reset || !tables || !widen || !counts || !reached || !probe || !episode_index || !history || !cursor)
        return vine_invalid_arg("null argument to vine_env_draw_adr_scheduled");
    if (spec->abi_version != VINE_ENV_DRAW_ADR_ABI_VERSION) return vine_invalid_arg("VineEnvDrawAdrSpec.abi_version mismatch");
    if (spec->checked != 1u) return vine_invalid_arg("VineEnvDrawAdrSpec was not filled by vine_env_draw_adr_spec");
    if (spec->num_adr < 1 || spec->num_adr > VDA_NAMES || spec->history_capacity < 1)
        return vine_invalid_arg("VineEnvDrawAdrSpec lies outside what vine_env_draw_adr_spec fills");
    int on_count = 0;
    for (int s = 0; s < VDA_NAMES; ++s) {
        const VineEnvDrawAdrSlot& sl = spec->slot[s];
        if (sl.group != group_of(s) || sl.row != row_of(s) || sl.integer != (integer_of(s) ? 1 : 0))
            return vine_invalid_arg("VineEnvDrawAdrSpec lies outside what vine_env_draw_adr_spec fills");
        if (!sl.adr.on) continue;
        ++on_count;
        if (sl.limits.form != VINE_REDRAW_RANGE) return vine_invalid_arg("VineEnvDrawAdrSpec lies outside what vine_env_draw_adr_spec fills");
        if (!tables[sl.group]) {
            char msg[160];
            snprintf(msg, sizeof msg, "null argument to vine_env_draw_adr_scheduled: %s is under ADR and needs the table of %s", kNames[s],
                     kGroups[sl.group]);
            return vine_invalid_arg(msg);
        }
    }
    // (the kernel indexes adr_slot by j >> 1 < num_adr and the tables by what it reads there)
    if (on_count != spec->num_adr) return vine_invalid_arg("VineEnvDrawAdrSpec lies outside what vine_env_draw_adr_spec fills");
    for (int a = 0; a < spec->num_adr; ++a) {
        const int s = spec->adr_slot[a];
        if (s < 0 || s >= VDA_NAMES || !spec->slot[s].adr.on) return vine_invalid_arg("VineEnvDrawAdrSpec lies outside what vine_env_draw_adr_spec fills");
    }
    VineHandleInfo info;
    int rc = vine_handle_info(h, &info);
    if (rc) return rc;
    const float *bound_params = nullptr, *bound_inertia = nullptr;
    unsigned env_off = 0;
    rc = vine_env_tables_of(h, &bound_params, &bound_inertia, &env_off);
    if (rc) return rc;
    const float* rmat = vine_reward_matrix_of(h);
    if (!rmat)
        return vine_invalid_arg("vine_env_draw_adr_scheduled needs a reward matrix bound to the handle (vine_bind_reward_matrix) "
                                "before the step it rides behind");
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(vine_env_draw_adr_decide_kernel, dim3(1), dim3(64), 0, st, *spec, info.counters, info.glog, widen, counts, history,
                       (unsigned long long*)cursor);
    rc = vine_launch_status("vine_env_draw_adr_decide");
    if (rc) return rc;
    const int blocks = (info.n + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(vine_env_draw_adr_redraw_kernel, dim3(blocks), dim3(THREADS), 0, st, *spec, info.n, env_off, (const long long*)reset,
                       rmat, tables[VDA_SENSOR], tables[VDA_PUSH], tables[VDA_TARGET], values, episode_index, (const int*)widen, counts,
                       reached, probe);
    return vine_launch_status("vine_env_draw_adr_redraw");
}

}  // extern "C"
