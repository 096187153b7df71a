// vine_mpc_filter.hip — a fixed-gain corrector over the frames of the predictive controller's sensing path, for MI355X
// (gfx950): include/vine_mpc_filter.h states the semantics, utils/mpc_filter.py (filter_pin_replay, filter_correct_replay) is
// the same statement in numpy.
//
// Two elementwise kernels, one lane per PLANT, 256 lanes per workgroup, no LDS, over the SoA state blocks (st[f * m + p]: every
// field access of a wave is one contiguous segment) and the two rings snap[slot][f][p] and est[slot][f][p], which have the
// block's layout per slot.  M-wide launches are latency-sized: a lane moves one column of 44 floats (nine of them for an
// episode's first frame) and a few words.  Both read the PLANT's step counter as the observers do (vine_observer.h
// vine_steps_completed); the pin reads the predictor's too.  No atomics anywhere; plain C++ stores only.
//
// CONTRACTION IS OFF FOR THIS TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it with
// -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): `x + g * v` must stay a multiply and an add, each
// rounded, as numpy forms it, and so must the sums of squares.  The one exception is vine_task_shared.h, included under
// contract(fast): task_new_command must give the words the step kernels put into the delay ring, and tip_fk_joint the words
// the measurement (vine_mpc_observe.hip) derives from a joint state.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/vine_env_params.h"
#include "../../include/vine_mpc_filter.h"
#include "vine_observer.h"
#include "vine_policy_head.h"
#pragma clang fp contract(fast)
#include "vine_task_shared.h"
#pragma clang fp contract(off)
#include "vine_mpc_shared.h"

namespace {

constexpr int THREADS = VINE_MPC_FILTER_THREADS;
constexpr int SLOTS = VINE_MPC_OBSERVE_SLOTS;
constexpr int LOG = VINE_MPC_OBSERVE_LOG;
constexpr int NQ = VINE_NUM_DOFS;
static_assert(VF_QD0 == VF_Q0 + NQ && VF_PREV_TIP_Y == VF_PREV_Q0 + NQ, "six q, six qd, six previous q");
static_assert(LOG == 2 * VINE_MAX_DELAY, "act_log[p][dd] lies inside the log, and dd + a reaches its end only with both at VINE_MAX_DELAY");

struct FilterParams {
    int m;
    int plant_glog, glog, delay;           // the PLANT's counter shift; the PREDICTOR's counter shift and ACTION_DELAY
    unsigned seed_lo, seed_hi;
    float L, z1, s0, c0;                   // the plant configuration's, for tip_fk_joint
    CommandParams cmd;                     // the predictor configuration's
};

__device__ __forceinline__ int clamp_delay(int v) { return min(max(v, 0), VINE_MAX_DELAY); }

// known, dd and e of plant p (include/vine_mpc_filter.h, NOTATION); cp = the plant's steps completed.
__device__ __forceinline__ long long filter_frame_step(const FilterParams& S, int p, unsigned long long cp,
                                                       const float* __restrict__ table, const int* __restrict__ age,
                                                       const unsigned char* __restrict__ fresh, bool& known, int& dd) {
    known = fresh[p] != 0 || cp == 0ull;
    dd = known ? 0 : min(clamp_delay((int)table[(size_t)VMO_DELAY * S.m + p]), clamp_delay(age[p]));
    return (long long)cp - 1ll - (long long)dd;
}

// step mod SLOTS, inside the ring whatever the caller's age and est_index hold
__device__ __forceinline__ int slot_of(long long step) { return (int)((step % (long long)SLOTS + SLOTS) % SLOTS); }

__global__ __launch_bounds__(THREADS) void vine_mpc_filter_pin_kernel(
    const FilterParams S, const float* __restrict__ pst, const unsigned long long* __restrict__ plant_counters,
    float* __restrict__ st, const unsigned long long* __restrict__ counters, const float* __restrict__ env_params,
    const float* __restrict__ table, const long long* __restrict__ plant_progress, const float* __restrict__ est,
    const long long* __restrict__ est_index, const float* __restrict__ act_log, const int* __restrict__ age,
    const unsigned char* __restrict__ fresh, float* __restrict__ actions, float* __restrict__ rew,
    long long* __restrict__ reset, long long* __restrict__ progress) {
    const unsigned long long cp = vine_steps_completed(plant_counters, S.plant_glog);
    const unsigned long long c = vine_steps_completed(counters, S.glog);
    const int m = S.m, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    bool known;
    int dd;
    const long long e = filter_frame_step(S, p, cp, table, age, fresh, known, dd);
    const long long have = est_index[p];
    const size_t slot_floats = (size_t)VF_COUNT * m;
    const float2* __restrict__ log = reinterpret_cast<const float2*>(act_log) + (size_t)p * LOG;
    if (!known && age[p] != 0 && have >= 0 && have == e - 1) {
        const float* __restrict__ src = est + (size_t)slot_of(e - 1) * slot_floats;
        MPC_COPY_COLUMN(src, m, p, st, m, p);
        // the delay ring in front of step e: this env's delay and action -> command constants, as the observe pin reads them
        CommandParams P = S.cmd;
        int a = S.delay;
        if (env_params) {
            P.rail_scale = env_params[(size_t)VP_RAIL_VELOCITY_SCALE * m + p];
            a = clamp_delay((int)env_params[(size_t)VP_ACTION_DELAY * m + p]);
        }
        // mpc_rebuild_ring indexes its history by a loop of run-time length: a local copy of the log would live in scratch.  So
        // the log itself is handed over wherever it reaches far enough, and a copy is formed only where its end is reached, with a
        // ring length that is a constant there (registers again).
        if (dd + a < LOG) {                                    // act_log[p][dd + 1 .. dd + a] lie inside the log
            mpc_rebuild_ring(P, a, c, log + dd + 1, st, m, p);
        } else {                                               // dd = a = VINE_MAX_DELAY: the last entry reads (0, 0)
            float2 hist[VINE_MAX_DELAY];
#pragma unroll
            for (int k = 0; k < VINE_MAX_DELAY - 1; ++k) hist[k] = log[VINE_MAX_DELAY + 1 + k];
            hist[VINE_MAX_DELAY - 1] = make_float2(0.0f, 0.0f);
            mpc_rebuild_ring(P, VINE_MAX_DELAY, c, hist, st, m, p);
        }
        progress[p] = plant_progress[p] - (long long)dd - 1ll;
        reset[p] = 0;
        rew[p] = 0.0f;
        reinterpret_cast<float2*>(actions)[p] = log[dd];
    } else {
        const float* __restrict__ src = pst;
        if (!known && have >= 0 && have == e) src = est + (size_t)slot_of(e) * slot_floats;
        MPC_COPY_COLUMN(src, m, p, st, m, p);
        reinterpret_cast<float2*>(actions)[p] = make_float2(0.0f, 0.0f);
    }
}

__global__ __launch_bounds__(THREADS) void vine_mpc_filter_correct_kernel(
    const FilterParams S, const unsigned long long* __restrict__ plant_counters, const float* __restrict__ st,
    const float* __restrict__ table, const float* __restrict__ gain, const float* __restrict__ snap,
    const int* __restrict__ age, const unsigned char* __restrict__ fresh, float* __restrict__ est,
    long long* __restrict__ est_index, float* __restrict__ innov) {
    const unsigned long long cp = vine_steps_completed(plant_counters, S.plant_glog);
    const int m = S.m, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    bool known;
    int dd;
    const long long e = filter_frame_step(S, p, cp, table, age, fresh, known, dd);
    if (known) {                                               // a.
        est_index[p] = -1;
        return;
    }
    const size_t slot_floats = (size_t)VF_COUNT * m;
    if (age[p] == 0) {                                         // b. (dd == 0: e is s)
        const float* __restrict__ y = snap + (size_t)slot_of(e) * slot_floats;
        float col[VF_COUNT];                                   // the frame read once (registers: every index below is a constant)
        MPC_COPY_COLUMN(y, m, p, col, 1, 0);
#pragma unroll 1
        for (int k = 0; k < SLOTS; ++k) {
            float* __restrict__ dst = est + (size_t)k * slot_floats;
            MPC_COPY_COLUMN(col, 1, 0, dst, m, p);
        }
        est_index[p] = e;
        innov[p] = 0.0f;
        innov[(size_t)m + p] = 0.0f;
        return;
    }
    const long long have = est_index[p];
    if (have == e) return;                                     // c.
    const float* __restrict__ y = snap + (size_t)slot_of(e) * slot_floats;
    float* __restrict__ dst = est + (size_t)slot_of(e) * slot_floats;
    est_index[p] = e;
    if (!(have >= 0 && have == e - 1)) {                       // e.
        MPC_COPY_COLUMN(y, m, p, dst, m, p);
        return;
    }
    // d. the hold draw of the measurement behind step e, read again
    unsigned w[4];
    const unsigned long long ue = (unsigned long long)e;
    philox4x32_10((unsigned)p, (unsigned)ue, VINE_MPC_FILTER_HOLD_PURPOSE | ((unsigned)(ue >> 32) << 8), 0u, S.seed_lo, S.seed_hi, w);
    if (u01(w[0]) < table[(size_t)VMO_HOLD * m + p]) {         // predicted through
        MPC_COPY_COLUMN(st, m, p, dst, m, p);
        innov[p] = 0.0f;
        innov[(size_t)m + p] = 0.0f;
        return;
    }
    const float gq = gain[(size_t)VMF_GAIN_Q * m + p], gqd = gain[(size_t)VMF_GAIN_QD * m + p];
    float xq[NQ], xqd[NQ], vq[NQ], vqd[NQ];
    float sum_q = 0.0f, sum_qd = 0.0f;
    bool moved = false;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        xq[i] = st[(size_t)(VF_Q0 + i) * m + p];
        xqd[i] = st[(size_t)(VF_QD0 + i) * m + p];
        vq[i] = y[(size_t)(VF_Q0 + i) * m + p] - xq[i];
        vqd[i] = y[(size_t)(VF_QD0 + i) * m + p] - xqd[i];
        const float sq = vq[i] * vq[i], sqd = vqd[i] * vqd[i];
        sum_q = sum_q + sq;
        sum_qd = sum_qd + sqd;
        moved = moved || vq[i] != 0.0f || vqd[i] != 0.0f;
    }
    innov[p] = sum_q;
    innov[(size_t)m + p] = sum_qd;
    MPC_COPY_COLUMN(y, m, p, dst, m, p);                       // what is recorded exactly; with both gains 1 the whole frame
    if (gq == 1.0f && gqd == 1.0f) return;
    if (!moved) {                                              // the prediction's own words for what the joints determine
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            dst[(size_t)(VF_Q0 + i) * m + p] = xq[i];
            dst[(size_t)(VF_QD0 + i) * m + p] = xqd[i];
            dst[(size_t)(VF_PREV_Q0 + i) * m + p] = st[(size_t)(VF_PREV_Q0 + i) * m + p];
        }
        for (int f = VF_TIP_Y; f <= VF_CART_VY; ++f) dst[(size_t)f * m + p] = st[(size_t)f * m + p];
        dst[(size_t)VF_PREV_TIP_Y * m + p] = st[(size_t)VF_PREV_TIP_Y * m + p];
        dst[(size_t)VF_PREV_TIP_Z * m + p] = st[(size_t)VF_PREV_TIP_Z * m + p];
        dst[(size_t)VF_PREV_CART_VEL * m + p] = st[(size_t)VF_PREV_CART_VEL * m + p];
        return;
    }
    float q[NQ], qd[NQ], tip[4];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const float cq = gq * vq[i], cqd = gqd * vqd[i];
        q[i] = xq[i] + cq;
        qd[i] = xqd[i] + cqd;
    }
    tip_fk_joint(q, qd, S.L, S.z1, S.s0, S.c0, tip);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        dst[(size_t)(VF_Q0 + i) * m + p] = q[i];
        dst[(size_t)(VF_QD0 + i) * m + p] = qd[i];
        dst[(size_t)(VF_PREV_Q0 + i) * m + p] = q[i];
    }
    dst[(size_t)VF_TIP_Y * m + p] = tip[0]; dst[(size_t)VF_TIP_Z * m + p] = tip[1];
    dst[(size_t)VF_TIP_VY * m + p] = tip[2]; dst[(size_t)VF_TIP_VZ * m + p] = tip[3];
    dst[(size_t)VF_CART_Y * m + p] = q[0]; dst[(size_t)VF_CART_VY * m + p] = qd[0];
    dst[(size_t)VF_PREV_TIP_Y * m + p] = tip[0]; dst[(size_t)VF_PREV_TIP_Z * m + p] = tip[1];
    dst[(size_t)VF_PREV_CART_VEL * m + p] = qd[0];
}
static_assert(VF_TIP_Y + 4 == VF_CART_Y && VF_CART_VY == VF_CART_Y + 1, "tip, tip velocity, cart: six fields in a row");

int validate(const VineMpcObserveConfig* c) {
    if (!c) return vine_invalid_arg("mpc filter: the observe config is NULL");
    if (c->abi_version != VINE_MPC_OBSERVE_ABI_VERSION) return vine_invalid_arg("mpc filter: VineMpcObserveConfig.abi_version mismatch");
    if (c->num_plants < 1) return vine_invalid_arg("mpc filter: num_plants must be at least 1");
    return VINE_OK;
}

// Both handles' part of a launch's parameters, and every refusal of a pair the observe pin would refuse.
int prepare(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* cfg, VineHandleInfo& pinfo, VineHandleInfo& info,
            FilterParams& S) {
    if (plant == predictor) return vine_invalid_arg("mpc filter: the plant and the predictor must be two handles");
    int rc = vine_handle_info(plant, &pinfo);
    if (rc) return rc;
    if (pinfo.n != cfg->num_plants) return vine_invalid_arg("mpc filter: the plant handle does not have num_plants envs");
    rc = vine_handle_info(predictor, &info);
    if (rc) return rc;
    if (info.n != cfg->num_plants) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc filter: the predictor handle has %d envs, not num_plants = %d", info.n, cfg->num_plants);
        return vine_invalid_arg(msg);
    }
    rc = mpc_stand_in("mpc filter", "predictor", "a replayed step must be a deterministic one", pinfo, info);
    if (rc) return rc;
    S = FilterParams{};
    S.m = cfg->num_plants; S.plant_glog = pinfo.glog; S.glog = info.glog; S.delay = info.delay;
    S.seed_lo = (unsigned)cfg->seed; S.seed_hi = (unsigned)(cfg->seed >> 32);
    S.L = pinfo.L; S.z1 = pinfo.z1; S.s0 = pinfo.s0; S.c0 = pinfo.c0;
    S.cmd = mpc_command_params(info);
    return VINE_OK;
}

}  // namespace

extern "C" {

int vine_mpc_filter_abi_version(void) { return VINE_MPC_FILTER_ABI_VERSION; }

int vine_mpc_filter_pin(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* cfg, const float* table,
                        const int64_t* plant_progress, const float* est, const int64_t* est_index, const float* act_log,
                        const int32_t* age, const uint8_t* fresh, float* actions, float* rew, int64_t* reset, int64_t* progress,
                        void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!plant || !predictor || !table || !plant_progress || !est || !est_index || !act_log || !age || !fresh || !actions || !rew ||
        !reset || !progress)
        return vine_invalid_arg("null argument to vine_mpc_filter_pin");
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(act_log)) & 7u)
        return vine_invalid_arg("mpc filter actions and act_log must be 8-byte aligned");
    VineHandleInfo pinfo, info;
    FilterParams S;
    rc = prepare(plant, predictor, cfg, pinfo, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_filter_pin_kernel, dim3((S.m + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, S,
                       (const float*)pinfo.state, pinfo.counters, info.state, info.counters, info.env_params, table,
                       (const long long*)plant_progress, est, (const long long*)est_index, act_log, age, fresh, actions, rew,
                       (long long*)reset, (long long*)progress);
    return vine_launch_status("vine_mpc_filter_pin");
}

int vine_mpc_filter_correct(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* cfg, const float* table,
                            const float* gain, const float* snap, const int32_t* age, const uint8_t* fresh, float* est,
                            int64_t* est_index, float* innov, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!plant || !predictor || !table || !gain || !snap || !age || !fresh || !est || !est_index || !innov)
        return vine_invalid_arg("null argument to vine_mpc_filter_correct");
    VineHandleInfo pinfo, info;
    FilterParams S;
    rc = prepare(plant, predictor, cfg, pinfo, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_filter_correct_kernel, dim3((S.m + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream,
                       S, pinfo.counters, (const float*)info.state, table, gain, snap, age, fresh, est, (long long*)est_index, innov);
    return vine_launch_status("vine_mpc_filter_correct");
}

}  // extern "C"
