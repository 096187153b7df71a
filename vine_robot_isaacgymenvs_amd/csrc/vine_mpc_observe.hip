// vine_mpc_observe.hip — the predictive controller's sensing path for MI355X (gfx950): include/vine_mpc_observe.h states the
// semantics, utils/mpc_observe.py (measure_replay, pin_replay, catchup_schedule) is the same statement in numpy.
//
// Three elementwise kernels, one lane per PLANT, 256 lanes per workgroup, no LDS, over the SoA state blocks (st[f * m + p]:
// every field access of a wave is one contiguous segment) and the frame ring snap[slot][f][p], which has the block's layout
// per slot.  M-wide launches are latency-sized: a lane moves one column of 44 floats (nine of them for an episode's first
// frame), sixteen actions and a few words.  vine_mpc_observe_measure_kernel reads the PLANT's step counter as the other
// observers do (vine_observer.h vine_steps_completed); the pin and the catch-up node read the plant's and the predictor's.
// The pin and the node's re-pin are one device function, observe_pin_plant.  No atomics anywhere; plain C++ stores only.
//
// CONTRACTION IS OFF FOR THIS TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it with
// -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): `q + z * c` must stay a multiply and an add, each
// rounded, as numpy forms it.  The one exception is vine_task_shared.h, included under contract(fast): task_new_command must
// give the words the step kernels put into the delay ring, and tip_fk_joint the words vine_sysid_pin (compiled with
// -ffp-contract=fast) derives from a joint state.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/vine_env_params.h"
#include "../../include/vine_mpc_observe.h"
#include "vine_observer.h"
#include "vine_policy_head.h"
#pragma clang fp contract(fast)
#include "vine_task_shared.h"
#pragma clang fp contract(off)
#include "vine_mpc_shared.h"

namespace {

constexpr int THREADS = VINE_MPC_OBSERVE_THREADS;
constexpr int SLOTS = VINE_MPC_OBSERVE_SLOTS;
constexpr int LOG = VINE_MPC_OBSERVE_LOG;
constexpr int NQ = VINE_NUM_DOFS;
static_assert(VF_QD0 == VF_Q0 + NQ && VF_PREV_TIP_Y == VF_PREV_Q0 + NQ, "six q, six qd, six previous q");
static_assert(LOG == 2 * VINE_MAX_DELAY && SLOTS == VINE_MAX_DELAY + 1, "sensor delay plus action delay fit the log");

struct ObserveParams {
    int m, C, compensate;
    int plant_glog, glog, delay;           // the PLANT's counter shift; the PREDICTOR's counter shift and ACTION_DELAY
    unsigned seed_lo, seed_hi;
    double k0;                             // 1 / sqrt(32 * (65536^2 - 1) / 12)
    float L, z1, s0, c0;                   // the plant configuration's, for tip_fk_joint
    CommandParams cmd;                     // the predictor configuration's
};


__device__ __forceinline__ int clamp_delay(int v) { return min(max(v, 0), VINE_MAX_DELAY); }

// x + z * c with z the eight-uniform deviate of counter (p, s, VINE_MPC_OBSERVE_RNG_NOISE | hi_word, field).
__device__ __forceinline__ float noisy_value(const ObserveParams& S, unsigned p, unsigned long long s, unsigned field, float x,
                                             float c) {
    unsigned w[4];
    philox4x32_10(p, (unsigned)s, VINE_MPC_OBSERVE_RNG_NOISE | ((unsigned)(s >> 32) << 8), field, S.seed_lo, S.seed_hi, w);
    const float z = (float)mpc_deviate_int(w);
    const float zc = z * c;
    return x + zc;
}

__global__ __launch_bounds__(THREADS) void vine_mpc_observe_measure_kernel(
    const ObserveParams S, const float* __restrict__ pst, const unsigned long long* __restrict__ plant_counters,
    const float* __restrict__ table, const long long* __restrict__ plant_progress, const float* __restrict__ plant_actions,
    float* __restrict__ snap, float* __restrict__ act_log, int* __restrict__ age, unsigned char* __restrict__ fresh) {
    const unsigned long long c = vine_steps_completed(plant_counters, S.plant_glog);
    if (c == 0ull) return;
    const int m = S.m, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const unsigned long long s = c - 1ull;
    const float hold = table[(size_t)VMO_HOLD * m + p];
    const float sq = table[(size_t)VMO_NOISE_Q * m + p], sqd = table[(size_t)VMO_NOISE_QD * m + p];
    const bool noisy = sq != 0.0f || sqd != 0.0f;
    const bool first = plant_progress[p] == 0 || fresh[p] != 0;

    float q[NQ], qd[NQ], tip[4];
    if (noisy) {
        const float cq = (float)((double)sq * S.k0), cqd = (float)((double)sqd * S.k0);
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            q[i] = pst[(size_t)(VF_Q0 + i) * m + p];
            qd[i] = pst[(size_t)(VF_QD0 + i) * m + p];
            if (sq != 0.0f) q[i] = noisy_value(S, (unsigned)p, s, (unsigned)i, q[i], cq);
            if (sqd != 0.0f) qd[i] = noisy_value(S, (unsigned)p, s, (unsigned)(NQ + i), qd[i], cqd);
        }
        tip_fk_joint(q, qd, S.L, S.z1, S.s0, S.c0, tip);
    }
    const size_t slot_floats = (size_t)VF_COUNT * m;
    // the frame into one slot: the column, then -- for a noisy plant -- the joint fields and what they determine
    auto store_frame = [&](int slot) {
        float* __restrict__ dst = snap + (size_t)slot * slot_floats;
        MPC_COPY_COLUMN(pst, m, p, dst, m, p);
        if (noisy) {
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
    };
    const int cur = (int)(s % (unsigned long long)SLOTS);
    if (first) {
#pragma unroll 1
        for (int k = 0; k < SLOTS; ++k) store_frame(k);
        age[p] = 0;
        fresh[p] = 0;
    } else {
        unsigned w[4];
        philox4x32_10((unsigned)p, (unsigned)s, VINE_MPC_OBSERVE_RNG_HOLD | ((unsigned)(s >> 32) << 8), 0u, S.seed_lo, S.seed_hi, w);
        const bool held = u01(w[0]) < hold;
        if (held) {
            const float* __restrict__ src = snap + (size_t)((cur + SLOTS - 1) % SLOTS) * slot_floats;
            float* __restrict__ dst = snap + (size_t)cur * slot_floats;
            MPC_COPY_COLUMN(src, m, p, dst, m, p);
        } else {
            store_frame(cur);
        }
        age[p] = min(max(age[p], 0) + 1, VINE_MAX_DELAY);
    }
    float2* __restrict__ log = reinterpret_cast<float2*>(act_log) + (size_t)p * LOG;
    for (int i = LOG - 1; i > 0; --i) log[i] = log[i - 1];
    log[0] = reinterpret_cast<const float2*>(plant_actions)[p];
}

// Which frame plant p is delivered (include/vine_mpc_observe.h, 2.): `known`, the plant's own column while nothing has been
// measured; else the frame dd steps behind the last one.  Returns d, the steps of it that are predicted forward.
__device__ __forceinline__ int observe_delivered(const ObserveParams& S, int p, unsigned long long cp,
                                                 const float* __restrict__ table, const int* __restrict__ age,
                                                 const unsigned char* __restrict__ fresh, bool& known, int& dd) {
    known = fresh[p] != 0 || cp == 0ull;
    dd = known ? 0 : min(clamp_delay((int)table[(size_t)VMO_DELAY * S.m + p]), clamp_delay(age[p]));
    return S.compensate ? min(dd, S.C) : 0;
}

// The action of the predictor's step i + 1 (3.): i < C.
__device__ __forceinline__ float2 observe_next_action(const ObserveParams& S, int i, int d, const float2* __restrict__ log) {
    return i >= S.C - d ? log[S.C - i - 1] : make_float2(0.0f, 0.0f);
}

// The pin, and the catch-up node's re-pin, of plant p: cp and c are the plant's and the predictor's steps completed.
__device__ __forceinline__ void observe_pin_plant(const ObserveParams& S, int p, unsigned long long cp, unsigned long long c,
                                                  bool known, int dd, int d, const float* __restrict__ pst,
                                                  float* __restrict__ st, const float* __restrict__ env_params,
                                                  const long long* __restrict__ plant_progress, const float* __restrict__ snap,
                                                  const float2* __restrict__ log, float* __restrict__ rew,
                                                  long long* __restrict__ reset, long long* __restrict__ progress,
                                                  int* __restrict__ lag) {
    const int m = S.m;
    // the delivered frame: the plant's own column while nothing has been measured, else slot (s - dd) mod SLOTS, s = cp - 1
    const float* __restrict__ src = pst;
    if (!known) {
        const int cur = (int)((cp - 1ull) % (unsigned long long)SLOTS);
        src = snap + (size_t)((cur + SLOTS - dd) % SLOTS) * VF_COUNT * m;
    }
    MPC_COPY_COLUMN(src, m, p, st, m, p);
    // the delay ring: this env's delay and action -> command constants (the step's env_params_of, vine_hip.hip)
    CommandParams P = S.cmd;
    int a = S.delay;
    if (env_params) {
        P.rail_scale = env_params[(size_t)VP_RAIL_VELOCITY_SCALE * m + p];
        a = clamp_delay((int)env_params[(size_t)VP_ACTION_DELAY * m + p]);
    }
    mpc_rebuild_ring(P, a, c, log + d, st, m, p);
    progress[p] = plant_progress[p] - (long long)dd;
    reset[p] = 0;
    rew[p] = 0.0f;
    lag[p] = d;
}

// i == 0: the pin.  1 <= i <= C: the node behind the predictor's i-th step.
__global__ __launch_bounds__(THREADS) void vine_mpc_observe_pin_kernel(
    const ObserveParams S, const int i, const float* __restrict__ pst, const unsigned long long* __restrict__ plant_counters,
    float* __restrict__ st, const unsigned long long* __restrict__ counters, const float* __restrict__ env_params,
    const float* __restrict__ table, const long long* __restrict__ plant_progress, const float* __restrict__ snap,
    const float* __restrict__ act_log, const int* __restrict__ age, const unsigned char* __restrict__ fresh,
    float* __restrict__ actions, float* __restrict__ rew, long long* __restrict__ reset, long long* __restrict__ progress,
    int* __restrict__ lag) {
    const unsigned long long cp = vine_steps_completed(plant_counters, S.plant_glog);
    const unsigned long long c = vine_steps_completed(counters, S.glog);
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S.m) return;
    bool known;
    int dd;
    const int d = observe_delivered(S, p, cp, table, age, fresh, known, dd);
    const float2* __restrict__ log = reinterpret_cast<const float2*>(act_log) + (size_t)p * LOG;
    if (i <= S.C - d)          // (the pin itself, or a step that did not count)
        observe_pin_plant(S, p, cp, c, known, dd, d, pst, st, env_params, plant_progress, snap, log, rew, reset, progress, lag);
    else                       // a real step: the plant is known to be inside its episode
        reset[p] = 0;
    if (i < S.C) reinterpret_cast<float2*>(actions)[p] = observe_next_action(S, i, d, log);
}

int validate(const VineMpcObserveConfig* c) {
    if (!c) return vine_invalid_arg("mpc observe config is NULL");
    if (c->abi_version != VINE_MPC_OBSERVE_ABI_VERSION) return vine_invalid_arg("VineMpcObserveConfig.abi_version mismatch");
    if (c->num_plants < 1) return vine_invalid_arg("mpc observe num_plants must be at least 1");
    if (c->catchup < 0 || c->catchup > VINE_MAX_DELAY)
        return vine_invalid_arg("mpc observe needs 0 <= catchup <= VINE_MAX_DELAY (8)");
    if (c->compensate != 0 && c->compensate != 1) return vine_invalid_arg("mpc observe compensate must be 0 or 1");
    return VINE_OK;
}

// The plant handle's part of a launch's parameters; refuses a handle that does not hold num_plants envs.
int prepare_plant(VineHandle* plant, const VineMpcObserveConfig* cfg, VineHandleInfo& pinfo, ObserveParams& S) {
    int rc = vine_handle_info(plant, &pinfo);
    if (rc) return rc;
    if (pinfo.n != cfg->num_plants) return vine_invalid_arg("mpc observe: the plant handle does not have num_plants envs");
    S = ObserveParams{};
    S.m = cfg->num_plants; S.C = cfg->catchup; S.compensate = cfg->compensate; S.plant_glog = pinfo.glog;
    S.seed_lo = (unsigned)cfg->seed; S.seed_hi = (unsigned)(cfg->seed >> 32);
    S.k0 = noise_scale();
    S.L = pinfo.L; S.z1 = pinfo.z1; S.s0 = pinfo.s0; S.c0 = pinfo.c0;
    return VINE_OK;
}

// The predictor's part, and every refusal of a predictor that could not stand in for the plant.
int prepare_predictor(VineHandle* predictor, const VineMpcObserveConfig* cfg, const VineHandleInfo& pinfo, VineHandleInfo& info,
                      ObserveParams& S) {
    int rc = vine_handle_info(predictor, &info);
    if (rc) return rc;
    if (info.n != cfg->num_plants) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc observe: the predictor handle has %d envs, not num_plants = %d", info.n, cfg->num_plants);
        return vine_invalid_arg(msg);
    }
    rc = mpc_stand_in("mpc observe", "predictor", "a replayed step must be a deterministic one", pinfo, info);
    if (rc) return rc;
    S.glog = info.glog; S.delay = info.delay;
    S.cmd = mpc_command_params(info);
    return VINE_OK;
}

int launch_pin(const char* what, int i, VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* cfg,
               const float* table, const int64_t* plant_progress, const float* snap, const float* act_log, const int32_t* age,
               const uint8_t* fresh, float* actions, float* rew, int64_t* reset, int64_t* progress, int32_t* lag, void* stream) {
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(act_log)) & 7u)
        return vine_invalid_arg("mpc observe actions and act_log must be 8-byte aligned");
    if (plant == predictor) return vine_invalid_arg("mpc observe: the plant and the predictor must be two handles");
    VineHandleInfo pinfo, info;
    ObserveParams S;
    int rc = prepare_plant(plant, cfg, pinfo, S);
    if (rc) return rc;
    rc = prepare_predictor(predictor, cfg, pinfo, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_observe_pin_kernel, dim3((S.m + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, S,
                       i, (const float*)pinfo.state, pinfo.counters, info.state, info.counters, info.env_params, table,
                       (const long long*)plant_progress, snap, act_log, age, fresh, actions, rew, (long long*)reset,
                       (long long*)progress, lag);
    return vine_launch_status(what);
}

}  // namespace

extern "C" {

int vine_mpc_observe_config_default(VineMpcObserveConfig* c) {
    if (!c) return vine_invalid_arg("mpc observe config is NULL");
    *c = VineMpcObserveConfig{};
    c->abi_version = VINE_MPC_OBSERVE_ABI_VERSION;
    c->compensate = 1;
    return VINE_OK;
}

int vine_mpc_observe_config_size(void) { return (int)sizeof(VineMpcObserveConfig); }

int vine_mpc_observe_measure(VineHandle* plant, const VineMpcObserveConfig* cfg, const float* table,
                             const int64_t* plant_progress, const float* plant_actions, float* snap, float* act_log,
                             int32_t* age, uint8_t* fresh, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!plant || !table || !plant_progress || !plant_actions || !snap || !act_log || !age || !fresh)
        return vine_invalid_arg("null argument to vine_mpc_observe_measure");
    if ((reinterpret_cast<uintptr_t>(plant_actions) | reinterpret_cast<uintptr_t>(act_log)) & 7u)
        return vine_invalid_arg("mpc observe plant_actions and act_log must be 8-byte aligned");
    VineHandleInfo pinfo;
    ObserveParams S;
    rc = prepare_plant(plant, cfg, pinfo, S);
    if (rc) return rc;
    VineDeviceScope scope(pinfo.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_observe_measure_kernel, dim3((S.m + THREADS - 1) / THREADS), dim3(THREADS), 0,
                       (hipStream_t)stream, S, (const float*)pinfo.state, pinfo.counters, table, (const long long*)plant_progress,
                       plant_actions, snap, act_log, age, fresh);
    return vine_launch_status("vine_mpc_observe_measure");
}

int vine_mpc_observe_pin(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* cfg, const float* table,
                         const int64_t* plant_progress, const float* snap, const float* act_log, const int32_t* age,
                         const uint8_t* fresh, float* actions, float* rew, int64_t* reset, int64_t* progress, int32_t* lag,
                         void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!plant || !predictor || !table || !plant_progress || !snap || !act_log || !age || !fresh || !actions || !rew || !reset ||
        !progress || !lag)
        return vine_invalid_arg("null argument to vine_mpc_observe_pin");
    return launch_pin("vine_mpc_observe_pin", 0, plant, predictor, cfg, table, plant_progress, snap, act_log, age, fresh, actions,
                      rew, reset, progress, lag, stream);
}

int vine_mpc_observe_catchup(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* cfg, int32_t step_index,
                             const float* table, const int64_t* plant_progress, const float* snap, const float* act_log,
                             const int32_t* age, const uint8_t* fresh, float* actions, float* rew, int64_t* reset,
                             int64_t* progress, int32_t* lag, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!plant || !predictor || !table || !plant_progress || !snap || !act_log || !age || !fresh || !actions || !rew || !reset ||
        !progress || !lag)
        return vine_invalid_arg("null argument to vine_mpc_observe_catchup");
    if (step_index < 1 || step_index > cfg->catchup)
        return vine_invalid_arg("mpc observe catchup needs 1 <= step_index <= catchup");
    return launch_pin("vine_mpc_observe_catchup", step_index, plant, predictor, cfg, table, plant_progress, snap, act_log, age,
                      fresh, actions, rew, reset, progress, lag, stream);
}

}  // extern "C"
