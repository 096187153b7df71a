// vine_sysid.hip — system identification (SYSID) for MI355X (gfx950): include/vine_sysid.h.
//
// Two elementwise kernels, one lane per env, 256 lanes per workgroup, over the SoA state block (st[f * n + e]: every field
// access of a wave is one contiguous segment).  The log row a launch works on is the same for every lane -- its index comes
// from the handle's step counter and the two window words, all uniform -- so its floats are scalar loads.
//
// vine_sysid_pin_kernel writes the pose of a log row into every env and fills each env's delay ring with the commands the
// log's last d actions would have left; the command is task_new_command<false> and the tip is tip_fk_joint, both of
// vine_task_shared.h, the functions the step kernels and the recorder call.
// vine_sysid_node_kernel reads the step counter exactly as the other observers do (vine_observer.h vine_steps_completed) and returns at once
// outside the window.  Inside, a lane reads its env's 12 joint-state fields, adds its weighted squared distance from the log
// row to err[e] in float64 and stores the next action: at most 65 B read (12 floats, err, the reset flag, alive) and 17 B
// written per env and step.
// No atomics, no LDS, no cross-lane operation; plain C++ stores only.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/vine_env_params.h"
#include "../../include/vine_sysid.h"
#include "vine_observer.h"
#include "vine_task_shared.h"

namespace {

constexpr int THREADS = 256;
static_assert(VINE_SYSID_FIELDS == VRF_TIP_VZ + 1 && VRF_Q0 == 0 && VRF_QD0 == VINE_NUM_DOFS, "the compared fields lead the row");

// What task_new_command reads (vine_task_shared.h).
struct CommandParams {
    float clip_act, act_noise, rail_scale, fpam_span, fpam_min;
};

struct SysidParams {
    int n, glog, T, H, delay;
    long long row;                         // the pin only
    float L, z1, s0, c0;
    CommandParams cmd;                     // the configuration's
    float w[VINE_SYSID_FIELDS];            // the node only
};

#define ST(f) st[(size_t)(f) * n + e]

__global__ __launch_bounds__(THREADS) void vine_sysid_pin_kernel(const SysidParams S, float* __restrict__ st,
                                                                 const unsigned long long* __restrict__ counters,
                                                                 const float* __restrict__ env_params,
                                                                 const float* __restrict__ log, float* __restrict__ actions,
                                                                 float* __restrict__ rew, long long* __restrict__ reset,
                                                                 long long* __restrict__ progress,
                                                                 long long* __restrict__ window) {
    const unsigned long long c = vine_steps_completed(counters, S.glog);
    const int n = S.n, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) {
        window[0] = (long long)c;
        window[1] = S.row;
    }
    if (e >= n) return;
    const float* __restrict__ Lr = log + S.row * VINE_RECORD_FIELDS;      // (the host checked 0 <= row, row + H < T)
    float q[VINE_NUM_DOFS], qd[VINE_NUM_DOFS], tip[4];
#pragma unroll
    for (int i = 0; i < VINE_NUM_DOFS; ++i) {
        q[i] = Lr[VRF_Q0 + i];
        qd[i] = Lr[VRF_QD0 + i];
    }
    tip_fk_joint(q, qd, S.L, S.z1, S.s0, S.c0, tip);
#pragma unroll
    for (int i = 0; i < VINE_NUM_DOFS; ++i) {
        ST(VF_Q0 + i) = q[i];
        ST(VF_QD0 + i) = qd[i];
        ST(VF_PREV_Q0 + i) = q[i];
    }
    ST(VF_TIP_Y) = tip[0]; ST(VF_TIP_Z) = tip[1]; ST(VF_TIP_VY) = tip[2]; ST(VF_TIP_VZ) = tip[3];
    ST(VF_CART_Y) = q[0]; ST(VF_CART_VY) = qd[0];
    ST(VF_PREV_TIP_Y) = tip[0]; ST(VF_PREV_TIP_Z) = tip[1];
    ST(VF_SMOOTHED_U) = Lr[VRF_SMOOTHED_U];
    ST(VF_PREV_CART_VEL) = qd[0];
    ST(VF_PREV_CART_VEL_ERR) = 0.0f;
    ST(VF_PREV_U_RAIL) = 0.0f;
    ST(VF_AGG_REW) = 0.0f;
    ST(VF_TARGET_Y) = Lr[VRF_TARGET_Y]; ST(VF_TARGET_Z) = Lr[VRF_TARGET_Z];
    // the delay ring: this env's delay and action -> command constants (the step's env_params_of, vine_hip.hip)
    CommandParams P = S.cmd;
    int d = S.delay;
    if (env_params) {
        P.rail_scale = env_params[(size_t)VP_RAIL_VELOCITY_SCALE * n + e];
        d = min(max((int)env_params[(size_t)VP_ACTION_DELAY * n + e], 0), VINE_MAX_DELAY);
    }
    if (d > 0) {
        const int cm = (int)(c % (unsigned long long)d);
        for (int k = 1; k <= d; ++k) {
            const long long r = S.row + 1 - k;
            float rail = 0.0f, fpam = 0.0f;                       // a row before the log: what a fresh handle's ring holds
            if (r >= 0) {
                const float2 a = make_float2(log[r * VINE_RECORD_FIELDS + VRF_ACTION0], log[r * VINE_RECORD_FIELDS + VRF_ACTION0 + 1]);
                task_new_command<false>(P, a, 0.0f, 0.0f, rail, fpam);
            }
            const int slot = (cm + d - k) % d;                    // (c - k) mod d, k <= d
            ST(VF_FIFO0 + 2 * slot) = rail;
            ST(VF_FIFO0 + 2 * slot + 1) = fpam;
        }
    }
    const float* __restrict__ Ln = Lr + VINE_RECORD_FIELDS;
    reinterpret_cast<float2*>(actions)[e] = make_float2(Ln[VRF_ACTION0], Ln[VRF_ACTION0 + 1]);
    rew[e] = 0.0f;
    reset[e] = 0;
    progress[e] = 0;
}

__global__ __launch_bounds__(THREADS) void vine_sysid_node_kernel(const SysidParams S, const float* __restrict__ st,
                                                                  const unsigned long long* __restrict__ counters,
                                                                  const float* __restrict__ log,
                                                                  const long long* __restrict__ window,
                                                                  float* __restrict__ actions,
                                                                  const long long* __restrict__ reset,
                                                                  double* __restrict__ err, unsigned char* __restrict__ alive) {
    // vine_steps_completed, written out: through the call the compiler orders this kernel's first adds differently
    const long long c = (long long)(counters[0] + (counters[1] >> S.glog));
    const long long k = c - window[0], r0 = window[1];
    if (k < 1 || k > (long long)S.H || r0 < 0 || r0 + k >= (long long)S.T) return;      // (rows stay inside the log whatever the words hold)
    const int n = S.n, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float* __restrict__ Lr = log + (r0 + k) * VINE_RECORD_FIELDS;
    if (alive[e]) {
        bool any_q = false, any_tip = false;
#pragma unroll
        for (int f = 0; f < 2 * VINE_NUM_DOFS; ++f) any_q |= S.w[f] != 0.0f;
#pragma unroll
        for (int f = VRF_TIP_Y; f <= VRF_TIP_VZ; ++f) any_tip |= S.w[f] != 0.0f;
        float x[VINE_SYSID_FIELDS];
#pragma unroll
        for (int f = 0; f < VINE_SYSID_FIELDS; ++f) x[f] = 0.0f;
        if (any_tip) {                                    // the kinematics needs the whole joint state
#pragma unroll
            for (int f = 0; f < 2 * VINE_NUM_DOFS; ++f) x[f] = ST(VF_Q0 + f);
            float tip[4];
            tip_fk_joint(&x[VRF_Q0], &x[VRF_QD0], S.L, S.z1, S.s0, S.c0, tip);
            x[VRF_TIP_Y] = tip[0]; x[VRF_TIP_Z] = tip[1]; x[VRF_TIP_VY] = tip[2]; x[VRF_TIP_VZ] = tip[3];
        } else if (any_q) {
#pragma unroll
            for (int f = 0; f < 2 * VINE_NUM_DOFS; ++f)
                if (S.w[f] != 0.0f) x[f] = ST(VF_Q0 + f);
        }
        double sum = 0.0;
        bool finite = true;
#pragma unroll
        for (int f = 0; f < VINE_SYSID_FIELDS; ++f) {
            if (S.w[f] != 0.0f) {
                finite &= isfinite(x[f]);
                const double dx = (double)x[f] - (double)Lr[f];
                sum += (double)S.w[f] * (dx * dx);
            }
        }
        if (reset[e] != 0 || !finite) alive[e] = 0;      // the candidate left the log's episode
        else err[e] += sum;
    }
    const long long ra = min(r0 + k + 1, min(r0 + (long long)S.H, (long long)S.T - 1));
    const float* __restrict__ La = log + ra * VINE_RECORD_FIELDS;
    reinterpret_cast<float2*>(actions)[e] = make_float2(La[VRF_ACTION0], La[VRF_ACTION0 + 1]);
}

#undef ST

int validate(const VineSysidConfig* c) {
    if (!c) return vine_invalid_arg("sysid config is NULL");
    if (c->abi_version != VINE_SYSID_ABI_VERSION) return vine_invalid_arg("VineSysidConfig.abi_version mismatch");
    if (c->reserved != 0) return vine_invalid_arg("VineSysidConfig.reserved must be 0");
    if (c->num_rows < 2) return vine_invalid_arg("sysid num_rows must be at least 2");
    if (c->horizon < 1 || c->horizon > c->num_rows - 1) return vine_invalid_arg("sysid needs 1 <= horizon <= num_rows - 1");
    for (int f = 0; f < VINE_SYSID_FIELDS; ++f)
        if (!std::isfinite(c->weights[f]) || c->weights[f] < 0.0f) return vine_invalid_arg("sysid weights must be finite and not negative");
    return VINE_OK;
}

int prepare(VineHandle* h, const VineSysidConfig* cfg, VineHandleInfo& info, SysidParams& S) {
    int rc = vine_handle_info(h, &info);
    if (rc) return rc;
    S.n = info.n; S.glog = info.glog; S.T = cfg->num_rows; S.H = cfg->horizon; S.delay = info.delay;
    S.row = 0;
    S.L = info.L; S.z1 = info.z1; S.s0 = info.s0; S.c0 = info.c0;
    S.cmd.clip_act = info.clip_act; S.cmd.act_noise = 0.0f; S.cmd.rail_scale = info.rail_scale;
    S.cmd.fpam_span = info.fpam_span; S.cmd.fpam_min = info.fpam_min;
    for (int f = 0; f < VINE_SYSID_FIELDS; ++f) S.w[f] = cfg->weights[f];
    return VINE_OK;
}

}  // namespace

extern "C" {

int vine_sysid_config_default(VineSysidConfig* c) {
    if (!c) return vine_invalid_arg("sysid config is NULL");
    c->abi_version = VINE_SYSID_ABI_VERSION;
    c->num_rows = 0;
    c->horizon = 50;
    c->reserved = 0;
    for (int f = 0; f < VINE_SYSID_FIELDS; ++f) c->weights[f] = (f < VINE_NUM_DOFS) ? 1.0f : 0.0f;
    return VINE_OK;
}

int vine_sysid_config_size(void) { return (int)sizeof(VineSysidConfig); }

int vine_sysid_pin(VineHandle* h, const VineSysidConfig* cfg, const float* log, int64_t row, float* actions, float* rew,
                   int64_t* reset, int64_t* progress, int64_t* window, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!h || !log || !actions || !rew || !reset || !progress || !window) return vine_invalid_arg("null argument to vine_sysid_pin");
    if (reinterpret_cast<uintptr_t>(actions) & 7u) return vine_invalid_arg("sysid actions must be 8-byte aligned");
    if (row < 0 || row >= cfg->num_rows) return vine_invalid_arg("sysid pin: row outside the log");
    if (row + cfg->horizon >= cfg->num_rows) return vine_invalid_arg("sysid pin: row + horizon outside the log");
    VineHandleInfo info;
    SysidParams S;
    rc = prepare(h, cfg, info, S);
    if (rc) return rc;
    if (info.flags & (VINE_FLAG_CREATE_SHELF | VINE_FLAG_CREATE_PIPE)) {
        vine_set_error("sysid pin: CREATE_SHELF / CREATE_PIPE handles are refused (obstacle poses are not in a log row: free space only)");
        return VINE_ERR_UNSUPPORTED;
    }
    if (info.flags & VINE_FLAG_VINE_RANDOMIZE) {
        vine_set_error("sysid pin: a handle with vine_randomize is refused (a candidate must be a deterministic plant)");
        return VINE_ERR_UNSUPPORTED;
    }
    S.row = row;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_sysid_pin_kernel, dim3((S.n + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, S,
                       info.state, info.counters, info.env_params, log, actions, rew, (long long*)reset, (long long*)progress,
                       (long long*)window);
    return vine_launch_status("vine_sysid_pin");
}

int vine_sysid_scheduled(VineHandle* h, const VineSysidConfig* cfg, const float* log, const int64_t* window, float* actions,
                         const int64_t* reset, double* err, uint8_t* alive, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!h || !log || !window || !actions || !reset || !err || !alive) return vine_invalid_arg("null argument to vine_sysid_scheduled");
    if (reinterpret_cast<uintptr_t>(actions) & 7u) return vine_invalid_arg("sysid actions must be 8-byte aligned");
    VineHandleInfo info;
    SysidParams S;
    rc = prepare(h, cfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_sysid_node_kernel, dim3((S.n + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, S,
                       info.state, info.counters, log, (const long long*)window, actions, (const long long*)reset, err, alive);
    return vine_launch_status("vine_sysid_scheduled");
}

}  // extern "C"
