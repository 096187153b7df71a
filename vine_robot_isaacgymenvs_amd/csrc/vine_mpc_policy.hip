// vine_mpc_policy.hip — policy-guided MPC for MI355X (gfx950): include/vine_mpc_policy.h states the semantics,
// utils/mpc_policy.py (head, act, keep, terminal, compose) is the same statement in numpy.
//
// The fork, the act and the terminal kernel lay one model env over a quad of lanes, 64 envs per workgroup of 256 lanes, as
// the four-lanes-per-env step kernel does: lane t of a quad holds units {16 i + 4 t .. + 3 : i < 16} of a 256-unit row, so the
// four lanes read or write 64 contiguous bytes per instruction, and the head is quad_ln_heads<3> (vine_policy_head.h), the
// function that kernel calls.  Its reductions are DPP quad_perm reads, which need the whole quad active: every return in
// front of them is uniform over the grid (the horizon step k) or over the quad (e >= n), and what only sample 0 or only lane 0
// does comes behind them.  N is a multiple of 512, so every workgroup is full.  The compose kernel is one lane per plant.
// No LDS, no atomics; plain C++ stores only.
//
// CONTRACTION IS OFF FOR THIS TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it with
// -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): `mu + d` and `cost - w * V` must stay the single
// operations numpy forms.  The two exceptions are vine_policy_head.h and vine_task_shared.h, included under contract(fast):
// the head must be the function the step kernels (compiled with -ffp-contract=fast) run, and clampf is the step's own.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "../../include/vine_mpc_policy.h"
#include "vine_observer.h"
#pragma clang fp contract(fast)
#include "vine_policy_head.h"
#include "vine_task_shared.h"
#pragma clang fp contract(off)
#include "vine_mpc_shared.h"      // the launch functions' shared refusals

namespace {

constexpr int THREADS = VINE_MPC_THREADS;
constexpr int UNITS = VINE_MPC_POLICY_UNITS;
static_assert(THREADS == 256 && UNITS == 256, "one quad per env, sixteen float4 per lane and row");

struct PolicyParams {
    int n, m, K, H, glog;                  // model envs, plants, samples, horizon; the MODEL handle's counter shift
    int obs_width;
    float clip, ln_eps, value_eps;         // the MODEL handle's clip_actions
    double terminal_value;
};

// This lane's sixteen float4 of row `row` (256 floats): units {16 i + 4 t .. + 3}.
__device__ __forceinline__ void quad_load_row(const float* rows, size_t row, int t, float4 (&q)[16]) {
    const float4* r = reinterpret_cast<const float4*>(rows + row * UNITS) + t;
#pragma unroll
    for (int i = 0; i < 16; ++i) q[i] = r[4 * i];
}
__device__ __forceinline__ void quad_store_row(float* rows, size_t row, size_t stride, int t, const float4 (&q)[16]) {
    float4* r = reinterpret_cast<float4*>(rows + row * stride) + t;
#pragma unroll
    for (int i = 0; i < 16; ++i) r[4 * i] = q[i];
}

// (component by component: a select between two float4 objects goes through scratch)
__device__ __forceinline__ float4 zero_if(bool c, const float4& v) {
    return make_float4(c ? 0.0f : v.x, c ? 0.0f : v.y, c ? 0.0f : v.z, c ? 0.0f : v.w);
}

__global__ __launch_bounds__(THREADS) void vine_mpc_policy_fork_kernel(const PolicyParams S, const float* __restrict__ plant_obs,
                                                                       float* __restrict__ model_obs,
                                                                       const float* __restrict__ plant_h,
                                                                       const float* __restrict__ plant_c,
                                                                       float* __restrict__ h_state, float* __restrict__ c_state,
                                                                       float* __restrict__ h_op, long long h_op_stride) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x, e = g >> 2, t = g & 3;
    if (e >= S.n) return;
    const int p = e / S.K;
    for (int col = t; col < S.obs_width; col += 4)
        model_obs[(size_t)e * S.obs_width + col] = plant_obs[(size_t)p * S.obs_width + col];
    float4 q[16];
    quad_load_row(plant_h, (size_t)p, t, q);
    quad_store_row(h_state, (size_t)e, UNITS, t, q);
    quad_store_row(h_op, (size_t)e, (size_t)h_op_stride, t, q);
    quad_load_row(plant_c, (size_t)p, t, q);
    quad_store_row(c_state, (size_t)e, UNITS, t, q);
}

__global__ __launch_bounds__(THREADS) void vine_mpc_policy_act_kernel(const PolicyParams S,
                                                                      const unsigned long long* __restrict__ counters,
                                                                      const long long* __restrict__ window,
                                                                      const float* __restrict__ y, const float* __restrict__ hw,
                                                                      const float* __restrict__ hc,
                                                                      const long long* __restrict__ plant_reset,
                                                                      const float* __restrict__ h_state,
                                                                      const float* __restrict__ c_state, float* __restrict__ actions,
                                                                      float* __restrict__ mu0, float* __restrict__ plant_h,
                                                                      float* __restrict__ plant_c, float* __restrict__ mu_out) {
    const long long k = (long long)vine_steps_completed(counters, S.glog) - window[0];
    if (k < 0 || k >= (long long)S.H) return;          // uniform over the grid
    const int g = blockIdx.x * blockDim.x + threadIdx.x, e = g >> 2, t = g & 3;
    if (e >= S.n) return;                              // uniform over the quad
    float4 yq[16];
    quad_load_row(y, (size_t)e, t, yq);
    // (lane 0 alone reads the perturbation it overwrites below)
    const float2 d = t == 0 ? reinterpret_cast<const float2*>(actions)[e] : make_float2(0.0f, 0.0f);
    float hd[3];
    quad_ln_heads<3>(yq, hw, t, S.ln_eps, hc, hd);
    const float m0 = hd[0], m1 = hd[1];
    const float s0 = m0 + d.x, s1 = m1 + d.y;
    if (t == 0) {
        reinterpret_cast<float2*>(actions)[e] = make_float2(clampf(s0, S.clip), clampf(s1, S.clip));
        if (mu_out) reinterpret_cast<float2*>(mu_out)[e] = make_float2(m0, m1);
    }
    if (k != 0) return;
    const int p = e / S.K;
    if (e != p * S.K) return;
    // the keep: the policy's state after seeing the plant's observation, or zeros where the plant's next step only consumes
    // its reset
    const bool consumed = plant_reset[p] != 0;
    const float4* hr = reinterpret_cast<const float4*>(h_state + (size_t)e * UNITS) + t;
    const float4* cr = reinterpret_cast<const float4*>(c_state + (size_t)e * UNITS) + t;
    float4* ph = reinterpret_cast<float4*>(plant_h + (size_t)p * UNITS) + t;
    float4* pc = reinterpret_cast<float4*>(plant_c + (size_t)p * UNITS) + t;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float4 hv = hr[4 * i], cv = cr[4 * i];
        ph[4 * i] = zero_if(consumed, hv);
        pc[4 * i] = zero_if(consumed, cv);
    }
    if (t == 0) reinterpret_cast<float2*>(mu0)[p] = consumed ? make_float2(0.0f, 0.0f) : make_float2(m0, m1);
}

__global__ __launch_bounds__(THREADS) void vine_mpc_policy_terminal_kernel(const PolicyParams S,
                                                                           const unsigned long long* __restrict__ counters,
                                                                           const long long* __restrict__ window,
                                                                           const float* __restrict__ y, const float* __restrict__ hw,
                                                                           const float* __restrict__ hc,
                                                                           const double* __restrict__ value_mean,
                                                                           const double* __restrict__ value_var,
                                                                           double* __restrict__ cost, unsigned char* __restrict__ alive,
                                                                           float* __restrict__ value_out) {
    const long long k = (long long)vine_steps_completed(counters, S.glog) - window[0];
    if (k != (long long)S.H) return;                   // uniform over the grid
    const int g = blockIdx.x * blockDim.x + threadIdx.x, e = g >> 2, t = g & 3;
    if (e >= S.n) return;                              // uniform over the quad
    float4 yq[16];
    quad_load_row(y, (size_t)e, t, yq);
    float hd[3];
    quad_ln_heads<3>(yq, hw, t, S.ln_eps, hc, hd);
    if (t != 0) return;
    // (the clamp inside unnormalize_value would swallow a NaN: a row that is not finite stays as it is)
    float v = hd[2];
    if (value_mean && isfinite(v)) v = unnormalize_value(v, value_mean, value_var, S.value_eps);
    if (value_out) value_out[e] = v;
    if (!alive[e]) return;
    if (!isfinite(v)) {
        cost[e] = INFINITY;
        alive[e] = 0;
    } else {
        const double wv = S.terminal_value * (double)v;
        cost[e] = cost[e] - wv;
    }
}

__global__ __launch_bounds__(THREADS) void vine_mpc_policy_compose_kernel(const PolicyParams S, const float* __restrict__ mu0,
                                                                          const long long* __restrict__ plant_reset,
                                                                          float* __restrict__ plant_actions,
                                                                          float* __restrict__ history) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S.m) return;
    if (plant_reset[p] != 0) return;                   // the update wrote (0, 0)
    const float2 m = reinterpret_cast<const float2*>(mu0)[p];
    const float2 r = reinterpret_cast<const float2*>(plant_actions)[p];
    const float s0 = m.x + r.x, s1 = m.y + r.y;
    const float2 a = make_float2(clampf(s0, S.clip), clampf(s1, S.clip));
    reinterpret_cast<float2*>(plant_actions)[p] = a;
    reinterpret_cast<float2*>(history)[(size_t)p * VINE_MAX_DELAY] = a;
}

// The part of vine_mpc.h's configuration these launches read, checked as vine_mpc.hip checks it.
int validate(const VineMpcConfig* c, const VineMpcPolicyConfig* pc) {
    if (!c) return vine_invalid_arg("mpc config is NULL");
    if (!pc) return vine_invalid_arg("mpc policy config is NULL");
    if (c->abi_version != VINE_MPC_ABI_VERSION) return vine_invalid_arg("VineMpcConfig.abi_version mismatch");
    if (pc->abi_version != VINE_MPC_POLICY_ABI_VERSION) return vine_invalid_arg("VineMpcPolicyConfig.abi_version mismatch");
    if (c->num_plants < 1) return vine_invalid_arg("mpc num_plants must be at least 1");
    if (c->samples < 2) return vine_invalid_arg("mpc samples must be at least 2");
    if ((long long)c->num_plants * c->samples > 0x7fffffffLL) return vine_invalid_arg("mpc num_plants * samples does not fit an int32");
    if (c->horizon < 1 || c->horizon > VINE_MPC_MAX_HORIZON) return vine_invalid_arg("mpc needs 1 <= horizon <= VINE_MPC_MAX_HORIZON (64)");
    if (((long long)c->num_plants * c->samples) % VINE_MPC_POLICY_ROWS)
        return vine_invalid_arg("mpc policy: num_plants * samples must be a multiple of 512 (the inference kernels' shape)");
    if (pc->obs_width < 1 || pc->obs_width > VINE_MAX_OBS) return vine_invalid_arg("mpc policy obs_width must be in 1 .. VINE_MAX_OBS");
    if (!std::isfinite(pc->ln_eps) || pc->ln_eps < 0.0f) return vine_invalid_arg("mpc policy ln_eps must be finite and not negative");
    if (!std::isfinite(pc->value_eps) || pc->value_eps < 0.0f) return vine_invalid_arg("mpc policy value_eps must be finite and not negative");
    if (!std::isfinite(pc->terminal_value) || pc->terminal_value < 0.0)
        return vine_invalid_arg("mpc policy terminal_value must be finite and not negative");
    return VINE_OK;
}

bool misaligned(unsigned mask, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & mask) != 0;
}

// The model handle's part of a launch's parameters; refuses a handle that does not hold num_plants * samples envs or whose
// clip_actions is above 1.
int prepare(VineHandle* model, const VineMpcConfig* cfg, const VineMpcPolicyConfig* pc, VineHandleInfo& info, PolicyParams& S) {
    int rc = vine_handle_info(model, &info);
    if (rc) return rc;
    if ((long long)info.n != (long long)cfg->num_plants * cfg->samples) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc policy: the model handle has %d envs, not num_plants * samples = %d * %d", info.n,
                 cfg->num_plants, cfg->samples);
        return vine_invalid_arg(msg);
    }
    if (!(info.clip_act <= 1.0f))
        return unsupported("mpc policy: a model handle with clip_actions above 1 is refused (no inner clamp is applied to mu)");
    S.n = info.n; S.m = cfg->num_plants; S.K = cfg->samples; S.H = cfg->horizon; S.glog = info.glog;
    S.obs_width = pc->obs_width;
    S.clip = info.clip_act; S.ln_eps = pc->ln_eps; S.value_eps = pc->value_eps;
    S.terminal_value = pc->terminal_value;
    return VINE_OK;
}

inline dim3 quad_grid(int n) { return dim3((unsigned)(((long long)n * 4 + THREADS - 1) / THREADS)); }

}  // namespace

extern "C" {

int vine_mpc_policy_config_default(VineMpcPolicyConfig* pc) {
    if (!pc) return vine_invalid_arg("mpc policy config is NULL");
    pc->abi_version = VINE_MPC_POLICY_ABI_VERSION;
    pc->obs_width = 0;
    pc->ln_eps = 1e-5f;
    pc->value_eps = 1e-5f;
    pc->terminal_value = 0.0;
    return VINE_OK;
}

int vine_mpc_policy_config_size(void) { return (int)sizeof(VineMpcPolicyConfig); }

int vine_mpc_policy_fork(VineHandle* plant, VineHandle* model, const VineMpcConfig* cfg, const VineMpcPolicyConfig* pcfg,
                         const float* plant_obs, int32_t plant_obs_width, float* model_obs, int32_t model_obs_width,
                         const float* plant_h, const float* plant_c, float* h_state, float* c_state, float* h_op,
                         int64_t h_op_stride, void* stream) {
    int rc = validate(cfg, pcfg);
    if (rc) return rc;
    if (!plant || !model || !plant_obs || !model_obs || !plant_h || !plant_c || !h_state || !c_state || !h_op)
        return vine_invalid_arg("null argument to vine_mpc_policy_fork");
    if (plant_obs_width != model_obs_width || plant_obs_width != pcfg->obs_width) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc policy fork: observation width of the plant (%d), of the model (%d) and of the "
                 "configuration (%d) must be one", plant_obs_width, model_obs_width, pcfg->obs_width);
        return vine_invalid_arg(msg);
    }
    if (misaligned(15u, {plant_h, plant_c, h_state, c_state, h_op}) || h_op_stride < UNITS || (h_op_stride & 3))
        return vine_invalid_arg("mpc policy fork: LSTM state rows must be 16-byte aligned (h_op_stride a multiple of 4, at least 256)");
    if (plant == model) return vine_invalid_arg("mpc policy fork: the plant and the model must be two handles");
    VineHandleInfo pinfo, info;
    PolicyParams S;
    rc = vine_handle_info(plant, &pinfo);
    if (rc) return rc;
    rc = prepare(model, cfg, pcfg, info, S);
    if (rc) return rc;
    if (pinfo.n != cfg->num_plants) return vine_invalid_arg("mpc policy fork: the plant handle does not have num_plants envs");
    rc = mpc_same_device("mpc policy fork", "model", pinfo, info);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_policy_fork_kernel, quad_grid(S.n), dim3(THREADS), 0, (hipStream_t)stream, S, plant_obs, model_obs,
                       plant_h, plant_c, h_state, c_state, h_op, (long long)h_op_stride);
    return vine_launch_status("vine_mpc_policy_fork");
}

int vine_mpc_policy_act(VineHandle* model, const VineMpcConfig* cfg, const VineMpcPolicyConfig* pcfg, const float* y,
                        const float* hw, const float* hc, const int64_t* window, const int64_t* plant_reset,
                        const float* h_state, const float* c_state, float* actions, float* mu0, float* plant_h,
                        float* plant_c, float* mu_out, void* stream) {
    int rc = validate(cfg, pcfg);
    if (rc) return rc;
    if (!model || !y || !hw || !hc || !window || !plant_reset || !h_state || !c_state || !actions || !mu0 || !plant_h || !plant_c)
        return vine_invalid_arg("null argument to vine_mpc_policy_act");
    if (misaligned(15u, {y, hw, h_state, c_state, plant_h, plant_c}))
        return vine_invalid_arg("mpc policy act: y, hw and the LSTM state rows must be 16-byte aligned");
    if (misaligned(7u, {actions, mu0, mu_out})) return vine_invalid_arg("mpc policy act: actions, mu0 and mu_out must be 8-byte aligned");
    VineHandleInfo info;
    PolicyParams S;
    rc = prepare(model, cfg, pcfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_policy_act_kernel, quad_grid(S.n), dim3(THREADS), 0, (hipStream_t)stream, S, info.counters,
                       (const long long*)window, y, hw, hc, (const long long*)plant_reset, h_state, c_state, actions, mu0, plant_h,
                       plant_c, mu_out);
    return vine_launch_status("vine_mpc_policy_act");
}

int vine_mpc_policy_terminal(VineHandle* model, const VineMpcConfig* cfg, const VineMpcPolicyConfig* pcfg, const float* y,
                             const float* hw, const float* hc, const double* value_mean, const double* value_var,
                             const int64_t* window, double* cost, uint8_t* alive, float* value_out, void* stream) {
    int rc = validate(cfg, pcfg);
    if (rc) return rc;
    if (!model || !y || !hw || !hc || !window || !cost || !alive) return vine_invalid_arg("null argument to vine_mpc_policy_terminal");
    if ((value_mean == nullptr) != (value_var == nullptr))
        return vine_invalid_arg("mpc policy terminal: value_mean and value_var are given both or neither");
    if (misaligned(15u, {y, hw})) return vine_invalid_arg("mpc policy terminal: y and hw must be 16-byte aligned");
    VineHandleInfo info;
    PolicyParams S;
    rc = prepare(model, cfg, pcfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_policy_terminal_kernel, quad_grid(S.n), dim3(THREADS), 0, (hipStream_t)stream, S, info.counters,
                       (const long long*)window, y, hw, hc, value_mean, value_var, cost, alive, value_out);
    return vine_launch_status("vine_mpc_policy_terminal");
}

int vine_mpc_policy_compose(VineHandle* model, const VineMpcConfig* cfg, const VineMpcPolicyConfig* pcfg, const float* mu0,
                            const int64_t* plant_reset, float* plant_actions, float* history, void* stream) {
    int rc = validate(cfg, pcfg);
    if (rc) return rc;
    if (!model || !mu0 || !plant_reset || !plant_actions || !history) return vine_invalid_arg("null argument to vine_mpc_policy_compose");
    if (misaligned(7u, {mu0, plant_actions, history}))
        return vine_invalid_arg("mpc policy compose: mu0, plant_actions and history must be 8-byte aligned");
    VineHandleInfo info;
    PolicyParams S;
    rc = prepare(model, cfg, pcfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_policy_compose_kernel, dim3((S.m + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, S,
                       mu0, (const long long*)plant_reset, plant_actions, history);
    return vine_launch_status("vine_mpc_policy_compose");
}

}  // extern "C"
