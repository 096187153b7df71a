// vine_mpc.hip — sampling-based model-predictive control (MPC) for MI355X (gfx950): include/vine_mpc.h states the semantics,
// utils/mpc.py mpc_replay is the same statement in numpy.
//
// vine_mpc_fork_kernel and vine_mpc_node_kernel are elementwise, one lane per model env, 256 lanes per workgroup, over the SoA
// state blocks (st[f * n + e]).  A wave of the fork reads one or two plants' columns (64 consecutive samples share a plant
// where K >= 64) and writes 64 contiguous floats per field.  The node reads the step counter exactly as the other observers
// do (vine_observer.h vine_steps_completed) and returns at once outside the window; inside, a lane reads its rew, reset
// word, alive byte and cost (21 B), writes at most cost and alive (9 B) and its next action (8 B, two Philox calls).
// vine_mpc_update_kernel is one workgroup per plant: lane-strided sums in float64, a 64-wide butterfly per wave, the four
// wave sums through LDS and added in wave order.  No atomics anywhere; plain C++ stores only.
//
// CONTRACTION IS OFF FOR THIS TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it with
// -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): `nominal + z * c` must stay a multiply and an add, each
// rounded, as numpy forms it.  The one exception is vine_task_shared.h, included under contract(fast): task_new_command must
// give the words the step kernels (compiled with -ffp-contract=fast) put into the delay ring.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/vine_env_params.h"
#include "../../include/vine_mpc.h"
#include "vine_observer.h"
#include "vine_policy_head.h"
// ... except the action -> command map: the ring must hold the STEP KERNELS' bits, and those units contract it
#pragma clang fp contract(fast)
#include "vine_task_shared.h"
#pragma clang fp contract(off)
// the column copy, the ring rebuild and the reduction's wave step: stated once for this unit and vine_mpc_adapt.hip
#include "vine_mpc_shared.h"

namespace {

constexpr int THREADS = VINE_MPC_THREADS;
constexpr int WAVES = THREADS / 64;
constexpr int HMAX = VINE_MPC_MAX_HORIZON;
static_assert(THREADS == 256 && 2 * HMAX <= THREADS, "one lane of the update per nominal entry");

struct MpcParams {
    int n, m, K, H, glog, delay;           // model envs, plants, samples, horizon; the MODEL handle's counter shift and delay
    unsigned seed_lo, seed_hi;
    float c[2];                            // float32(float64(sigma[a]) * K0)
    double lambda;
    CommandParams cmd;                     // the model configuration's
};

// u[j][k][a] of sample e = p * K + j at control step `tick` around the nominal entry (nom0, nom1): include/vine_mpc.h NOISE.
__device__ __forceinline__ float2 mpc_action(const MpcParams& S, unsigned e, bool first, long long tick, int k, float nom0,
                                             float nom1) {
    float z[2] = {0.0f, 0.0f};
    if (!first) {
        const unsigned long long t = (unsigned long long)tick;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            unsigned w[4];
            philox4x32_10(e, (unsigned)t, VINE_MPC_RNG_NOISE | ((unsigned)(t >> 32) << 8), (unsigned)(2 * k + a), S.seed_lo,
                          S.seed_hi, w);
            z[a] = (float)mpc_deviate_int(w);
        }
    }
    const float zc0 = z[0] * S.c[0], zc1 = z[1] * S.c[1];
    const float x0 = nom0 + zc0, x1 = nom1 + zc1;
    return make_float2(clampf(x0, S.cmd.clip_act), clampf(x1, S.cmd.clip_act));
}

__global__ __launch_bounds__(THREADS) void vine_mpc_fork_kernel(const MpcParams S, const float* __restrict__ pst,
                                                                float* __restrict__ st,
                                                                const unsigned long long* __restrict__ counters,
                                                                const float* __restrict__ env_params,
                                                                const long long* __restrict__ plant_progress,
                                                                const float* __restrict__ nominal,
                                                                const float* __restrict__ history,
                                                                const long long* __restrict__ tick, float* __restrict__ actions,
                                                                float* __restrict__ rew, long long* __restrict__ reset,
                                                                long long* __restrict__ progress, double* __restrict__ cost,
                                                                unsigned char* __restrict__ alive, long long* __restrict__ window) {
    const unsigned long long c = vine_steps_completed(counters, S.glog);
    const int n = S.n, m = S.m, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) window[0] = (long long)c;
    if (e >= n) return;
    const int p = e / S.K, j = e - p * S.K;
    MPC_COPY_COLUMN(pst, m, p, st, n, e);
    // the delay ring: this sample's delay and action -> command constants (the step's env_params_of, vine_hip.hip)
    CommandParams P = S.cmd;
    int d = S.delay;
    if (env_params) {
        P.rail_scale = env_params[(size_t)VP_RAIL_VELOCITY_SCALE * n + e];
        d = min(max((int)env_params[(size_t)VP_ACTION_DELAY * n + e], 0), VINE_MAX_DELAY);
    }
    mpc_rebuild_ring(P, d, c, reinterpret_cast<const float2*>(history) + (size_t)p * VINE_MAX_DELAY, st, n, e);
    const float2 nom = reinterpret_cast<const float2*>(nominal)[(size_t)p * S.H];
    reinterpret_cast<float2*>(actions)[e] = mpc_action(S, (unsigned)e, j == 0, tick[p], 0, nom.x, nom.y);
    rew[e] = 0.0f;
    reset[e] = 0;
    progress[e] = plant_progress[p];
    cost[e] = 0.0;
    alive[e] = 1;
}

__global__ __launch_bounds__(THREADS) void vine_mpc_node_kernel(const MpcParams S, const unsigned long long* __restrict__ counters,
                                                                const float* __restrict__ nominal,
                                                                const long long* __restrict__ tick,
                                                                const long long* __restrict__ window, float* __restrict__ actions,
                                                                const float* __restrict__ rew, const long long* __restrict__ reset,
                                                                double* __restrict__ cost, unsigned char* __restrict__ alive) {
    const long long c = (long long)vine_steps_completed(counters, S.glog);
    const long long k = c - window[0];
    if (k < 1 || k > (long long)S.H) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S.n) return;
    const int p = e / S.K, j = e - p * S.K;
    if (alive[e]) {
        const float r = rew[e];
        if (!isfinite(r)) {
            cost[e] = INFINITY;
            alive[e] = 0;
        } else {
            cost[e] += -(double)r;
            if (reset[e] != 0) alive[e] = 0;      // the step that ends an episode still counted
        }
    }
    if (k < (long long)S.H) {
        const float2 nom = reinterpret_cast<const float2*>(nominal)[(size_t)p * S.H + (int)k];
        reinterpret_cast<float2*>(actions)[e] = mpc_action(S, (unsigned)e, j == 0, tick[p], (int)k, nom.x, nom.y);
    }
}

// The sum (or the minimum) of one value per lane over the workgroup, in a fixed order: wave_sum / wave_min (vine_mpc_shared.h)
// over the 64 lanes of each wave, the four wave values through LDS, combined in wave order.
// part: WAVES doubles of LDS per call site; the caller's __syncthreads() stands between the write and the read.

__global__ __launch_bounds__(THREADS) void vine_mpc_update_kernel(const MpcParams S, const double* __restrict__ cost,
                                                                  const long long* __restrict__ plant_reset,
                                                                  float* __restrict__ nominal, float* __restrict__ history,
                                                                  long long* __restrict__ tick, float* __restrict__ plant_actions,
                                                                  double* __restrict__ weights) {
    __shared__ float nom[2 * HMAX];                    // nominal[p], read before anything is written
    __shared__ float fresh[2 * HMAX];                  // new[k][a]
    __shared__ double part_min[WAVES];
    __shared__ double part_w[WAVES];
    __shared__ double part_u[2 * HMAX][WAVES];
    const int p = blockIdx.x, t = (int)threadIdx.x, K = S.K, H = S.H;
    const int wave = t >> 6, lane = t & 63;
    if (t < 2 * H) nom[t] = nominal[(size_t)p * 2 * H + t];
    const long long tk = tick[p];
    const double* __restrict__ cp = cost + (size_t)p * K;

    // 1. beta
    double lo = INFINITY;
    for (int j = t; j < K; j += THREADS) lo = fmin(lo, cp[j]);
    lo = wave_min(lo);
    if (lane == 0) part_min[wave] = lo;
    __syncthreads();                                   // (also: nom is complete)
    double beta = part_min[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) beta = fmin(beta, part_min[w]);
    const bool any = beta < INFINITY;                  // uniform over the workgroup

    if (any) {
        // 2. the weights' sum; 3. per (k, a) the weighted sum of u: a lane goes through its samples in ascending j
        double sw = 0.0;
        for (int j = t; j < K; j += THREADS) {
            const double cj = cp[j];
            const double w = cj < INFINITY ? exp(-(cj - beta) / S.lambda) : 0.0;
            if (weights) weights[(size_t)p * K + j] = w;
            sw += w;
        }
        sw = wave_sum(sw);
        if (lane == 0) part_w[wave] = sw;
        for (int k = 0; k < H; ++k) {
            double s0 = 0.0, s1 = 0.0;
            const float n0 = nom[2 * k], n1 = nom[2 * k + 1];
            for (int j = t; j < K; j += THREADS) {
                const double cj = cp[j];
                const double w = cj < INFINITY ? exp(-(cj - beta) / S.lambda) : 0.0;
                const float2 u = mpc_action(S, (unsigned)(p * K + j), j == 0, tk, k, n0, n1);
                s0 += w * (double)u.x;
                s1 += w * (double)u.y;
            }
            s0 = wave_sum(s0);
            s1 = wave_sum(s1);
            if (lane == 0) {
                part_u[2 * k][wave] = s0;
                part_u[2 * k + 1][wave] = s1;
            }
        }
    } else if (weights) {
        for (int j = t; j < K; j += THREADS) weights[(size_t)p * K + j] = 0.0;
    }
    __syncthreads();
    if (t < 2 * H) {
        float v = nom[t];                              // 4. no finite cost: the nominal stays
        if (any) {
            double sw = part_w[0], su = part_u[t][0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) {
                sw += part_w[w];
                su += part_u[t][w];
            }
            v = (float)(su / sw);
        }
        fresh[t] = v;
    }
    __syncthreads();
    const bool consumed = plant_reset[p] != 0;         // the plant's next step only consumes its reset
    if (t < 2 * H) {
        const int k = t >> 1, a = t & 1;
        nominal[(size_t)p * 2 * H + t] = consumed ? 0.0f : fresh[2 * min(k + 1, H - 1) + a];
    }
    if (t == 0) {
        const float2 act = consumed ? make_float2(0.0f, 0.0f) : make_float2(fresh[0], fresh[1]);
        reinterpret_cast<float2*>(plant_actions)[p] = act;
        float2* hist = reinterpret_cast<float2*>(history) + (size_t)p * VINE_MAX_DELAY;
        for (int i = VINE_MAX_DELAY - 1; i > 0; --i) hist[i] = hist[i - 1];
        hist[0] = act;
        tick[p] = tk + 1;
    }
}

int validate(const VineMpcConfig* c) {
    if (!c) return vine_invalid_arg("mpc config is NULL");
    if (c->abi_version != VINE_MPC_ABI_VERSION) return vine_invalid_arg("VineMpcConfig.abi_version mismatch");
    if (c->num_plants < 1) return vine_invalid_arg("mpc num_plants must be at least 1");
    if (c->samples < 2) return vine_invalid_arg("mpc samples must be at least 2");
    if ((long long)c->num_plants * c->samples > 0x7fffffffLL) return vine_invalid_arg("mpc num_plants * samples does not fit an int32");
    if (c->horizon < 1 || c->horizon > VINE_MPC_MAX_HORIZON) return vine_invalid_arg("mpc needs 1 <= horizon <= VINE_MPC_MAX_HORIZON (64)");
    if (!std::isfinite(c->lambda) || !(c->lambda > 0.0)) return vine_invalid_arg("mpc lambda must be finite and positive");
    for (int a = 0; a < 2; ++a)
        if (!std::isfinite(c->sigma[a]) || c->sigma[a] < 0.0f) return vine_invalid_arg("mpc sigma must be finite and not negative");
    return VINE_OK;
}

// The model handle's part of a launch's parameters; refuses a handle that does not hold num_plants * samples envs.
int prepare(VineHandle* model, const VineMpcConfig* cfg, VineHandleInfo& info, MpcParams& S) {
    int rc = vine_handle_info(model, &info);
    if (rc) return rc;
    if ((long long)info.n != (long long)cfg->num_plants * cfg->samples) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc: the model handle has %d envs, not num_plants * samples = %d * %d", info.n,
                 cfg->num_plants, cfg->samples);
        return vine_invalid_arg(msg);
    }
    S.n = info.n; S.m = cfg->num_plants; S.K = cfg->samples; S.H = cfg->horizon; S.glog = info.glog; S.delay = info.delay;
    S.seed_lo = (unsigned)cfg->seed; S.seed_hi = (unsigned)(cfg->seed >> 32);
    for (int a = 0; a < 2; ++a) S.c[a] = (float)((double)cfg->sigma[a] * noise_scale());
    S.lambda = cfg->lambda;
    S.cmd = mpc_command_params(info);
    return VINE_OK;
}

}  // namespace

extern "C" {

int vine_mpc_config_default(VineMpcConfig* c) {
    if (!c) return vine_invalid_arg("mpc config is NULL");
    c->abi_version = VINE_MPC_ABI_VERSION;
    c->num_plants = 0;
    c->samples = 256;
    c->horizon = 20;
    c->lambda = 0.05;
    c->sigma[0] = c->sigma[1] = 0.5f;
    c->seed = 0;
    return VINE_OK;
}

int vine_mpc_config_size(void) { return (int)sizeof(VineMpcConfig); }

int vine_mpc_fork(VineHandle* plant, VineHandle* model, const VineMpcConfig* cfg, const int64_t* plant_progress,
                  const float* nominal, const float* history, const int64_t* tick, float* actions, float* rew,
                  int64_t* reset, int64_t* progress, double* cost, uint8_t* alive, int64_t* window, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!plant || !model || !plant_progress || !nominal || !history || !tick || !actions || !rew || !reset || !progress ||
        !cost || !alive || !window)
        return vine_invalid_arg("null argument to vine_mpc_fork");
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(nominal) | reinterpret_cast<uintptr_t>(history)) & 7u)
        return vine_invalid_arg("mpc actions, nominal and history must be 8-byte aligned");
    if (plant == model) return vine_invalid_arg("mpc fork: the plant and the model must be two handles");
    VineHandleInfo pinfo, info;
    MpcParams S;
    rc = vine_handle_info(plant, &pinfo);
    if (rc) return rc;
    rc = prepare(model, cfg, info, S);
    if (rc) return rc;
    if (pinfo.n != cfg->num_plants) return vine_invalid_arg("mpc fork: the plant handle does not have num_plants envs");
    rc = mpc_stand_in("mpc fork", "model", "a sample must be a deterministic plant", pinfo, info);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_fork_kernel, dim3((S.n + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, S,
                       (const float*)pinfo.state, info.state, info.counters, info.env_params, (const long long*)plant_progress,
                       nominal, history, (const long long*)tick, actions, rew, (long long*)reset, (long long*)progress, cost,
                       alive, (long long*)window);
    return vine_launch_status("vine_mpc_fork");
}

int vine_mpc_scheduled(VineHandle* model, const VineMpcConfig* cfg, const float* nominal, const int64_t* tick,
                       const int64_t* window, float* actions, const float* rew, const int64_t* reset, double* cost,
                       uint8_t* alive, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!model || !nominal || !tick || !window || !actions || !rew || !reset || !cost || !alive)
        return vine_invalid_arg("null argument to vine_mpc_scheduled");
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(nominal)) & 7u)
        return vine_invalid_arg("mpc actions and nominal must be 8-byte aligned");
    VineHandleInfo info;
    MpcParams S;
    rc = prepare(model, cfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_node_kernel, dim3((S.n + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, S,
                       info.counters, nominal, (const long long*)tick, (const long long*)window, actions, rew,
                       (const long long*)reset, cost, alive);
    return vine_launch_status("vine_mpc_scheduled");
}

int vine_mpc_update(VineHandle* model, const VineMpcConfig* cfg, const double* cost, const int64_t* plant_reset,
                    float* nominal, float* history, int64_t* tick, float* plant_actions, double* weights, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!model || !cost || !plant_reset || !nominal || !history || !tick || !plant_actions)
        return vine_invalid_arg("null argument to vine_mpc_update");
    if ((reinterpret_cast<uintptr_t>(plant_actions) | reinterpret_cast<uintptr_t>(history)) & 7u)
        return vine_invalid_arg("mpc plant_actions and history must be 8-byte aligned");
    VineHandleInfo info;
    MpcParams S;
    rc = prepare(model, cfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_update_kernel, dim3(S.m), dim3(THREADS), 0, (hipStream_t)stream, S, cost,
                       (const long long*)plant_reset, nominal, history, (long long*)tick, plant_actions, weights);
    return vine_launch_status("vine_mpc_update");
}

}  // extern "C"
