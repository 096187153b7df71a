// vine_mpc_ensemble.hip — the predictive controller's ensemble of candidate plants (MPC_ENSEMBLE) for MI355X (gfx950): a common
// perturbation for the members of a sequence and an update that reduces over members before it reduces over sequences.
// include/vine_mpc_ensemble.h states the semantics, utils/mpc_ensemble.py (group_actions, group_costs, ensemble_replay) is the
// same statement in numpy.
//
// vine_mpc_ensemble_node_kernel has one lane per model env: it reads the step counter as every observer does (vine_observer.h
// vine_steps_completed) and returns at once outside the window; inside, a lane loads its plant's nominal entry and tick (8 B
// each, shared by the wave), forms its GROUP's action (two Philox calls; the E members of a group are neighbouring lanes and
// form the same words) and stores it (8 B, contiguous over the wave).  vine_mpc_ensemble_update_kernel is
// vine_mpc_update_kernel of vine_mpc.hip RESTATED -- that unit is not edited -- with a group in the place of a sample: one
// workgroup per plant, lane t takes the groups t, t + 256, ..; a group's cost is formed from its E consecutive costs by the
// lane itself (no exchange between lanes: E <= 16 doubles, 128 B) and held in registers where a lane has at most HELD groups
// (the weight takes its place behind the minimum), else formed again in every loop; then lane-strided sums in float64, a
// 64-wide butterfly per wave (vine_mpc_shared.h), the four wave sums through LDS and added in wave order.  No atomics anywhere;
// plain C++ stores only.
//
// CONTRACTION IS OFF FOR THIS TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it with
// -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): `nominal + z * c` must stay a multiply and an add, and
// `theta * (c - cmax)`, the members' sum and `cmax + log(..) / theta` the float64 operations numpy performs, each rounded.
// vine_task_shared.h is included as vine_mpc.hip includes it; of it this unit uses clampf alone, which has nothing to contract.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/vine_env_params.h"
#include "../../include/vine_mpc_ensemble.h"
#include "vine_observer.h"
#include "vine_policy_head.h"
#pragma clang fp contract(fast)
#include "vine_task_shared.h"
#pragma clang fp contract(off)
// the reduction's wave step, the deviate's integer and its scale: stated once for the vine_mpc*.hip units
#include "vine_mpc_shared.h"

namespace {

constexpr int THREADS = VINE_MPC_THREADS;
constexpr int WAVES = THREADS / 64;
constexpr int HMAX = VINE_MPC_MAX_HORIZON;
constexpr int HELD = 4;                    // group costs / weights a lane keeps in registers: G <= HELD * THREADS forms each once
static_assert(THREADS == 256 && 2 * HMAX <= THREADS, "one lane of the update per nominal entry");

struct EnsembleParams {
    int n, m, K, H, E, G, glog, risk;      // model envs, plants, samples, horizon, members, groups; the MODEL handle's counter shift
    unsigned seed_lo, seed_hi;
    float clip_act;                        // the MODEL handle's clipActions
    float c[2];                            // float32(float64(sigma[a]) * K0)
    double lambda, theta;
};

// u_g[k][a] of group `index` = p * G + g at control step `tick` around the nominal entry (nom0, nom1): mpc_action of
// vine_mpc.hip restated, with the group's index in the counter's first word.
__device__ __forceinline__ float2 group_action(const EnsembleParams& S, unsigned index, bool first, long long tick, int k,
                                               float nom0, float nom1) {
    float z[2] = {0.0f, 0.0f};
    if (!first) {
        const unsigned long long t = (unsigned long long)tick;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            unsigned w[4];
            philox4x32_10(index, (unsigned)t, VINE_MPC_RNG_NOISE | ((unsigned)(t >> 32) << 8), (unsigned)(2 * k + a), S.seed_lo,
                          S.seed_hi, w);
            z[a] = (float)mpc_deviate_int(w);
        }
    }
    const float zc0 = z[0] * S.c[0], zc1 = z[1] * S.c[1];
    const float x0 = nom0 + zc0, x1 = nom1 + zc1;
    return make_float2(clampf(x0, S.clip_act), clampf(x1, S.clip_act));
}

// C_g of the E consecutive member costs at c: include/vine_mpc_ensemble.h, 2. THE UPDATE.
__device__ __forceinline__ double group_cost_of(const EnsembleParams& S, const double* __restrict__ c) {
    const int E = S.E;
    double cmax = c[0];
    bool finite = isfinite(cmax);
    for (int m = 1; m < E; ++m) {
        const double cm = c[m];
        finite = finite && isfinite(cm);
        cmax = fmax(cmax, cm);
    }
    if (!finite) return INFINITY;
    if (S.risk == VINE_MPC_RISK_MAX) return cmax;
    if (S.risk == VINE_MPC_RISK_MEAN) {
        double s = c[0];
        for (int m = 1; m < E; ++m) s += c[m];
        return s / (double)E;
    }
    double s = exp(S.theta * (c[0] - cmax));
    for (int m = 1; m < E; ++m) s += exp(S.theta * (c[m] - cmax));
    return cmax + log(s / (double)E) / S.theta;
}

__global__ __launch_bounds__(THREADS) void vine_mpc_ensemble_node_kernel(const EnsembleParams S,
                                                                         const unsigned long long* __restrict__ counters,
                                                                         const float* __restrict__ nominal,
                                                                         const long long* __restrict__ tick,
                                                                         const long long* __restrict__ window,
                                                                         float* __restrict__ actions) {
    const long long c = (long long)vine_steps_completed(counters, S.glog);
    const long long k = c - window[0];
    if (k < 0 || k >= (long long)S.H) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S.n) return;
    const int p = e / S.K, g = (e - p * S.K) / S.E;
    const float2 nom = reinterpret_cast<const float2*>(nominal)[(size_t)p * S.H + (int)k];
    reinterpret_cast<float2*>(actions)[e] = group_action(S, (unsigned)(p * S.G + g), g == 0, tick[p], (int)k, nom.x, nom.y);
}

// vine_mpc_update_kernel of vine_mpc.hip, restated: a group in the place of a sample.  `held[i]` belongs to the lane's group
// t + i * THREADS: first its cost, behind the minimum its weight.  Two instantiations, chosen by the launch function: with
// N_HELD = HELD every group of the plant is held (G <= HELD * THREADS) and the loops below that form a cost again are not
// compiled; with N_HELD = 0 none is held and those loops are the whole kernel, as vine_mpc.hip forms its weights again per
// horizon step.  Both go through the groups in the same order and give the same bits.
template <int N_HELD>
__global__ __launch_bounds__(THREADS) void vine_mpc_ensemble_update_kernel(const EnsembleParams S, const double* __restrict__ cost,
                                                                           const long long* __restrict__ plant_reset,
                                                                           float* __restrict__ nominal, float* __restrict__ history,
                                                                           long long* __restrict__ tick,
                                                                           float* __restrict__ plant_actions,
                                                                           double* __restrict__ weights,
                                                                           double* __restrict__ group_cost) {
    __shared__ float nom[2 * HMAX];                    // nominal[p], read before anything is written
    __shared__ float fresh[2 * HMAX];                  // new[k][a]
    __shared__ double part_min[WAVES];
    __shared__ double part_w[WAVES];
    __shared__ double part_u[2 * HMAX][WAVES];
    const int p = blockIdx.x, t = (int)threadIdx.x, K = S.K, H = S.H, E = S.E, G = S.G;
    const int wave = t >> 6, lane = t & 63;
    if (t < 2 * H) nom[t] = nominal[(size_t)p * 2 * H + t];
    const long long tk = tick[p];
    const double* __restrict__ cp = cost + (size_t)p * K;
    double held[N_HELD ? N_HELD : 1];

    // 0. the group costs; 1. beta
    double lo = INFINITY;
#pragma unroll
    for (int i = 0; i < N_HELD; ++i) {
        const int g = t + i * THREADS;
        held[i] = g < G ? group_cost_of(S, cp + (size_t)g * E) : INFINITY;
        if (g < G && group_cost) group_cost[(size_t)p * G + g] = held[i];
        lo = fmin(lo, held[i]);
    }
    if constexpr (N_HELD == 0) {
        for (int g = t; g < G; g += THREADS) {
            const double cg = group_cost_of(S, cp + (size_t)g * E);
            if (group_cost) group_cost[(size_t)p * G + g] = cg;
            lo = fmin(lo, cg);
        }
    }
    lo = wave_min(lo);
    if (lane == 0) part_min[wave] = lo;
    __syncthreads();                                   // (also: nom is complete)
    double beta = part_min[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) beta = fmin(beta, part_min[w]);
    const bool any = beta < INFINITY;                  // uniform over the workgroup

    // w_g of a group cost; stored into every member of the group where the caller asked for it
    auto weight_of = [&](double cg) { return cg < INFINITY ? exp(-(cg - beta) / S.lambda) : 0.0; };
    auto store_weight = [&](int g, double w) {
        if (weights)
            for (int m = 0; m < E; ++m) weights[(size_t)p * K + (size_t)g * E + m] = w;
    };

    if (any) {
        // 2. the weights' sum; 3. per (k, a) the weighted sum of u_g: a lane goes through its groups in ascending g
        double sw = 0.0;
#pragma unroll
        for (int i = 0; i < N_HELD; ++i) {
            const int g = t + i * THREADS;
            if (g < G) {
                held[i] = weight_of(held[i]);
                store_weight(g, held[i]);
                sw += held[i];
            }
        }
        if constexpr (N_HELD == 0) {
            for (int g = t; g < G; g += THREADS) {
                const double w = weight_of(group_cost_of(S, cp + (size_t)g * E));
                store_weight(g, w);
                sw += w;
            }
        }
        sw = wave_sum(sw);
        if (lane == 0) part_w[wave] = sw;
        for (int k = 0; k < H; ++k) {
            double s0 = 0.0, s1 = 0.0;
            const float n0 = nom[2 * k], n1 = nom[2 * k + 1];
#pragma unroll
            for (int i = 0; i < N_HELD; ++i) {
                const int g = t + i * THREADS;
                if (g < G) {
                    const float2 u = group_action(S, (unsigned)(p * G + g), g == 0, tk, k, n0, n1);
                    s0 += held[i] * (double)u.x;
                    s1 += held[i] * (double)u.y;
                }
            }
            if constexpr (N_HELD == 0) {
                for (int g = t; g < G; g += THREADS) {
                    const double w = weight_of(group_cost_of(S, cp + (size_t)g * E));
                    const float2 u = group_action(S, (unsigned)(p * G + g), g == 0, tk, k, n0, n1);
                    s0 += w * (double)u.x;
                    s1 += w * (double)u.y;
                }
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
        float v = nom[t];                              // 4. no finite group cost: the nominal stays
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

// What vine_mpc.hip refuses of a VineMpcConfig, in its words (restated: that unit keeps its validate to itself).
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

int validate_ensemble(const VineMpcConfig* c, const VineMpcEnsembleConfig* ec) {
    if (!ec) return vine_invalid_arg("mpc ensemble config is NULL");
    if (ec->abi_version != VINE_MPC_ENSEMBLE_ABI_VERSION) return vine_invalid_arg("VineMpcEnsembleConfig.abi_version mismatch");
    if (ec->members < 1 || ec->members > VINE_MPC_ENSEMBLE_MAX_MEMBERS)
        return vine_invalid_arg("mpc ensemble members must be in 1 .. VINE_MPC_ENSEMBLE_MAX_MEMBERS (16)");
    if (c->samples % ec->members != 0) return vine_invalid_arg("mpc ensemble members must divide samples of the VineMpcConfig");
    if (ec->risk != VINE_MPC_RISK_MEAN && ec->risk != VINE_MPC_RISK_MAX && ec->risk != VINE_MPC_RISK_ENTROPIC)
        return vine_invalid_arg("mpc ensemble risk must be VINE_MPC_RISK_MEAN, VINE_MPC_RISK_MAX or VINE_MPC_RISK_ENTROPIC");
    if (ec->risk == VINE_MPC_RISK_ENTROPIC && (!std::isfinite(ec->theta) || !(ec->theta > 0.0)))
        return vine_invalid_arg("mpc ensemble theta must be finite and positive with VINE_MPC_RISK_ENTROPIC");
    return VINE_OK;
}

int validate_both(const VineMpcConfig* cfg, const VineMpcEnsembleConfig* ecfg) {
    const int rc = validate(cfg);
    return rc ? rc : validate_ensemble(cfg, ecfg);
}

// The model handle's part of a launch's parameters; refuses a handle that does not hold num_plants * samples envs.
int prepare(VineHandle* model, const VineMpcConfig* cfg, const VineMpcEnsembleConfig* ecfg, VineHandleInfo& info,
            EnsembleParams& S) {
    int rc = vine_handle_info(model, &info);
    if (rc) return rc;
    if ((long long)info.n != (long long)cfg->num_plants * cfg->samples) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc: the model handle has %d envs, not num_plants * samples = %d * %d", info.n,
                 cfg->num_plants, cfg->samples);
        return vine_invalid_arg(msg);
    }
    S.n = info.n; S.m = cfg->num_plants; S.K = cfg->samples; S.H = cfg->horizon; S.glog = info.glog;
    S.E = ecfg->members; S.G = cfg->samples / ecfg->members; S.risk = ecfg->risk;
    S.seed_lo = (unsigned)cfg->seed; S.seed_hi = (unsigned)(cfg->seed >> 32);
    S.clip_act = info.clip_act;
    for (int a = 0; a < 2; ++a) S.c[a] = (float)((double)cfg->sigma[a] * noise_scale());
    S.lambda = cfg->lambda;
    S.theta = ecfg->risk == VINE_MPC_RISK_ENTROPIC ? ecfg->theta : 1.0;
    return VINE_OK;
}

}  // namespace

extern "C" {

int vine_mpc_ensemble_config_default(VineMpcEnsembleConfig* c) {
    if (!c) return vine_invalid_arg("mpc ensemble config is NULL");
    memset(c, 0, sizeof *c);                           // (the padding in front of theta too)
    c->abi_version = VINE_MPC_ENSEMBLE_ABI_VERSION;
    c->members = 4;
    c->risk = VINE_MPC_RISK_MEAN;
    c->theta = 1.0;
    return VINE_OK;
}

int vine_mpc_ensemble_config_size(void) { return (int)sizeof(VineMpcEnsembleConfig); }

int vine_mpc_ensemble_scheduled(VineHandle* model, const VineMpcConfig* cfg, const VineMpcEnsembleConfig* ecfg,
                                const float* nominal, const int64_t* tick, const int64_t* window, float* actions, void* stream) {
    int rc = validate_both(cfg, ecfg);
    if (rc) return rc;
    if (!model || !nominal || !tick || !window || !actions) return vine_invalid_arg("null argument to vine_mpc_ensemble_scheduled");
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(nominal)) & 7u)
        return vine_invalid_arg("mpc actions and nominal must be 8-byte aligned");
    VineHandleInfo info;
    EnsembleParams S;
    rc = prepare(model, cfg, ecfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_ensemble_node_kernel, dim3((S.n + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream,
                       S, info.counters, nominal, (const long long*)tick, (const long long*)window, actions);
    return vine_launch_status("vine_mpc_ensemble_scheduled");
}

int vine_mpc_ensemble_update(VineHandle* model, const VineMpcConfig* cfg, const VineMpcEnsembleConfig* ecfg, const double* cost,
                             const int64_t* plant_reset, float* nominal, float* history, int64_t* tick, float* plant_actions,
                             double* weights, double* group_cost, void* stream) {
    int rc = validate_both(cfg, ecfg);
    if (rc) return rc;
    if (!model || !cost || !plant_reset || !nominal || !history || !tick || !plant_actions)
        return vine_invalid_arg("null argument to vine_mpc_ensemble_update");
    if ((reinterpret_cast<uintptr_t>(plant_actions) | reinterpret_cast<uintptr_t>(history)) & 7u)
        return vine_invalid_arg("mpc plant_actions and history must be 8-byte aligned");
    VineHandleInfo info;
    EnsembleParams S;
    rc = prepare(model, cfg, ecfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    const auto kernel = S.G <= HELD * THREADS ? vine_mpc_ensemble_update_kernel<HELD> : vine_mpc_ensemble_update_kernel<0>;
    hipLaunchKernelGGL(kernel, dim3(S.m), dim3(THREADS), 0, (hipStream_t)stream, S, cost, (const long long*)plant_reset, nominal,
                       history, (long long*)tick, plant_actions, weights, group_cost);
    return vine_launch_status("vine_mpc_ensemble_update");
}

}  // extern "C"
