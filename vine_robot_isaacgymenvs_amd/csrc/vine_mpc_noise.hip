// vine_mpc_noise.hip — the predictive controller's sample distribution (MPC_NOISE) for MI355X (gfx950): perturbations
// correlated over the horizon and an amplitude per plant.  include/vine_mpc_noise.h states the semantics, utils/mpc_noise.py
// (colored_deviate, colored_actions, noise_replay) is the same statement in numpy.
//
// vine_mpc_noise_draw_kernel has one lane per (sample, component): 2 N lanes walk the horizon, one Philox call and one float
// per step, and a wave's 64 stores of a step are one contiguous segment of eps[k] (k is the table's outermost index).
// vine_mpc_noise_node_kernel has one lane per model env: it reads the step counter as every observer does (vine_observer.h
// vine_steps_completed) and returns at once outside the window; inside, a lane loads its plant's nominal entry and amplitude
// (8 B each, shared by the wave) and its own table entry (8 B, contiguous over the wave) and stores its action (8 B): no
// Philox call.  vine_mpc_noise_update_kernel is vine_mpc_update_kernel of vine_mpc.hip RESTATED -- that unit is not edited and
// its kernels take their actions from a function of the counter, not from a table -- with the action read from eps and sigma_p
// and two more float64 sums for the adapted amplitude: one workgroup per plant, lane-strided sums, a 64-wide butterfly per wave
// (vine_mpc_shared.h), the four wave sums through LDS and added in wave order.  No atomics anywhere; plain C++ stores only.
//
// CONTRACTION IS OFF FOR THIS TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it with
// -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): `b * eps + g * z` and `nominal + eps * c` must stay
// multiplies and adds, each rounded, as numpy forms them.  vine_task_shared.h is included as vine_mpc.hip includes it; of it
// this unit uses clampf alone, which has nothing to contract.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/vine_env_params.h"
#include "../../include/vine_mpc_noise.h"
#include "vine_observer.h"
#include "vine_policy_head.h"
#pragma clang fp contract(fast)
#include "vine_task_shared.h"
#pragma clang fp contract(off)
// the reduction's wave step, the deviate's integer and its scale: stated once for the vine_mpc*.hip units
#include "vine_mpc_shared.h"

namespace {

constexpr int THREADS = VINE_MPC_NOISE_THREADS;
constexpr int WAVES = THREADS / 64;
constexpr int HMAX = VINE_MPC_MAX_HORIZON;
static_assert(THREADS == VINE_MPC_THREADS && 2 * HMAX <= THREADS, "one lane of the update per nominal entry");

struct NoiseParams {
    int n, m, K, H, glog, adapt;           // model envs, plants, samples, horizon; the MODEL handle's counter shift
    unsigned seed_lo, seed_hi;
    float clip_act;                        // the MODEL handle's clipActions
    float b[2], g[2];                      // beta[a] and float32(sqrt(1 - beta[a]^2))
    float sigma0[2], sigma_min[2], sigma_max[2];
    double k0, lambda, rate;               // the deviate's scale (vine_mpc_shared.h noise_scale)
};

// c_p[a] of a plant's amplitude: float32((double)sigma_p[p][a] * K0)
__device__ __forceinline__ float2 noise_scale_of(const NoiseParams& S, float2 sg) {
    return make_float2((float)((double)sg.x * S.k0), (float)((double)sg.y * S.k0));
}

// u'[j][k] around the nominal entry (nom0, nom1): include/vine_mpc_noise.h, 2. THE NODE.
__device__ __forceinline__ float2 noise_action(const NoiseParams& S, float2 ep, float2 c, float nom0, float nom1) {
    const float zc0 = ep.x * c.x, zc1 = ep.y * c.y;
    const float x0 = nom0 + zc0, x1 = nom1 + zc1;
    return make_float2(clampf(x0, S.clip_act), clampf(x1, S.clip_act));
}

__global__ __launch_bounds__(THREADS) void vine_mpc_noise_draw_kernel(const NoiseParams S, const long long* __restrict__ tick,
                                                                      float* __restrict__ eps) {
    const long long total = 2LL * S.n;                                 // floats per horizon step
    const long long i = (long long)blockIdx.x * THREADS + (long long)threadIdx.x;      // 2 e + a
    if (i >= total) return;
    const int e = (int)(i >> 1), a = (int)(i & 1);
    const int p = e / S.K, j = e - p * S.K;
    if (j == 0) {                                                      // sample 0 is the nominal itself
        for (int k = 0; k < S.H; ++k) eps[(size_t)k * (size_t)total + (size_t)i] = 0.0f;
        return;
    }
    const unsigned long long t = (unsigned long long)tick[p];
    const float b = a ? S.b[1] : S.b[0], g = a ? S.g[1] : S.g[0];
    float prev = 0.0f;
    for (int k = 0; k < S.H; ++k) {
        unsigned w[4];
        philox4x32_10((unsigned)e, (unsigned)t, VINE_MPC_RNG_NOISE | ((unsigned)(t >> 32) << 8), (unsigned)(2 * k + a), S.seed_lo,
                      S.seed_hi, w);
        const float z = (float)mpc_deviate_int(w);
        float v = z;
        if (k > 0) {
            const float bz = b * prev, gz = g * z;
            v = bz + gz;
        }
        eps[(size_t)k * (size_t)total + (size_t)i] = v;
        prev = v;
    }
}

__global__ __launch_bounds__(THREADS) void vine_mpc_noise_node_kernel(const NoiseParams S,
                                                                      const unsigned long long* __restrict__ counters,
                                                                      const float* __restrict__ nominal,
                                                                      const long long* __restrict__ window,
                                                                      const float* __restrict__ eps,
                                                                      const float* __restrict__ sigma_p, float* __restrict__ actions) {
    const long long c = (long long)vine_steps_completed(counters, S.glog);
    const long long k = c - window[0];
    if (k < 0 || k >= (long long)S.H) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S.n) return;
    const int p = e / S.K;
    const float2 nom = reinterpret_cast<const float2*>(nominal)[(size_t)p * S.H + (int)k];
    const float2 ep = reinterpret_cast<const float2*>(eps)[(size_t)k * S.n + e];
    const float2 cp = noise_scale_of(S, reinterpret_cast<const float2*>(sigma_p)[p]);
    reinterpret_cast<float2*>(actions)[e] = noise_action(S, ep, cp, nom.x, nom.y);
}

// vine_mpc_update_kernel of vine_mpc.hip, restated: `u` is u' of the table, and with adapt the sums q_a ride in its loop.
__global__ __launch_bounds__(THREADS) void vine_mpc_noise_update_kernel(const NoiseParams S, const double* __restrict__ cost,
                                                                        const long long* __restrict__ plant_reset,
                                                                        const float* __restrict__ eps, float* __restrict__ nominal,
                                                                        float* __restrict__ history, long long* __restrict__ tick,
                                                                        float* __restrict__ plant_actions,
                                                                        float* __restrict__ sigma_p, double* __restrict__ weights) {
    __shared__ float nom[2 * HMAX];                    // nominal[p], read before anything is written
    __shared__ float fresh[2 * HMAX];                  // new[k][a]
    __shared__ double part_min[WAVES];
    __shared__ double part_w[WAVES];
    __shared__ double part_u[2 * HMAX][WAVES];
    __shared__ double part_q[2][WAVES];
    const int p = blockIdx.x, t = (int)threadIdx.x, K = S.K, H = S.H;
    const int wave = t >> 6, lane = t & 63;
    if (t < 2 * H) nom[t] = nominal[(size_t)p * 2 * H + t];
    const long long tk = tick[p];
    const float2 sg = reinterpret_cast<const float2*>(sigma_p)[p];     // read by every lane before the first barrier
    const float2 cs = noise_scale_of(S, sg);
    const double* __restrict__ cp = cost + (size_t)p * K;
    const float2* __restrict__ ep = reinterpret_cast<const float2*>(eps) + (size_t)p * K;     // + k * n + j

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
        // 2. the weights' sum; 3. per (k, a) the weighted sum of u': a lane goes through its samples in ascending j
        double sw = 0.0;
        for (int j = t; j < K; j += THREADS) {
            const double cj = cp[j];
            const double w = cj < INFINITY ? exp(-(cj - beta) / S.lambda) : 0.0;
            if (weights) weights[(size_t)p * K + j] = w;
            sw += w;
        }
        sw = wave_sum(sw);
        if (lane == 0) part_w[wave] = sw;
        double q0 = 0.0, q1 = 0.0;                     // with adapt: sum_k sum_j w_j d^2 of this lane's samples, k outer
        for (int k = 0; k < H; ++k) {
            double s0 = 0.0, s1 = 0.0;
            const float n0 = nom[2 * k], n1 = nom[2 * k + 1];
            for (int j = t; j < K; j += THREADS) {
                const double cj = cp[j];
                const double w = cj < INFINITY ? exp(-(cj - beta) / S.lambda) : 0.0;
                const float2 u = noise_action(S, ep[(size_t)k * S.n + j], cs, n0, n1);
                s0 += w * (double)u.x;
                s1 += w * (double)u.y;
                if (S.adapt) {
                    const double d0 = (double)u.x - (double)n0, d1 = (double)u.y - (double)n1;
                    q0 += w * (d0 * d0);
                    q1 += w * (d1 * d1);
                }
            }
            s0 = wave_sum(s0);
            s1 = wave_sum(s1);
            if (lane == 0) {
                part_u[2 * k][wave] = s0;
                part_u[2 * k + 1][wave] = s1;
            }
        }
        if (S.adapt) {
            q0 = wave_sum(q0);
            q1 = wave_sum(q1);
            if (lane == 0) {
                part_q[0][wave] = q0;
                part_q[1][wave] = q1;
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
    if (S.adapt && t < 2) {                            // lane a: the amplitude of component a
        if (consumed) {
            sigma_p[(size_t)p * 2 + t] = S.sigma0[t];
        } else if (any) {
            double sw = part_w[0], q = part_q[t][0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) {
                sw += part_w[w];
                q += part_q[t][w];
            }
            const double v = q / (sw * (double)H);
            const double s = (double)(t ? sg.y : sg.x);
            const double mixed = sqrt((1.0 - S.rate) * s * s + S.rate * v);
            sigma_p[(size_t)p * 2 + t] = (float)fmin(fmax(mixed, (double)S.sigma_min[t]), (double)S.sigma_max[t]);
        }                                              // no finite cost: the amplitude keeps its bits
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

int validate_noise(const VineMpcConfig* c, const VineMpcNoiseConfig* nc) {
    if (!nc) return vine_invalid_arg("mpc noise config is NULL");
    if (nc->abi_version != VINE_MPC_NOISE_ABI_VERSION) return vine_invalid_arg("VineMpcNoiseConfig.abi_version mismatch");
    for (int a = 0; a < 2; ++a)
        if (!std::isfinite(nc->beta[a]) || nc->beta[a] < 0.0f || !(nc->beta[a] < 1.0f))
            return vine_invalid_arg("mpc noise beta must be finite and in [0, 1)");
    if (nc->adapt && (!std::isfinite(nc->rate) || !(nc->rate > 0.0) || nc->rate > 1.0))
        return vine_invalid_arg("mpc noise rate must be in (0, 1] with adapt");
    for (int a = 0; a < 2; ++a) {
        if (!std::isfinite(nc->sigma_min[a]) || nc->sigma_min[a] < 0.0f)
            return vine_invalid_arg("mpc noise sigma_min must be finite and not negative");
        if (!std::isfinite(nc->sigma_max[a])) return vine_invalid_arg("mpc noise sigma_max must be finite");
        if (!(nc->sigma_min[a] <= c->sigma[a] && c->sigma[a] <= nc->sigma_max[a]))
            return vine_invalid_arg("mpc noise needs sigma_min <= sigma <= sigma_max, sigma of the VineMpcConfig");
    }
    return VINE_OK;
}

// The model handle's part of a launch's parameters; refuses a handle that does not hold num_plants * samples envs.
int prepare(VineHandle* model, const VineMpcConfig* cfg, const VineMpcNoiseConfig* ncfg, VineHandleInfo& info, NoiseParams& S) {
    int rc = vine_handle_info(model, &info);
    if (rc) return rc;
    if ((long long)info.n != (long long)cfg->num_plants * cfg->samples) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc: the model handle has %d envs, not num_plants * samples = %d * %d", info.n,
                 cfg->num_plants, cfg->samples);
        return vine_invalid_arg(msg);
    }
    S.n = info.n; S.m = cfg->num_plants; S.K = cfg->samples; S.H = cfg->horizon; S.glog = info.glog; S.adapt = ncfg->adapt ? 1 : 0;
    S.seed_lo = (unsigned)cfg->seed; S.seed_hi = (unsigned)(cfg->seed >> 32);
    S.clip_act = info.clip_act;
    for (int a = 0; a < 2; ++a) {
        S.b[a] = ncfg->beta[a];
        S.g[a] = (float)sqrt(1.0 - (double)ncfg->beta[a] * (double)ncfg->beta[a]);
        S.sigma0[a] = cfg->sigma[a];
        S.sigma_min[a] = ncfg->sigma_min[a];
        S.sigma_max[a] = ncfg->sigma_max[a];
    }
    S.k0 = noise_scale();
    S.lambda = cfg->lambda;
    S.rate = ncfg->rate;
    return VINE_OK;
}

int validate_both(const VineMpcConfig* cfg, const VineMpcNoiseConfig* ncfg) {
    const int rc = validate(cfg);
    return rc ? rc : validate_noise(cfg, ncfg);
}

}  // namespace

extern "C" {

int vine_mpc_noise_config_default(VineMpcNoiseConfig* c) {
    if (!c) return vine_invalid_arg("mpc noise config is NULL");
    c->abi_version = VINE_MPC_NOISE_ABI_VERSION;
    c->beta[0] = c->beta[1] = 0.0f;
    c->adapt = 0;
    c->rate = 0.2;
    c->sigma_min[0] = c->sigma_min[1] = 0.0f;
    c->sigma_max[0] = c->sigma_max[1] = 3.402823466e+38f;      // FLT_MAX
    return VINE_OK;
}

int vine_mpc_noise_config_size(void) { return (int)sizeof(VineMpcNoiseConfig); }

int vine_mpc_noise_draw(VineHandle* model, const VineMpcConfig* cfg, const VineMpcNoiseConfig* ncfg, const int64_t* tick,
                        float* eps, void* stream) {
    int rc = validate_both(cfg, ncfg);
    if (rc) return rc;
    if (!model || !tick || !eps) return vine_invalid_arg("null argument to vine_mpc_noise_draw");
    if (reinterpret_cast<uintptr_t>(eps) & 7u) return vine_invalid_arg("mpc eps must be 8-byte aligned");
    VineHandleInfo info;
    NoiseParams S;
    rc = prepare(model, cfg, ncfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    const long long total = 2LL * S.n;
    hipLaunchKernelGGL(vine_mpc_noise_draw_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                       (hipStream_t)stream, S, (const long long*)tick, eps);
    return vine_launch_status("vine_mpc_noise_draw");
}

int vine_mpc_noise_scheduled(VineHandle* model, const VineMpcConfig* cfg, const VineMpcNoiseConfig* ncfg, const float* nominal,
                             const int64_t* window, const float* eps, const float* sigma_p, float* actions, void* stream) {
    int rc = validate_both(cfg, ncfg);
    if (rc) return rc;
    if (!model || !nominal || !window || !eps || !sigma_p || !actions)
        return vine_invalid_arg("null argument to vine_mpc_noise_scheduled");
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(nominal) | reinterpret_cast<uintptr_t>(eps) |
         reinterpret_cast<uintptr_t>(sigma_p)) & 7u)
        return vine_invalid_arg("mpc actions, nominal, eps and sigma_p must be 8-byte aligned");
    VineHandleInfo info;
    NoiseParams S;
    rc = prepare(model, cfg, ncfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_noise_node_kernel, dim3((S.n + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, S,
                       info.counters, nominal, (const long long*)window, eps, sigma_p, actions);
    return vine_launch_status("vine_mpc_noise_scheduled");
}

int vine_mpc_noise_update(VineHandle* model, const VineMpcConfig* cfg, const VineMpcNoiseConfig* ncfg, const double* cost,
                          const int64_t* plant_reset, const float* eps, float* nominal, float* history, int64_t* tick,
                          float* plant_actions, float* sigma_p, double* weights, void* stream) {
    int rc = validate_both(cfg, ncfg);
    if (rc) return rc;
    if (!model || !cost || !plant_reset || !eps || !nominal || !history || !tick || !plant_actions || !sigma_p)
        return vine_invalid_arg("null argument to vine_mpc_noise_update");
    if ((reinterpret_cast<uintptr_t>(plant_actions) | reinterpret_cast<uintptr_t>(history) | reinterpret_cast<uintptr_t>(eps) |
         reinterpret_cast<uintptr_t>(sigma_p)) & 7u)
        return vine_invalid_arg("mpc plant_actions, history, eps and sigma_p must be 8-byte aligned");
    VineHandleInfo info;
    NoiseParams S;
    rc = prepare(model, cfg, ncfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_noise_update_kernel, dim3(S.m), dim3(THREADS), 0, (hipStream_t)stream, S, cost,
                       (const long long*)plant_reset, eps, nominal, history, (long long*)tick, plant_actions, sigma_p, weights);
    return vine_launch_status("vine_mpc_noise_update");
}

}  // extern "C"
