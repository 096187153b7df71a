// vine_mpc_adapt.hip — online adaptation of the predictive controller's model for MI355X (gfx950): include/vine_mpc_adapt.h
// states the semantics, utils/mpc_adapt.py (candidates, score, estimate) is the same statement in numpy.
//
// vine_mpc_adapt_anchor_kernel and vine_mpc_adapt_trace_kernel are one lane per PLANT (M lanes: a copy of a column, twelve
// floats and an action).  vine_mpc_adapt_pin_kernel and vine_mpc_adapt_node_kernel are one lane per model env, 256 lanes per
// workgroup, over the SoA state block and the SoA parameter table (table[row * n + e]: a wave writes 64 contiguous floats
// per row).  The node reads the step counter as the other observers do and returns at once outside the window.
// vine_mpc_adapt_estimate_kernel is one workgroup per plant with the reduction of vine_mpc_update_kernel.  The candidate
// value is recomputed wherever it is needed (one Philox call per sample and dimension) and never stored.  No atomics
// anywhere; plain C++ stores only.
//
// CONTRACTION IS OFF FOR THIS TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it with
// -ffp-contract=fast-honor-pragmas): `mean + z * std`, `(1 - rate) * mean + rate * m` and the score's sum must stay the
// multiplies and adds numpy forms.  The one exception is vine_task_shared.h, included under contract(fast): task_new_command
// must give the words the step kernels put into the delay ring.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/vine_env_params.h"
#include "../../include/vine_mpc_adapt.h"
#include "vine_observer.h"
#include "vine_policy_head.h"
#pragma clang fp contract(fast)
#include "vine_task_shared.h"
#pragma clang fp contract(off)
#include "vine_mpc_shared.h"

namespace {

constexpr int THREADS = VINE_MPC_THREADS;
constexpr int WAVES = THREADS / 64;
constexpr int DMAX = VINE_MPC_ADAPT_MAX_DIMS;
constexpr int NF = VINE_MPC_ADAPT_FIELDS;
static_assert(THREADS == 256 && DMAX <= 64, "one lane of the estimate per dimension");
static_assert(VF_QD0 == VF_Q0 + VINE_NUM_DOFS && NF == 2 * VINE_NUM_DOFS, "the compared fields are twelve consecutive ones");
static_assert(VP_COUNT - VP_FPAM_K0 == VINE_MPC_ADAPT_BASE_ROWS, "base_rows covers the four FPAM vectors");

struct AdaptDim {
    int first, count;
    double lo, hi, floor;
};

struct AdaptParams {
    int n, m, K, W, D, min_steps, forget, glog, delay;   // glog, delay: of the handle the launch reads its step count from
    unsigned seed_lo, seed_hi;
    double k0, temperature, rate;
    float w[NF];
    float base[VINE_MPC_ADAPT_BASE_ROWS];
    AdaptDim dim[DMAX];
    CommandParams cmd;                                   // the model configuration's
};


// theta of sample e (candidate j of its plant) in dimension d during pass `pass`: include/vine_mpc_adapt.h CANDIDATES.
__device__ __forceinline__ double adapt_theta(const AdaptParams& S, unsigned e, bool first, long long pass, int d, double mean,
                                              double std) {
    float z = 0.0f;
    if (!first) {
        const unsigned long long t = (unsigned long long)pass;
        unsigned w[4];
        philox4x32_10(e, (unsigned)t, VINE_MPC_ADAPT_RNG | ((unsigned)(t >> 32) << 8), (unsigned)d, S.seed_lo, S.seed_hi, w);
        z = (float)((double)mpc_deviate_int(w) * S.k0);
    }
    const double zs = (double)z * std;
    const double x = mean + zs;
    return fmin(fmax(x, S.dim[d].lo), S.dim[d].hi);
}

// The table rows of dimension d for the value theta, in the rounding of env_params.set_rows.
__device__ __forceinline__ void adapt_write_rows(const AdaptParams& S, int d, double theta, float* table, int e) {
    const int first = S.dim[d].first, count = S.dim[d].count;
    if (count == 1) {
        table[(size_t)first * S.n + e] = (float)theta;
    } else {
        for (int r = 0; r < count; ++r) {
            const double v = (double)S.base[first - VP_FPAM_K0 + r] * theta;
            table[(size_t)(first + r) * S.n + e] = (float)v;
        }
    }
}

__global__ __launch_bounds__(THREADS) void vine_mpc_adapt_anchor_kernel(
    const AdaptParams S, const float* __restrict__ pst, const unsigned long long* __restrict__ counters,
    const long long* __restrict__ plant_progress, const long long* __restrict__ plant_reset, const float* __restrict__ history,
    float* __restrict__ anchor_state, float* __restrict__ anchor_history, long long* __restrict__ anchor_progress,
    long long* __restrict__ anchor_count, int* __restrict__ trace_len, unsigned char* __restrict__ trace_open,
    unsigned char* __restrict__ episode_ended) {
    const int m = S.m, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) anchor_count[0] = (long long)vine_steps_completed(counters, S.glog);
    if (p >= m) return;
    for (int f = 0; f < VF_COUNT; ++f) anchor_state[(size_t)f * m + p] = pst[(size_t)f * m + p];
    for (int i = 0; i < 2 * VINE_MAX_DELAY; ++i)
        anchor_history[(size_t)p * 2 * VINE_MAX_DELAY + i] = history[(size_t)p * 2 * VINE_MAX_DELAY + i];
    anchor_progress[p] = plant_progress[p];
    trace_len[p] = 0;
    trace_open[p] = plant_reset[p] == 0 ? 1 : 0;
    episode_ended[p] = 0;
}

__global__ __launch_bounds__(THREADS) void vine_mpc_adapt_trace_kernel(
    const AdaptParams S, const float* __restrict__ pst, const unsigned long long* __restrict__ counters,
    const float* __restrict__ plant_actions, const long long* __restrict__ plant_reset, const float* __restrict__ plant_rew,
    const long long* __restrict__ anchor_count, float* __restrict__ trace_actions, float* __restrict__ trace_rows,
    int* __restrict__ trace_len, unsigned char* __restrict__ trace_open, unsigned char* __restrict__ episode_ended,
    double* __restrict__ returns) {
    const long long s = (long long)vine_steps_completed(counters, S.glog) - anchor_count[0];
    if (s < 1) return;
    const int m = S.m, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const bool raised = plant_reset[p] != 0;
    if (s <= (long long)S.W && trace_open[p]) {
        const size_t slot = (size_t)p * S.W + (size_t)(s - 1);
        trace_actions[2 * slot] = plant_actions[2 * p];
        trace_actions[2 * slot + 1] = plant_actions[2 * p + 1];
        for (int f = 0; f < NF; ++f) trace_rows[slot * NF + f] = pst[(size_t)(VF_Q0 + f) * m + p];
        trace_len[p] = (int)s;
        if (raised) trace_open[p] = 0;                    // the step that ends an episode is still a valid row
    }
    if (raised) episode_ended[p] = 1;
    if (returns) returns[p] += (double)plant_rew[p];
}

__global__ __launch_bounds__(THREADS) void vine_mpc_adapt_pin_kernel(
    const AdaptParams S, float* __restrict__ st, const unsigned long long* __restrict__ counters, float* table,
    const double* __restrict__ mean, const double* __restrict__ std, const long long* __restrict__ passes,
    const float* __restrict__ anchor_state, const float* __restrict__ anchor_history,
    const long long* __restrict__ anchor_progress, const float* __restrict__ trace_actions, float* __restrict__ actions,
    float* __restrict__ rew, long long* __restrict__ reset, long long* __restrict__ progress, double* __restrict__ err,
    unsigned char* __restrict__ alive, long long* __restrict__ window) {
    const unsigned long long c = vine_steps_completed(counters, S.glog);
    const int n = S.n, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) window[0] = (long long)c;
    if (e >= n) return;
    const int p = e / S.K, j = e - p * S.K;
    const long long pass = passes[p];
    for (int d = 0; d < S.D; ++d)
        adapt_write_rows(S, d, adapt_theta(S, (unsigned)e, j == 0, pass, d, mean[(size_t)p * S.D + d], std[(size_t)p * S.D + d]),
                         table, e);
    MPC_COPY_COLUMN(anchor_state, S.m, p, st, n, e);
    // the delay ring: this sample's delay and action -> command constants, read behind the lane's own candidate rows
    CommandParams P = S.cmd;
    P.rail_scale = table[(size_t)VP_RAIL_VELOCITY_SCALE * n + e];
    const int dl = min(max((int)table[(size_t)VP_ACTION_DELAY * n + e], 0), VINE_MAX_DELAY);
    mpc_rebuild_ring(P, dl, c, reinterpret_cast<const float2*>(anchor_history) + (size_t)p * VINE_MAX_DELAY, st, n, e);
    reinterpret_cast<float2*>(actions)[e] = reinterpret_cast<const float2*>(trace_actions)[(size_t)p * S.W];
    rew[e] = 0.0f;
    reset[e] = 0;
    progress[e] = anchor_progress[p];
    err[e] = 0.0;
    alive[e] = 1;
}

__global__ __launch_bounds__(THREADS) void vine_mpc_adapt_node_kernel(
    const AdaptParams S, const float* __restrict__ st, const unsigned long long* __restrict__ counters,
    const float* __restrict__ trace_actions, const float* __restrict__ trace_rows, const int* __restrict__ trace_len,
    const long long* __restrict__ window, float* __restrict__ actions, const long long* __restrict__ reset,
    double* __restrict__ err, unsigned char* __restrict__ alive) {
    const long long c = (long long)vine_steps_completed(counters, S.glog);
    const long long k = c - window[0];
    if (k < 1 || k > (long long)S.W) return;
    const int n = S.n, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int p = e / S.K;
    const int tl = min(max(trace_len[p], 0), S.W);        // (slots stay inside the trace whatever the word holds)
    if (k <= (long long)tl && alive[e]) {
        const float* __restrict__ row = trace_rows + ((size_t)p * S.W + (size_t)(k - 1)) * NF;
        double sum = 0.0;
        bool finite = true;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (S.w[f] != 0.0f) {
                const float x = st[(size_t)(VF_Q0 + f) * n + e];
                finite &= isfinite(x);
                const double dx = (double)x - (double)row[f];
                sum += (double)S.w[f] * (dx * dx);
            }
        }
        if (!finite) {
            err[e] = INFINITY;
            alive[e] = 0;
        } else {
            const double total = err[e] + sum;
            const bool left = reset[e] != 0 && k < (long long)tl;      // left the episode before the plant did
            err[e] = left ? (double)INFINITY : total;
            if (left) alive[e] = 0;
        }
    }
    if (tl > 0) {
        const int slot = (int)min(k, (long long)(tl - 1));
        reinterpret_cast<float2*>(actions)[e] = reinterpret_cast<const float2*>(trace_actions)[(size_t)p * S.W + slot];
    }
}

// The sum (or the minimum) of one value per lane over the workgroup in the order of vine_mpc_update_kernel: the wave's
// butterfly, the four wave values through LDS, combined in wave order.  Every lane returns the same bits.  `part` is WAVES
// doubles of LDS; the second barrier lets the next call reuse them.
__device__ __forceinline__ double block_sum(double v, double* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = part[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += part[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ double block_min(double v, double* part) {
    v = wave_min(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = part[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s = fmin(s, part[w]);
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(THREADS) void vine_mpc_adapt_estimate_kernel(
    const AdaptParams S, float* __restrict__ table, const double* __restrict__ err, const int* __restrict__ trace_len,
    const unsigned char* __restrict__ episode_ended, double* __restrict__ mean, double* __restrict__ std,
    const double* __restrict__ prior_mean, const double* __restrict__ prior_std, long long* __restrict__ passes,
    double* __restrict__ weights) {
    __shared__ double old_mean[DMAX], old_std[DMAX];     // mean[p], std[p], read before anything is written
    __shared__ double new_mean[DMAX];
    __shared__ double part[WAVES];
    const int p = blockIdx.x, t = (int)threadIdx.x, K = S.K, D = S.D;
    if (t < D) {
        old_mean[t] = mean[(size_t)p * D + t];
        old_std[t] = std[(size_t)p * D + t];
    }
    const long long pass = passes[p];
    const double* __restrict__ ep = err + (size_t)p * K;
    __syncthreads();

    double lo = INFINITY, cnt = 0.0, tot = 0.0;
    for (int j = t; j < K; j += THREADS) {
        const double ej = ep[j];
        lo = fmin(lo, ej);
        if (ej < INFINITY) {
            cnt += 1.0;
            tot += ej;
        }
    }
    const double beta = block_min(lo, part);
    cnt = block_sum(cnt, part);
    tot = block_sum(tot, part);
    // all three uniform over the workgroup
    const bool forget = S.forget != 0 && episode_ended[p] != 0;
    const bool estimated = !forget && trace_len[p] >= S.min_steps && beta < INFINITY;

    if (estimated) {
        const double ebar = tot / cnt;
        const double tau = S.temperature * (ebar - beta);
        double sw = 0.0;
        for (int j = t; j < K; j += THREADS) {
            const double ej = ep[j];
            const double w = ej < INFINITY ? (tau > 0.0 ? exp(-(ej - beta) / tau) : 1.0) : 0.0;
            if (weights) weights[(size_t)p * K + j] = w;
            sw += w;
        }
        sw = block_sum(sw, part);
        for (int d = 0; d < D; ++d) {
            const double m0 = old_mean[d], s0 = old_std[d];
            double a = 0.0;
            for (int j = t; j < K; j += THREADS) {
                const double ej = ep[j];
                const double w = ej < INFINITY ? (tau > 0.0 ? exp(-(ej - beta) / tau) : 1.0) : 0.0;
                a += w * adapt_theta(S, (unsigned)(p * K + j), j == 0, pass, d, m0, s0);
            }
            const double md = block_sum(a, part) / sw;
            double b = 0.0;
            for (int j = t; j < K; j += THREADS) {
                const double ej = ep[j];
                const double w = ej < INFINITY ? (tau > 0.0 ? exp(-(ej - beta) / tau) : 1.0) : 0.0;
                const double dv = adapt_theta(S, (unsigned)(p * K + j), j == 0, pass, d, m0, s0) - md;
                b += w * (dv * dv);
            }
            const double vd = block_sum(b, part) / sw;
            if (t == 0) {
                const double keep = 1.0 - S.rate;
                const double nm = keep * m0 + S.rate * md;
                const double ns = fmax(keep * s0 + S.rate * sqrt(vd), S.dim[d].floor);
                new_mean[d] = nm;
                mean[(size_t)p * D + d] = nm;
                std[(size_t)p * D + d] = ns;
            }
        }
    } else {
        if (weights)
            for (int j = t; j < K; j += THREADS) weights[(size_t)p * K + j] = 0.0;
        if (t < D) {
            const double nm = forget ? prior_mean[(size_t)p * D + t] : old_mean[t];
            new_mean[t] = nm;
            if (forget) {
                mean[(size_t)p * D + t] = nm;
                std[(size_t)p * D + t] = prior_std[(size_t)p * D + t];
            }
        }
    }
    __syncthreads();
    // the planning value: the candidates' statement at z = 0 on the new mean, into the rows of all K samples
    for (int d = 0; d < D; ++d) {
        const double plan = fmin(fmax(new_mean[d], S.dim[d].lo), S.dim[d].hi);
        for (int j = t; j < K; j += THREADS) adapt_write_rows(S, d, plan, table, p * K + j);
    }
    if (t == 0) passes[p] = pass + 1;
}

int validate(const VineMpcAdaptConfig* c) {
    if (!c) return vine_invalid_arg("mpc adapt config is NULL");
    if (c->abi_version != VINE_MPC_ADAPT_ABI_VERSION) return vine_invalid_arg("VineMpcAdaptConfig.abi_version mismatch");
    if (c->num_plants < 1) return vine_invalid_arg("mpc adapt num_plants must be at least 1");
    if (c->samples < 2) return vine_invalid_arg("mpc adapt samples must be at least 2");
    if ((long long)c->num_plants * c->samples > 0x7fffffffLL)
        return vine_invalid_arg("mpc adapt num_plants * samples does not fit an int32");
    if (c->window < 1 || c->window > VINE_MPC_ADAPT_MAX_WINDOW)
        return vine_invalid_arg("mpc adapt needs 1 <= window <= VINE_MPC_ADAPT_MAX_WINDOW (32)");
    if (c->every < c->window) return vine_invalid_arg("mpc adapt needs window <= every");
    if (c->num_dims < 1 || c->num_dims > VINE_MPC_ADAPT_MAX_DIMS)
        return vine_invalid_arg("mpc adapt needs 1 <= num_dims <= VINE_MPC_ADAPT_MAX_DIMS (8)");
    if (c->min_steps < 1 || c->min_steps > c->window) return vine_invalid_arg("mpc adapt needs 1 <= min_steps <= window");
    if (c->forget_on_reset != 0 && c->forget_on_reset != 1) return vine_invalid_arg("mpc adapt forget_on_reset must be 0 or 1");
    if (!std::isfinite(c->temperature) || !(c->temperature > 0.0))
        return vine_invalid_arg("mpc adapt temperature must be finite and positive");
    if (!std::isfinite(c->rate) || !(c->rate > 0.0) || c->rate > 1.0) return vine_invalid_arg("mpc adapt needs 0 < rate <= 1");
    for (int f = 0; f < VINE_MPC_ADAPT_FIELDS; ++f)
        if (!std::isfinite(c->weights[f]) || c->weights[f] < 0.0f)
            return vine_invalid_arg("mpc adapt weights must be finite and not negative");
    for (int r = 0; r < VINE_MPC_ADAPT_BASE_ROWS; ++r)
        if (!std::isfinite(c->base_rows[r])) return vine_invalid_arg("mpc adapt base_rows must be finite");
    unsigned taken = 0;                                   // one bit per table row
    for (int d = 0; d < c->num_dims; ++d) {
        const VineMpcAdaptDim& m = c->dims[d];
        char msg[200];
        if (m.first_row == VP_ACTION_DELAY && m.num_rows == 1)
            return unsupported("mpc adapt: ACTION_DELAY is refused (an integer: its belief is not Gaussian)");
        const bool scalar = m.num_rows == 1 && m.first_row >= 0 && m.first_row < VP_ACTION_DELAY;
        const bool fpam = m.num_rows == 5 && (m.first_row == VP_FPAM_K0 || m.first_row == VP_FPAM_C0 ||
                                              m.first_row == VP_FPAM_b0 || m.first_row == VP_FPAM_B0);
        if (!scalar && !fpam) {
            snprintf(msg, sizeof msg, "mpc adapt dims[%d]: rows %d .. +%d are neither one scalar row nor one FPAM vector", d,
                     m.first_row, m.num_rows);
            return vine_invalid_arg(msg);
        }
        if (!std::isfinite(m.lo) || !std::isfinite(m.hi) || m.lo > m.hi) {
            snprintf(msg, sizeof msg, "mpc adapt dims[%d]: needs finite lo <= hi", d);
            return vine_invalid_arg(msg);
        }
        if (!std::isfinite(m.std_floor) || m.std_floor < 0.0) {
            snprintf(msg, sizeof msg, "mpc adapt dims[%d]: std_floor must be finite and not negative", d);
            return vine_invalid_arg(msg);
        }
        const unsigned bits = ((1u << m.num_rows) - 1u) << m.first_row;
        if (taken & bits) {
            snprintf(msg, sizeof msg, "mpc adapt dims[%d]: overlaps an earlier dimension", d);
            return vine_invalid_arg(msg);
        }
        taken |= bits;
    }
    return VINE_OK;
}

void fill(const VineMpcAdaptConfig* cfg, const VineHandleInfo& info, AdaptParams& S) {
    S.m = cfg->num_plants; S.K = cfg->samples; S.n = S.m * S.K; S.W = cfg->window; S.D = cfg->num_dims;
    S.min_steps = cfg->min_steps; S.forget = cfg->forget_on_reset; S.glog = info.glog; S.delay = info.delay;
    S.seed_lo = (unsigned)cfg->seed; S.seed_hi = (unsigned)(cfg->seed >> 32);
    S.k0 = noise_scale(); S.temperature = cfg->temperature; S.rate = cfg->rate;
    for (int f = 0; f < NF; ++f) S.w[f] = cfg->weights[f];
    for (int r = 0; r < VINE_MPC_ADAPT_BASE_ROWS; ++r) S.base[r] = cfg->base_rows[r];
    for (int d = 0; d < DMAX; ++d) {
        const bool on = d < cfg->num_dims;
        S.dim[d].first = on ? cfg->dims[d].first_row : 0;
        S.dim[d].count = on ? cfg->dims[d].num_rows : 0;
        S.dim[d].lo = on ? cfg->dims[d].lo : 0.0;
        S.dim[d].hi = on ? cfg->dims[d].hi : 0.0;
        S.dim[d].floor = on ? cfg->dims[d].std_floor : 0.0;
    }
    S.cmd = mpc_command_params(info);
}

// The plant handle's part of a launch's parameters; refuses a handle that does not hold num_plants envs.
int prepare_plant(VineHandle* plant, const VineMpcAdaptConfig* cfg, VineHandleInfo& info, AdaptParams& S) {
    int rc = vine_handle_info(plant, &info);
    if (rc) return rc;
    if (info.n != cfg->num_plants) return vine_invalid_arg("mpc adapt: the plant handle does not have num_plants envs");
    fill(cfg, info, S);
    return VINE_OK;
}

// The model handle's; refuses a handle that does not hold num_plants * samples envs or has no parameter table bound.
int prepare_model(VineHandle* model, const VineMpcAdaptConfig* cfg, VineHandleInfo& info, AdaptParams& S) {
    int rc = vine_handle_info(model, &info);
    if (rc) return rc;
    if ((long long)info.n != (long long)cfg->num_plants * cfg->samples) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc adapt: the model handle has %d envs, not num_plants * samples = %d * %d", info.n,
                 cfg->num_plants, cfg->samples);
        return vine_invalid_arg(msg);
    }
    if (!info.env_params)
        return unsupported("mpc adapt: the model handle has no per-env parameter table bound (the table is what is adapted)");
    fill(cfg, info, S);
    return VINE_OK;
}

}  // namespace

extern "C" {

int vine_mpc_adapt_config_default(VineMpcAdaptConfig* c) {
    if (!c) return vine_invalid_arg("mpc adapt config is NULL");
    *c = VineMpcAdaptConfig{};
    c->abi_version = VINE_MPC_ADAPT_ABI_VERSION;
    c->samples = 256;
    c->window = 8;
    c->every = 8;
    c->min_steps = 4;
    c->temperature = 0.1;
    c->rate = 0.5;
    for (int f = 0; f < VINE_NUM_DOFS; ++f) c->weights[f] = 1.0f;
    return VINE_OK;
}

int vine_mpc_adapt_config_size(void) { return (int)sizeof(VineMpcAdaptConfig); }

int vine_mpc_adapt_anchor(VineHandle* plant, const VineMpcAdaptConfig* cfg, const int64_t* plant_progress,
                          const int64_t* plant_reset, const float* history, float* anchor_state, float* anchor_history,
                          int64_t* anchor_progress, int64_t* anchor_count, int32_t* trace_len, uint8_t* trace_open,
                          uint8_t* episode_ended, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!plant || !plant_progress || !plant_reset || !history || !anchor_state || !anchor_history || !anchor_progress ||
        !anchor_count || !trace_len || !trace_open || !episode_ended)
        return vine_invalid_arg("null argument to vine_mpc_adapt_anchor");
    VineHandleInfo info;
    AdaptParams S;
    rc = prepare_plant(plant, cfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_adapt_anchor_kernel, dim3((S.m + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream,
                       S, (const float*)info.state, info.counters, (const long long*)plant_progress,
                       (const long long*)plant_reset, history, anchor_state, anchor_history, (long long*)anchor_progress,
                       (long long*)anchor_count, trace_len, trace_open, episode_ended);
    return vine_launch_status("vine_mpc_adapt_anchor");
}

int vine_mpc_adapt_trace(VineHandle* plant, const VineMpcAdaptConfig* cfg, const float* plant_actions,
                         const int64_t* plant_reset, const float* plant_rew, const int64_t* anchor_count, float* trace_actions,
                         float* trace_rows, int32_t* trace_len, uint8_t* trace_open, uint8_t* episode_ended, double* returns,
                         void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!plant || !plant_actions || !plant_reset || !plant_rew || !anchor_count || !trace_actions || !trace_rows || !trace_len ||
        !trace_open || !episode_ended)
        return vine_invalid_arg("null argument to vine_mpc_adapt_trace");
    VineHandleInfo info;
    AdaptParams S;
    rc = prepare_plant(plant, cfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_adapt_trace_kernel, dim3((S.m + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream,
                       S, (const float*)info.state, info.counters, plant_actions, (const long long*)plant_reset, plant_rew,
                       (const long long*)anchor_count, trace_actions, trace_rows, trace_len, trace_open, episode_ended, returns);
    return vine_launch_status("vine_mpc_adapt_trace");
}

int vine_mpc_adapt_pin(VineHandle* model, const VineMpcAdaptConfig* cfg, const double* mean, const double* std,
                       const int64_t* passes, const float* anchor_state, const float* anchor_history,
                       const int64_t* anchor_progress, const float* trace_actions, float* actions, float* rew, int64_t* reset,
                       int64_t* progress, double* err, uint8_t* alive, int64_t* window, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!model || !mean || !std || !passes || !anchor_state || !anchor_history || !anchor_progress || !trace_actions ||
        !actions || !rew || !reset || !progress || !err || !alive || !window)
        return vine_invalid_arg("null argument to vine_mpc_adapt_pin");
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(trace_actions) |
         reinterpret_cast<uintptr_t>(anchor_history)) & 7u)
        return vine_invalid_arg("mpc adapt actions, trace_actions and anchor_history must be 8-byte aligned");
    VineHandleInfo info;
    AdaptParams S;
    rc = prepare_model(model, cfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_adapt_pin_kernel, dim3((S.n + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, S,
                       info.state, info.counters, const_cast<float*>(info.env_params), mean, std, (const long long*)passes,
                       anchor_state, anchor_history, (const long long*)anchor_progress, trace_actions, actions, rew,
                       (long long*)reset, (long long*)progress, err, alive, (long long*)window);
    return vine_launch_status("vine_mpc_adapt_pin");
}

int vine_mpc_adapt_scheduled(VineHandle* model, const VineMpcAdaptConfig* cfg, const float* trace_actions,
                             const float* trace_rows, const int32_t* trace_len, const int64_t* window, float* actions,
                             const int64_t* reset, double* err, uint8_t* alive, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!model || !trace_actions || !trace_rows || !trace_len || !window || !actions || !reset || !err || !alive)
        return vine_invalid_arg("null argument to vine_mpc_adapt_scheduled");
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(trace_actions)) & 7u)
        return vine_invalid_arg("mpc adapt actions and trace_actions must be 8-byte aligned");
    VineHandleInfo info;
    AdaptParams S;
    rc = prepare_model(model, cfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_adapt_node_kernel, dim3((S.n + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream, S,
                       (const float*)info.state, info.counters, trace_actions, trace_rows, trace_len, (const long long*)window,
                       actions, (const long long*)reset, err, alive);
    return vine_launch_status("vine_mpc_adapt_scheduled");
}

int vine_mpc_adapt_estimate(VineHandle* model, const VineMpcAdaptConfig* cfg, const double* err, const int32_t* trace_len,
                            const uint8_t* episode_ended, double* mean, double* std, const double* prior_mean,
                            const double* prior_std, int64_t* passes, double* weights, void* stream) {
    int rc = validate(cfg);
    if (rc) return rc;
    if (!model || !err || !trace_len || !episode_ended || !mean || !std || !prior_mean || !prior_std || !passes)
        return vine_invalid_arg("null argument to vine_mpc_adapt_estimate");
    VineHandleInfo info;
    AdaptParams S;
    rc = prepare_model(model, cfg, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_adapt_estimate_kernel, dim3(S.m), dim3(THREADS), 0, (hipStream_t)stream, S,
                       const_cast<float*>(info.env_params), err, trace_len, episode_ended, mean, std, prior_mean, prior_std,
                       (long long*)passes, weights);
    return vine_launch_status("vine_mpc_adapt_estimate");
}

}  // extern "C"
