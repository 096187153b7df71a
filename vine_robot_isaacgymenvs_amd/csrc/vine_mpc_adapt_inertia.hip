// vine_mpc_adapt_inertia.hip — the mass dimensions of the predictive controller's online model adaptation for MI355X (gfx950):
// include/vine_mpc_adapt_inertia.h states the semantics, utils/mpc_adapt_inertia.py (mass_candidates, inertia_rows,
// mass_estimate) is the same statement in numpy.
//
// vine_mpc_adapt_inertia_pin_kernel is one lane per model env, 256 lanes per workgroup, over the SoA inertia table
// (table[row * n + e]: a wave writes 64 contiguous floats per row); no LDS.  vine_mpc_adapt_inertia_estimate_kernel is one
// workgroup per plant with the reduction of vine_mpc_adapt_estimate_kernel, whose weights and update it restates for the mass
// dimensions (vine_mpc_adapt.hip keeps them in its anonymous namespace and is not edited; a GPU test holds a degenerate mass
// belief beside the plain adaptive controller bit for bit).  A candidate's value is recomputed wherever it is needed and
// never stored.  No atomics anywhere; plain C++ stores only.
//
// CONTRACTION IS OFF FOR THIS TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it with
// -ffp-contract=fast-honor-pragmas): `mean + z * std`, `(1 - rate) * mean + rate * m` and the composites of
// vine_inertia_composites.h (`m l + L distal`) must stay the multiplies and adds that numpy and the host pass form, or a
// column would differ from vine_env_inertia_derive's in the last bit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/vine_env_inertia.h"
#include "../../include/vine_mpc_adapt_inertia.h"
#include "vine_inertia_composites.h"
#include "vine_observer.h"
#include "vine_policy_head.h"
#include "vine_task_shared.h"
#include "vine_mpc_shared.h"

namespace {

constexpr int THREADS = VINE_MPC_THREADS;
constexpr int WAVES = THREADS / 64;
constexpr int NAMES = VINE_MPC_ADAPT_INERTIA_MAX_DIMS;
constexpr int NL = VINE_NUM_LINKS;
static_assert(THREADS == 256, "four waves per workgroup");
static_assert(NAMES == 3 && VINE_MPC_ADAPT_INERTIA_CART == 0 && VINE_MPC_ADAPT_INERTIA_LINK == 1 &&
                  VINE_MPC_ADAPT_INERTIA_TIP == 2, "one slot per name");
static_assert(VI_PRIMARY_COUNT == 1 + 2 * NL && VI_COUNT == VI_PRIMARY_COUNT + 1 + 3 * NL + (NL - 1), "the table's rows");

// Everything per NAME (cart, link, tip), so that the kernels index it with constants; slot[a] is the name's dimension in the
// belief (the column of mass_mean), or -1 where the name is absent.
struct MassParams {
    int n, m, K, Dm, min_steps, forget;
    unsigned seed_lo, seed_hi;
    double k0, temperature, rate;
    int slot[NAMES];
    double lo[NAMES], hi[NAMES], floor[NAMES];
    float base[VI_PRIMARY_COUNT];
    float L, l, g;
};

// theta of sample e (candidate j of its plant) in mass dimension i during pass `pass`: the header's CANDIDATES.
__device__ __forceinline__ double mass_theta(const MassParams& S, unsigned e, bool first, long long pass, int i, double lo,
                                             double hi, double mean, double std) {
    float z = 0.0f;
    if (!first) {
        const unsigned long long t = (unsigned long long)pass;
        unsigned w[4];
        philox4x32_10(e, (unsigned)t, VINE_MPC_ADAPT_RNG | ((unsigned)(t >> 32) << 8), (unsigned)(VINE_MPC_ADAPT_MAX_DIMS + i),
                      S.seed_lo, S.seed_hi, w);
        z = (float)((double)mpc_deviate_int(w) * S.k0);
    }
    const double zs = (double)z * std;
    const double x = mean + zs;
    return fmin(fmax(x, lo), hi);
}

// The value of an absent name: the base cart mass, or the factor 1.
__device__ __forceinline__ double mass_absent(const MassParams& S, int a) {
    return a == VINE_MPC_ADAPT_INERTIA_CART ? (double)S.base[VI_CART_MASS] : 1.0;
}

// The column of the per-name values tn: the header's THE COLUMN (the inertia half of csrc/vine_env_redraw_draw.h's statement).
__device__ __forceinline__ void mass_column(const MassParams& S, const double tn[NAMES], float col[VI_COUNT]) {
    col[VI_CART_MASS] = (float)tn[VINE_MPC_ADAPT_INERTIA_CART];
    const double link = tn[VINE_MPC_ADAPT_INERTIA_LINK];
    const double both = link * tn[VINE_MPC_ADAPT_INERTIA_TIP];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const double f = i == NL - 1 ? both : link;
        col[VI_LINK_MASS0 + i] = (float)((double)S.base[VI_LINK_MASS0 + i] * f);
        col[VI_LINK_INERTIA0 + i] = (float)((double)S.base[VI_LINK_INERTIA0 + i] * f);
    }
    InertiaComposites ic;
    inertia_composites(col[VI_CART_MASS], col + VI_LINK_MASS0, col + VI_LINK_INERTIA0, S.L, S.l, S.g, ic);
    col[VI_MTOT] = (float)ic.mtot;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        col[VI_B0 + i] = (float)ic.b[i];
        col[VI_GB0 + i] = (float)ic.gb[i];
        col[VI_ADIAG0 + i] = (float)ic.adiag[i];
        if (i > 0) col[VI_AOFF1 + i - 1] = (float)ic.aoff[i];
    }
}

__global__ __launch_bounds__(THREADS) void vine_mpc_adapt_inertia_pin_kernel(
    const MassParams S, float* __restrict__ table, const double* __restrict__ mean, const double* __restrict__ std,
    const long long* __restrict__ passes) {
    const int n = S.n, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int p = e / S.K, j = e - p * S.K;
    const long long pass = passes[p];
    double tn[NAMES];
#pragma unroll
    for (int a = 0; a < NAMES; ++a) {
        const int i = S.slot[a];
        tn[a] = i >= 0 ? mass_theta(S, (unsigned)e, j == 0, pass, i, S.lo[a], S.hi[a], mean[(size_t)p * S.Dm + i],
                                    std[(size_t)p * S.Dm + i])
                       : mass_absent(S, a);
    }
    float col[VI_COUNT];
    mass_column(S, tn, col);
#pragma unroll
    for (int r = 0; r < VI_COUNT; ++r) table[(size_t)r * n + e] = col[r];
}

// The workgroup reductions of vine_mpc_adapt.hip, restated: the wave's butterfly, the four wave values through LDS, combined
// in wave order.  Every lane returns the same bits; the second barrier lets the next call reuse `part`.
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

__global__ __launch_bounds__(THREADS) void vine_mpc_adapt_inertia_estimate_kernel(
    const MassParams S, float* __restrict__ table, const double* __restrict__ err, const int* __restrict__ trace_len,
    const unsigned char* __restrict__ episode_ended, double* __restrict__ mean, double* __restrict__ std,
    const double* __restrict__ prior_mean, const double* __restrict__ prior_std, const long long* __restrict__ passes,
    double* __restrict__ weights) {
    __shared__ double old_mean[NAMES], old_std[NAMES];   // by NAME: mean[p], std[p], read before anything is written
    __shared__ double new_mean[NAMES];                   // by name too (an absent name's holds its fixed value)
    __shared__ double part[WAVES];
    const int p = blockIdx.x, t = (int)threadIdx.x, K = S.K, Dm = S.Dm, n = S.n;
    if (t < NAMES) {
        const int i = S.slot[t];
        old_mean[t] = i >= 0 ? mean[(size_t)p * Dm + i] : mass_absent(S, t);
        old_std[t] = i >= 0 ? std[(size_t)p * Dm + i] : 0.0;
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
#pragma unroll
        for (int a = 0; a < NAMES; ++a) {
            const int i = S.slot[a];                     // uniform over the workgroup
            if (i < 0) {
                if (t == 0) new_mean[a] = old_mean[a];
                continue;
            }
            const double m0 = old_mean[a], s0 = old_std[a];
            double acc = 0.0;
            for (int j = t; j < K; j += THREADS) {
                const double ej = ep[j];
                const double w = ej < INFINITY ? (tau > 0.0 ? exp(-(ej - beta) / tau) : 1.0) : 0.0;
                acc += w * mass_theta(S, (unsigned)(p * K + j), j == 0, pass, i, S.lo[a], S.hi[a], m0, s0);
            }
            const double md = block_sum(acc, part) / sw;
            double b = 0.0;
            for (int j = t; j < K; j += THREADS) {
                const double ej = ep[j];
                const double w = ej < INFINITY ? (tau > 0.0 ? exp(-(ej - beta) / tau) : 1.0) : 0.0;
                const double dv = mass_theta(S, (unsigned)(p * K + j), j == 0, pass, i, S.lo[a], S.hi[a], m0, s0) - md;
                b += w * (dv * dv);
            }
            const double vd = block_sum(b, part) / sw;
            if (t == 0) {
                const double keep = 1.0 - S.rate;
                const double nm = keep * m0 + S.rate * md;
                const double ns = fmax(keep * s0 + S.rate * sqrt(vd), S.floor[a]);
                new_mean[a] = nm;
                mean[(size_t)p * Dm + i] = nm;
                std[(size_t)p * Dm + i] = ns;
            }
        }
    } else {
        if (weights)
            for (int j = t; j < K; j += THREADS) weights[(size_t)p * K + j] = 0.0;
        if (t < NAMES) {
            const int i = S.slot[t];
            const double nm = (forget && i >= 0) ? prior_mean[(size_t)p * Dm + i] : old_mean[t];
            new_mean[t] = nm;
            if (forget && i >= 0) {
                mean[(size_t)p * Dm + i] = nm;
                std[(size_t)p * Dm + i] = prior_std[(size_t)p * Dm + i];
            }
        }
    }
    __syncthreads();
    // the planning value: the candidates' statement at z = 0 on the new mean, into the columns of all K samples (every lane
    // forms the same column)
    double tn[NAMES];
#pragma unroll
    for (int a = 0; a < NAMES; ++a) tn[a] = S.slot[a] >= 0 ? fmin(fmax(new_mean[a], S.lo[a]), S.hi[a]) : mass_absent(S, a);
    float col[VI_COUNT];
    mass_column(S, tn, col);
    for (int j = t; j < K; j += THREADS) {
        const size_t e = (size_t)p * K + j;
#pragma unroll
        for (int r = 0; r < VI_COUNT; ++r) table[(size_t)r * n + e] = col[r];
    }
}

// What vine_mpc_adapt.hip's own check refuses of the base configuration, in its words (restated: that function is in its
// anonymous namespace).
int validate_base(const VineMpcAdaptConfig* c) {
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

int bad_dim(int d, const char* why) {
    char msg[200];
    snprintf(msg, sizeof msg, "mpc adapt inertia dims[%d]: %s", d, why);
    return vine_invalid_arg(msg);
}

int validate(const VineMpcAdaptConfig* c, const VineMpcAdaptInertiaConfig* ic) {
    if (const int rc = validate_base(c)) return rc;
    if (!ic) return vine_invalid_arg("mpc adapt inertia config is NULL");
    if (ic->abi_version != VINE_MPC_ADAPT_INERTIA_ABI_VERSION)
        return vine_invalid_arg("VineMpcAdaptInertiaConfig.abi_version mismatch");
    if (ic->num_mass_dims < 1 || ic->num_mass_dims > NAMES)
        return vine_invalid_arg("mpc adapt inertia needs 1 <= num_mass_dims <= VINE_MPC_ADAPT_INERTIA_MAX_DIMS (3)");
    unsigned taken = 0;
    for (int d = 0; d < ic->num_mass_dims; ++d) {
        const VineMpcAdaptInertiaDim& m = ic->dims[d];
        if (m.name < 0 || m.name >= NAMES) return bad_dim(d, "unknown name (0 cart, 1 link, 2 tip)");
        if (taken & (1u << m.name)) return bad_dim(d, "repeats the name of an earlier dimension");
        taken |= 1u << m.name;
        if (!std::isfinite(m.lo) || !std::isfinite(m.hi) || m.lo > m.hi) return bad_dim(d, "needs finite lo <= hi");
        if (!(m.lo > 0.0)) return bad_dim(d, "needs lo > 0 (a candidate mass must be positive)");
        if (!std::isfinite(m.std_floor) || m.std_floor < 0.0) return bad_dim(d, "std_floor must be finite and not negative");
    }
    for (int r = 0; r < VI_PRIMARY_COUNT; ++r) {
        const float v = ic->base_inertia[r];
        if (!std::isfinite(v) || (r < VI_LINK_INERTIA0 ? !(v > 0.0f) : v < 0.0f))
            return vine_invalid_arg("mpc adapt inertia base_inertia needs finite masses > 0 and inertias >= 0");
    }
    if (!std::isfinite(ic->link_length) || !(ic->link_length > 0.0f))
        return vine_invalid_arg("mpc adapt inertia link_length must be finite and positive");
    if (!std::isfinite(ic->link_com) || !(ic->link_com > 0.0f))
        return vine_invalid_arg("mpc adapt inertia link_com must be finite and positive");
    if (!std::isfinite(ic->gravity)) return vine_invalid_arg("mpc adapt inertia gravity must be finite");
    return VINE_OK;
}

// The model handle's part: refuses a handle that does not hold num_plants * samples envs, has no inertia table bound or has
// another one bound than the memory passed.
int prepare(VineHandle* model, const VineMpcAdaptConfig* cfg, const VineMpcAdaptInertiaConfig* ic, const float* inertia_table,
            VineHandleInfo& info, MassParams& S) {
    int rc = vine_handle_info(model, &info);
    if (rc) return rc;
    if ((long long)info.n != (long long)cfg->num_plants * cfg->samples) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc adapt inertia: the model handle has %d envs, not num_plants * samples = %d * %d", info.n,
                 cfg->num_plants, cfg->samples);
        return vine_invalid_arg(msg);
    }
    const float *bound_params = nullptr, *bound_inertia = nullptr;
    unsigned env_off = 0;
    rc = vine_env_tables_of(model, &bound_params, &bound_inertia, &env_off);
    if (rc) return rc;
    if (!bound_inertia)
        return unsupported("mpc adapt inertia: the model handle has no inertia table bound (vine_bind_env_inertia): the table is "
                           "what is adapted");
    if (bound_inertia != inertia_table)
        return unsupported("mpc adapt inertia: inertia_table is not the table bound to the model handle");
    S.m = cfg->num_plants; S.K = cfg->samples; S.n = S.m * S.K; S.Dm = ic->num_mass_dims;
    S.min_steps = cfg->min_steps; S.forget = cfg->forget_on_reset;
    S.seed_lo = (unsigned)cfg->seed; S.seed_hi = (unsigned)(cfg->seed >> 32);
    S.k0 = noise_scale(); S.temperature = cfg->temperature; S.rate = cfg->rate;
    for (int a = 0; a < NAMES; ++a) {
        S.slot[a] = -1;
        S.lo[a] = S.hi[a] = S.floor[a] = 0.0;
    }
    for (int d = 0; d < ic->num_mass_dims; ++d) {
        const VineMpcAdaptInertiaDim& m = ic->dims[d];
        S.slot[m.name] = d;
        S.lo[m.name] = m.lo; S.hi[m.name] = m.hi; S.floor[m.name] = m.std_floor;
    }
    for (int r = 0; r < VI_PRIMARY_COUNT; ++r) S.base[r] = ic->base_inertia[r];
    S.L = ic->link_length; S.l = ic->link_com; S.g = ic->gravity;
    return VINE_OK;
}

}  // namespace

extern "C" {

int vine_mpc_adapt_inertia_config_default(VineMpcAdaptInertiaConfig* c) {
    if (!c) return vine_invalid_arg("mpc adapt inertia config is NULL");
    *c = VineMpcAdaptInertiaConfig{};
    c->abi_version = VINE_MPC_ADAPT_INERTIA_ABI_VERSION;
    return VINE_OK;
}

int vine_mpc_adapt_inertia_config_size(void) { return (int)sizeof(VineMpcAdaptInertiaConfig); }

int vine_mpc_adapt_inertia_pin(VineHandle* model, const VineMpcAdaptConfig* cfg, const VineMpcAdaptInertiaConfig* icfg,
                               float* inertia_table, const double* mass_mean, const double* mass_std, const int64_t* passes,
                               void* stream) {
    int rc = validate(cfg, icfg);
    if (rc) return rc;
    if (!model || !inertia_table || !mass_mean || !mass_std || !passes)
        return vine_invalid_arg("null argument to vine_mpc_adapt_inertia_pin");
    VineHandleInfo info;
    MassParams S;
    rc = prepare(model, cfg, icfg, inertia_table, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_adapt_inertia_pin_kernel, dim3((S.n + THREADS - 1) / THREADS), dim3(THREADS), 0,
                       (hipStream_t)stream, S, inertia_table, mass_mean, mass_std, (const long long*)passes);
    return vine_launch_status("vine_mpc_adapt_inertia_pin");
}

int vine_mpc_adapt_inertia_estimate(VineHandle* model, const VineMpcAdaptConfig* cfg, const VineMpcAdaptInertiaConfig* icfg,
                                    float* inertia_table, const double* err, const int32_t* trace_len,
                                    const uint8_t* episode_ended, double* mass_mean, double* mass_std,
                                    const double* mass_prior_mean, const double* mass_prior_std, const int64_t* passes,
                                    double* weights, void* stream) {
    int rc = validate(cfg, icfg);
    if (rc) return rc;
    if (!model || !inertia_table || !err || !trace_len || !episode_ended || !mass_mean || !mass_std || !mass_prior_mean ||
        !mass_prior_std || !passes)
        return vine_invalid_arg("null argument to vine_mpc_adapt_inertia_estimate");
    VineHandleInfo info;
    MassParams S;
    rc = prepare(model, cfg, icfg, inertia_table, info, S);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_adapt_inertia_estimate_kernel, dim3(S.m), dim3(THREADS), 0, (hipStream_t)stream, S,
                       inertia_table, err, trace_len, episode_ended, mass_mean, mass_std, mass_prior_mean, mass_prior_std,
                       (const long long*)passes, weights);
    return vine_launch_status("vine_mpc_adapt_inertia_estimate");
}

}  // extern "C"
