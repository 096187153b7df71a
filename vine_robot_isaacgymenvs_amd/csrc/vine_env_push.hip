// vine_env_push.hip — per-env random impulses on the chain (ENV_PUSH) for MI355X (gfx950): include/vine_env_push.h states the
// semantics, utils/env_push.py push_replay is the same statement in numpy.
//
// One lane per env, VINE_ENV_PUSH_THREADS envs per workgroup, no LDS, no atomics.  A lane that is not pushed reads its reset
// word, its two values and its Philox draw, and leaves.  A pushed lane issues all its loads together, before anything depends
// on one -- the five joint angles (the mass matrix does not depend on the cart's position), the six velocities and, where an
// inertia table is bound, its 20 composites -- then factors its 6x6 mass matrix in registers (an unrolled Cholesky), solves,
// and stores six velocities.  The launch is latency-bound at rollout sizes (profiles/env_sensor/node_cost.txt), not byte-bound.
//
// CONTRACTION IS OFF FOR THIS WHOLE TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it
// with -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): the draw of vine_named_draw.h must hold the
// host's bits, and the solve is then the float32 statement numpy makes, product by product.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/vine_env_push.h"
#include "vine_named_draw.h"
#include "vine_observer.h"
#include "vine_policy_head.h"

namespace {

constexpr int THREADS = VINE_ENV_PUSH_THREADS;
constexpr int NL = VINE_NUM_LINKS;
constexpr int ND = NL + 1;
constexpr int NC = VINE_PUSH_COMPOSITES;
static_assert(VI_COUNT - VI_MTOT == NC && VI_B0 == VI_MTOT + 1 && VI_GB0 == VI_B0 + NL && VI_ADIAG0 == VI_GB0 + NL &&
                  VI_AOFF1 == VI_ADIAG0 + NL,
              "the composites of a spec are the derived rows of the inertia table, in its order");
static_assert(VINE_PUSH_MAX_POINTS == ND && NL == 5, "a point per generalised coordinate");
// offsets into the 20 composites
constexpr int C_MTOT = 0, C_B = VI_B0 - VI_MTOT, C_ADIAG = VI_ADIAG0 - VI_MTOT, C_AOFF1 = VI_AOFF1 - VI_MTOT;

// M = G G^T row by row, G y = Q, G^T x = y; every sum subtracts its products in ascending k (push_replay: the same order)
__device__ __forceinline__ void cholesky_solve(float (&A)[ND][ND], float (&x)[ND]) {
#pragma unroll
    for (int i = 0; i < ND; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float sum = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) sum = sum - A[i][k] * A[j][k];
            A[i][j] = i == j ? sqrtf(sum) : sum / A[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        float sum = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) sum = sum - A[i][k] * x[k];
        x[i] = sum / A[i][i];
    }
#pragma unroll
    for (int i = ND - 1; i >= 0; --i) {
        float sum = x[i];
#pragma unroll
        for (int k = i + 1; k < ND; ++k) sum = sum - A[k][i] * x[k];
        x[i] = sum / A[i][i];
    }
}

template <bool BOUND>
__global__ __launch_bounds__(THREADS) void vine_env_push_kernel(const VineEnvPushSpec S, const int n, const unsigned env_off,
                                                                const unsigned long long* __restrict__ counters, const int glog,
                                                                float* __restrict__ state, const float* __restrict__ inertia,
                                                                const float L, const float s0, const float c0,
                                                                const long long* __restrict__ reset, float* __restrict__ table,
                                                                int* __restrict__ episode_index, int* __restrict__ push_count) {
    const unsigned long long c = vine_steps_completed(counters, glog);
    if (c == 0ull) return;
    const int e = blockIdx.x * THREADS + (int)threadIdx.x;
    if (e >= n) return;
    const unsigned long long s = c - 1ull;
    const unsigned g = env_off + (unsigned)e;

    const bool flagged = reset[e] != 0;
    const float p = table[(size_t)VPU_RATE * n + e];
    const float imp = table[(size_t)VPU_IMPULSE * n + e];
    unsigned w[4];
    philox4x32_10(g, (unsigned)s, VINE_PUSH_RNG | ((unsigned)(s >> 32) << 8), 0u, (unsigned)S.seed, (unsigned)(S.seed >> 32), w);

    if (!flagged && u01(w[3]) < p) {
        push_count[e] = push_count[e] + 1;
        if (imp != 0.0f) {
            // every load first
            float q[NL], qd[ND], cm[NC];
#pragma unroll
            for (int i = 0; i < NL; ++i) q[i] = state[(size_t)(VF_Q0 + 1 + i) * n + e];
#pragma unroll
            for (int i = 0; i < ND; ++i) qd[i] = state[(size_t)(VF_QD0 + i) * n + e];
#pragma unroll
            for (int r = 0; r < NC; ++r) cm[r] = BOUND ? inertia[(size_t)(VI_MTOT + r) * n + e] : S.composites[r];

            const float ay = (float)(w[0] >> 8) * (1.0f / 8388608.0f) - 1.0f;
            const float az = (float)(w[1] >> 8) * (1.0f / 8388608.0f) - 1.0f;
            const float Py = imp * ay, Pz = imp * az;
            // (the index is below num_points <= 6 by construction; the clamp keeps a spec altered behind the check inside the array)
            const unsigned pick = min((unsigned)(((unsigned long long)(w[2] >> 8) * (unsigned)S.num_points) >> 24),
                                      (unsigned)(VINE_PUSH_MAX_POINTS - 1));
            int m = 0;
#pragma unroll
            for (int i = 0; i < VINE_PUSH_MAX_POINTS; ++i) m = pick == (unsigned)i ? S.points[i] : m;

            float sn[NL], cs[NL], A[ND][ND], x[ND];
            float th = 0.0f;
            A[0][0] = cm[C_MTOT];
            x[0] = Py;
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                th = th + q[i];
                sincosf(th, &sn[i], &cs[i]);
                const float sp = s0 * cs[i] + c0 * sn[i];
                const float cp = c0 * cs[i] - s0 * sn[i];
                A[i + 1][0] = -cm[C_B + i] * cp;
                x[i + 1] = i < m ? -L * (cp * Py + sp * Pz) : 0.0f;
#pragma unroll
                for (int j = 0; j <= i; ++j)      // a_ij, j < i, is AOFF_i
                    A[i + 1][j + 1] = (j == i ? cm[C_ADIAG + i] : cm[C_AOFF1 + i - 1]) * (cs[i] * cs[j] + sn[i] * sn[j]);
            }
            cholesky_solve(A, x);
            state[(size_t)(VF_QD0 + 0) * n + e] = qd[0] + x[0];
            state[(size_t)(VF_QD0 + 1) * n + e] = qd[1] + x[1];
#pragma unroll
            for (int k = 1; k < NL; ++k) state[(size_t)(VF_QD0 + 1 + k) * n + e] = qd[k + 1] + (x[k + 1] - x[k]);
        }
    }

    if (S.per_episode && flagged) VINE_NAMED_REDRAW_ROWS(VPU_NAMES, S.name, 0u, S.values, S.seed, env_off, e, n, table, episode_index);
}

const char* const kNames[VPU_NAMES] = {"PUSH_RATE", "PUSH_IMPULSE"};

int bad_name(int s, const char* why) { return named_refusal("env push spec", kNames[s], why); }

// is v a value the name may take?  (what the kernel would write into the table: the float32 of it)
const char* bad_value(int s, double v) {
    if (s == VPU_RATE) return (!(v >= 0.0) || !(v <= 1.0)) ? "must lie in [0, 1]" : nullptr;
    return !(v >= 0.0) ? "must not be negative" : nullptr;
}

}  // namespace

extern "C" {

int vine_env_push_spec_size(void) { return (int)sizeof(VineEnvPushSpec); }

int vine_env_push_spec(const VineConfig* cfg, const VineEnvRedrawName names[VPU_NAMES], const double* host_values,
                       const double* device_values, int num_values, const int32_t* points, int num_points, int per_episode,
                       VineEnvPushSpec* out) {
    if (!cfg || !names || !points || !out) return vine_invalid_arg("null argument to vine_env_push_spec");
    if (num_values < 0 || (num_values > 0 && (!host_values || !device_values)))
        return vine_invalid_arg("null argument to vine_env_push_spec: the value lists need a host and a device array");
    VineEnvPushSpec S;
    memset(&S, 0, sizeof S);
    S.abi_version = VINE_ENV_PUSH_ABI_VERSION;
    S.num_values = num_values;
    S.seed = cfg->seed;
    S.values = device_values;
    S.per_episode = per_episode ? 1 : 0;
    if (num_points < 1) return vine_invalid_arg("env push spec: POINTS: the list is empty");
    if (num_points > VINE_PUSH_MAX_POINTS) return vine_invalid_arg("env push spec: POINTS: more than VINE_PUSH_MAX_POINTS (6) entries");
    S.num_points = num_points;
    unsigned seen = 0u;
    for (int i = 0; i < num_points; ++i) {
        if (points[i] < 0 || points[i] >= VINE_PUSH_MAX_POINTS) return vine_invalid_arg("env push spec: POINTS: a point index lies outside 0 .. 5");
        if (seen & (1u << points[i])) return vine_invalid_arg("env push spec: POINTS: a point is listed twice");
        seen |= 1u << points[i];
        S.points[i] = points[i];
    }
    float row[VI_COUNT];
    const int rc = vine_env_inertia_row(cfg, row);
    if (rc) return rc;
    for (int r = 0; r < NC; ++r) S.composites[r] = row[VI_MTOT + r];
    for (int s = 0; s < VPU_NAMES; ++s) {
        const VineEnvRedrawName& nm = names[s];
        S.name[s] = nm;
        const NamedCheck c = named_check(nm, host_values, num_values, false, [s](double v) { return bad_value(s, v); });
        if (c.why) return bad_name(s, c.why);
        const bool zero = c.hi == 0.0;           // (no value is negative: the largest is zero where all are)
        if (zero && !S.per_episode) return bad_name(s, "constant zero: nothing to do");
    }
    S.checked = 1u;
    *out = S;
    return VINE_OK;
}

int vine_env_push_scheduled(VineHandle* h, const VineEnvPushSpec* spec, const int64_t* reset, float* push_table,
                            int32_t* episode_index, int32_t* push_count, void* stream) {
    if (!h || !spec || !reset || !push_table || !episode_index || !push_count)
        return vine_invalid_arg("null argument to vine_env_push_scheduled");
    if (spec->abi_version != VINE_ENV_PUSH_ABI_VERSION) return vine_invalid_arg("VineEnvPushSpec.abi_version mismatch");
    if (spec->checked != 1u) return vine_invalid_arg("VineEnvPushSpec was not filled by vine_env_push_spec");
    if (spec->num_values > 0 && !spec->values) return vine_invalid_arg("VineEnvPushSpec.values is NULL");
    if (spec->num_points < 1 || spec->num_points > VINE_PUSH_MAX_POINTS) return vine_invalid_arg("VineEnvPushSpec.num_points lies outside 1 .. 6");
    VineHandleInfo info;
    int rc = vine_handle_info(h, &info);
    if (rc) return rc;
    const float *bound_params = nullptr, *bound_inertia = nullptr;
    unsigned env_off = 0;
    rc = vine_env_tables_of(h, &bound_params, &bound_inertia, &env_off);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    const hipStream_t st = (hipStream_t)stream;
    const int blocks = (info.n + THREADS - 1) / THREADS;
    if (bound_inertia)
        hipLaunchKernelGGL(vine_env_push_kernel<true>, dim3(blocks), dim3(THREADS), 0, st, *spec, info.n, env_off, info.counters,
                           info.glog, info.state, bound_inertia, info.L, info.s0, info.c0, (const long long*)reset, push_table,
                           episode_index, push_count);
    else
        hipLaunchKernelGGL(vine_env_push_kernel<false>, dim3(blocks), dim3(THREADS), 0, st, *spec, info.n, env_off, info.counters,
                           info.glog, info.state, bound_inertia, info.L, info.s0, info.c0, (const long long*)reset, push_table,
                           episode_index, push_count);
    return vine_launch_status("vine_env_push");
}

}  // extern "C"
