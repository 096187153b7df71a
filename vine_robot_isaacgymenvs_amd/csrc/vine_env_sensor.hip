// vine_env_sensor.hip — per-env observation delay, dropped frames and noise (ENV_SENSOR) for MI355X (gfx950):
// include/vine_env_sensor.h states the semantics, utils/env_sensor.py sensor_replay is the same statement in numpy.
//
// One lane per env, VINE_ENV_SENSOR_THREADS envs per workgroup, no LDS, no atomics.  A lane reads its env's three values, then
// moves its row in vectors of V floats (16 bytes where the row allows it): per vector one load of the observation, one store
// into the ring, where a delay or a held frame asks for it one load from the ring, and one store of the delivered frame where
// it differs from what the step wrote; the loads of a row are all issued first.  Nothing else is read but the env's progress
// word, reset word and fresh byte.
//
// CONTRACTION IS OFF FOR THIS WHOLE TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it
// with -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): `obs + z * c` must stay a multiply and an add,
// each rounded, as numpy forms it, and the draw of vine_named_draw.h likewise.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/vine_env_sensor.h"
#include "vine_named_draw.h"
#include "vine_observer.h"
#include "vine_policy_head.h"

namespace {

constexpr int THREADS = VINE_ENV_SENSOR_THREADS;
constexpr int SLOTS = VINE_SENSOR_SLOTS;
static_assert(VINE_SENSOR_MAX_DELAY == VINE_MAX_DELAY, "the sensing path delays by what the command path can");
static_assert(VINE_MAX_OBS <= 32, "the column mask has 32 bits");

template <int V> struct RowVec;
template <> struct RowVec<4> { using type = float4; };
template <> struct RowVec<2> { using type = float2; };
__device__ __forceinline__ void unpack(const float4& v, float (&o)[4]) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
__device__ __forceinline__ void unpack(const float2& v, float (&o)[2]) { o[0] = v.x; o[1] = v.y; }
__device__ __forceinline__ float4 pack(const float (&o)[4]) { return make_float4(o[0], o[1], o[2], o[3]); }
__device__ __forceinline__ float2 pack(const float (&o)[2]) { return make_float2(o[0], o[1]); }

// 1 / sqrt(32 * (65536^2 - 1) / 12): the deviate's scale, in float64 (host and device form it by the same statement)
__host__ __device__ inline double sensor_noise_scale() { return 1.0 / sqrt(32.0 * (65536.0 * 65536.0 - 1.0) / 12.0); }

constexpr unsigned INTEGER_NAMES = 1u << VSN_DELAY;      // the names whose range is over the integers

template <int NOBS>
__global__ __launch_bounds__(THREADS) void vine_env_sensor_kernel(const VineEnvSensorSpec S, const int n, const unsigned env_off,
                                                                  const unsigned long long* __restrict__ counters, const int glog,
                                                                  float* obs, const long long* __restrict__ reset,
                                                                  const long long* __restrict__ progress, float* __restrict__ table,
                                                                  float* ring, unsigned char* __restrict__ fresh,
                                                                  int* __restrict__ episode_index) {
    constexpr int V = NOBS % 4 == 0 ? 4 : 2;
    using Vec = typename RowVec<V>::type;
    const unsigned long long c = vine_steps_completed(counters, glog);
    if (c == 0ull) return;
    const int e = blockIdx.x * THREADS + (int)threadIdx.x;
    if (e >= n) return;
    const unsigned long long s = c - 1ull;
    const unsigned g = env_off + (unsigned)e;

    // (clamped: the table is the caller's memory, and d indexes the ring)
    const int d = min(max((int)table[(size_t)VSN_DELAY * n + e], 0), VINE_SENSOR_MAX_DELAY);
    const float p = table[(size_t)VSN_HOLD * n + e];
    const float sd = table[(size_t)VSN_NOISE_STD * n + e];
    const bool is_fresh = fresh[e] != 0;
    const bool first = progress[e] == 0 || is_fresh;
    const unsigned seed_lo = (unsigned)S.seed, seed_hi = (unsigned)(S.seed >> 32);
    const unsigned hi_word = (unsigned)(s >> 32) << 8;
    const bool noisy = sd != 0.0f;
    const float cs = noisy ? (float)((double)sd * sensor_noise_scale()) : 0.0f;

    bool held = false;
    if (!first) {
        unsigned w[4];
        philox4x32_10(g, (unsigned)s, VINE_SENSOR_RNG_HOLD | hi_word, 0u, seed_lo, seed_hi, w);
        held = u01(w[0]) < p;
    }
    const int cur = (int)(s % (unsigned long long)SLOTS);
    const int prev = (cur + SLOTS - 1) % SLOTS;
    const int del = (cur + SLOTS - d) % SLOTS;
    const size_t slot_vecs = (size_t)n * (NOBS / V);
    const size_t row = (size_t)e * NOBS;
    const bool same = !noisy && (first || (!held && d == 0));       // the delivered frame is what the step wrote

    // every load of the row is issued before anything depends on one: at 16384 envs a SIMD holds one wave, and a lane that
    // waited for each vector in turn would pay the memory latency NV times over
    constexpr int NV = NOBS / V;
    Vec* const orow = reinterpret_cast<Vec*>(obs + row);
    Vec* const rrow = reinterpret_cast<Vec*>(ring + row);           // slot k: rrow + k * slot_vecs
    Vec ov[NV], pv[NV], dv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) ov[i] = orow[i];
    if (held) {
#pragma unroll
        for (int i = 0; i < NV; ++i) pv[i] = rrow[prev * slot_vecs + i];
    }
    if (!first && d != 0) {                                         // (del != cur: the slot is not written by this launch)
#pragma unroll
        for (int i = 0; i < NV; ++i) dv[i] = rrow[del * slot_vecs + i];
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float o[V], f[V];
        unpack(ov[i], o);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int col = i * V + j;
            f[j] = o[j];
            if (noisy && ((S.column_mask >> col) & 1u)) {
                unsigned w[4];
                philox4x32_10(g, (unsigned)s, VINE_SENSOR_RNG_NOISE | hi_word, (unsigned)col, seed_lo, seed_hi, w);
                const int sum = (int)((w[0] & 0xffffu) + (w[0] >> 16) + (w[1] & 0xffffu) + (w[1] >> 16) + (w[2] & 0xffffu) +
                                      (w[2] >> 16) + (w[3] & 0xffffu) + (w[3] >> 16));
                const float z = (float)(2 * sum - 524280);
                const float zc = z * cs;
                const float x = o[j] + zc;
                f[j] = fminf(fmaxf(x, -S.clip_observations), S.clip_observations);
            }
        }
        const Vec frame = pack(f);
        Vec delivered = frame;
        if (first) {
            Vec* q = rrow + i;
#pragma unroll 1
            for (int k = 0; k < SLOTS; ++k, q += slot_vecs) *q = frame;
        } else {
            Vec pushed = frame;
            if (held) pushed = pv[i];
            rrow[cur * slot_vecs + i] = pushed;
            delivered = pushed;
            if (d != 0) delivered = dv[i];
        }
        if (!same) {
            float out[V];
            unpack(delivered, out);
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (!((S.column_mask >> (i * V + j)) & 1u)) out[j] = o[j];
            orow[i] = pack(out);
        }
    }
    if (is_fresh) fresh[e] = 0;

    if (S.per_episode && reset[e] != 0) VINE_NAMED_REDRAW_ROWS(VSN_NAMES, S.name, INTEGER_NAMES, S.values, S.seed, env_off, e, n, table, episode_index);
}

const char* const kNames[VSN_NAMES] = {"SENSOR_DELAY", "SENSOR_HOLD", "SENSOR_NOISE_STD"};

int bad_name(int s, const char* why) { return named_refusal("env sensor spec", kNames[s], why); }

// is v a value the name may take?  (what the kernel would write into the table: the float32 of it)
const char* bad_value(int s, double v) {
    if (s == VSN_DELAY)
        return (v != std::floor(v) || v < 0.0 || v > (double)VINE_SENSOR_MAX_DELAY) ? "must be an integer in 0 .. VINE_SENSOR_MAX_DELAY (8)" : nullptr;
    if (s == VSN_HOLD) return (!(v >= 0.0) || !((float)v < 1.0f)) ? "must lie in [0, 1)" : nullptr;
    return !(v >= 0.0) ? "must not be negative" : nullptr;
}

template <int NOBS>
void launch(const VineEnvSensorSpec& S, const VineHandleInfo& info, unsigned env_off, float* obs, const int64_t* reset,
            const int64_t* progress, float* table, float* ring, uint8_t* fresh, int32_t* episode_index, hipStream_t stream) {
    const int blocks = (info.n + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(vine_env_sensor_kernel<NOBS>, dim3(blocks), dim3(THREADS), 0, stream, S, info.n, env_off, info.counters,
                       info.glog, obs, (const long long*)reset, (const long long*)progress, table, ring, fresh, episode_index);
}

}  // namespace

extern "C" {

int vine_env_sensor_spec_size(void) { return (int)sizeof(VineEnvSensorSpec); }

int vine_env_sensor_spec(const VineConfig* cfg, const VineEnvRedrawName names[VSN_NAMES], const double* host_values,
                         const double* device_values, int num_values, uint32_t column_mask, int per_episode,
                         VineEnvSensorSpec* out) {
    if (!cfg || !names || !out) return vine_invalid_arg("null argument to vine_env_sensor_spec");
    if (num_values < 0 || (num_values > 0 && (!host_values || !device_values)))
        return vine_invalid_arg("null argument to vine_env_sensor_spec: the value lists need a host and a device array");
    VineEnvSensorSpec S;
    memset(&S, 0, sizeof S);
    S.abi_version = VINE_ENV_SENSOR_ABI_VERSION;
    S.num_values = num_values;
    S.seed = cfg->seed;
    S.values = device_values;
    S.num_obs = vine_num_obs(cfg);
    if (S.num_obs != 14 && S.num_obs != 18 && S.num_obs != 26 && S.num_obs != 28)
        return vine_invalid_arg("env sensor spec: the configuration's observation type has no known column count");
    S.column_mask = column_mask;
    S.clip_observations = cfg->clip_observations;
    S.per_episode = per_episode ? 1 : 0;
    if (column_mask == 0u) return vine_invalid_arg("env sensor spec: COLUMNS: the mask is empty");
    if (S.num_obs < 32 && (column_mask >> S.num_obs) != 0u)
        return vine_invalid_arg("env sensor spec: COLUMNS: a column index lies outside [0, num_obs)");
    if (!(S.clip_observations > 0.0f)) return vine_invalid_arg("env sensor spec: clip_observations must be positive");
    bool all_zero = true;
    for (int s = 0; s < VSN_NAMES; ++s) {
        const VineEnvRedrawName& nm = names[s];
        S.name[s] = nm;
        const NamedCheck c = named_check(nm, host_values, num_values, false, [s](double v) { return bad_value(s, v); });
        if (c.why) return bad_name(s, c.why);
        all_zero = all_zero && c.hi == 0.0;      // (no value is negative: the largest is zero where all are)
    }
    if (all_zero && !S.per_episode)
        return vine_invalid_arg("env sensor spec: SENSOR_DELAY, SENSOR_HOLD and SENSOR_NOISE_STD are all constant zero: nothing to do");
    S.checked = 1u;
    *out = S;
    return VINE_OK;
}

int vine_env_sensor_scheduled(VineHandle* h, const VineEnvSensorSpec* spec, float* obs, const int64_t* reset,
                              const int64_t* progress, float* sensor_table, float* ring, uint8_t* fresh,
                              int32_t* episode_index, void* stream) {
    if (!h || !spec || !obs || !reset || !progress || !sensor_table || !ring || !fresh || !episode_index)
        return vine_invalid_arg("null argument to vine_env_sensor_scheduled");
    if (spec->abi_version != VINE_ENV_SENSOR_ABI_VERSION) return vine_invalid_arg("VineEnvSensorSpec.abi_version mismatch");
    if (spec->checked != 1u) return vine_invalid_arg("VineEnvSensorSpec was not filled by vine_env_sensor_spec");
    if (spec->num_values > 0 && !spec->values) return vine_invalid_arg("VineEnvSensorSpec.values is NULL");
    const size_t align = spec->num_obs % 4 == 0 ? 16 : 8;
    if (((size_t)obs | (size_t)ring) % align != 0)
        return vine_invalid_arg("vine_env_sensor_scheduled: obs and ring must be aligned to the row vector (16 bytes, 8 where "
                                "num_obs is no multiple of four)");
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
    switch (spec->num_obs) {
        case 14: launch<14>(*spec, info, env_off, obs, reset, progress, sensor_table, ring, fresh, episode_index, st); break;
        case 18: launch<18>(*spec, info, env_off, obs, reset, progress, sensor_table, ring, fresh, episode_index, st); break;
        case 26: launch<26>(*spec, info, env_off, obs, reset, progress, sensor_table, ring, fresh, episode_index, st); break;
        case 28: launch<28>(*spec, info, env_off, obs, reset, progress, sensor_table, ring, fresh, episode_index, st); break;
        default: return vine_invalid_arg("VineEnvSensorSpec.num_obs is not a column count of this library");
    }
    return vine_launch_status("vine_env_sensor");
}

}  // extern "C"
