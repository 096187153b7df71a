// vine_mpc_track.hip — the predictive controller's samples follow their plant's moving target (MPC_TRACK) for MI355X (gfx950):
// include/vine_mpc_track.h states the semantics, utils/mpc_track.py (plan_replay, node_replay) is the same statement in numpy.
//
// Two elementwise kernels, 256 lanes per workgroup, no LDS, no atomics.  The plan has one lane per PLANT: it reads three
// words of the plant's state column, nine floats of the observer's motion block, two spans, a reset word and a fresh byte, and
// writes the plant's H entries of three floats and one byte.  The node has one lane per MODEL env: it reads the model's step
// counter as every observer does (vine_observer.h vine_steps_completed) and returns at once outside the window; inside, a
// lane of a live plant's live sample loads one entry and stores two or three floats of the SoA state block (st[f * n + e]:
// a wave's stores to a field are one contiguous segment).  Both launches are latency-sized, like the target's own
// (profiles/env_target/node_cost.txt), not byte-bound.
//
// CONTRACTION IS OFF FOR THIS WHOLE TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it
// with -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): `off + vel * cdt` and `ay - off * c` must stay a
// multiply and an add, each rounded, as numpy and vine_env_target.hip form them (vine_target_path.h states both once).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "../../include/vine_mpc_track.h"
#include "vine_observer.h"
#include "vine_target_path.h"

namespace {

constexpr int THREADS = VINE_MPC_TRACK_THREADS;
constexpr int WORDS = VINE_MPC_TRACK_WORDS;

template <int MODE>
__global__ __launch_bounds__(THREADS) void vine_mpc_track_plan_kernel(const VineMpcTrackSpec S, const float* __restrict__ pst,
                                                                      const long long* __restrict__ plant_reset,
                                                                      const unsigned char* __restrict__ fresh,
                                                                      const float* __restrict__ table,
                                                                      const float* __restrict__ motion, float* __restrict__ path,
                                                                      unsigned char* __restrict__ live) {
    const int m = S.num_plants, H = S.horizon, p = blockIdx.x * THREADS + (int)threadIdx.x;
    if (p >= m) return;
#define MO(r) motion[(size_t)(r) * m + p]
    const float ty0 = pst[(size_t)VF_TARGET_Y * m + p], tz0 = pst[(size_t)VF_TARGET_Z * m + p];
    const float dp0 = pst[(size_t)VF_OBJ_DEPTH * m + p];
    float* const out = path + (size_t)p * H * WORDS;
    out[0] = ty0;
    out[1] = tz0;
    out[2] = dp0;
    float va = MO(VTM_VEL_ALONG), vc = MO(VTM_VEL_ACROSS);
    const bool is_live = S.path != VINE_TRACK_HELD && plant_reset[p] == 0 && fresh[p] == 0 && (va != 0.0f || vc != 0.0f);
    live[p] = is_live ? 1 : 0;
    if (!is_live) {
        for (int k = 1; k < H; ++k) {
            out[k * WORDS + 0] = ty0;
            out[k * WORDS + 1] = tz0;
            out[k * WORDS + 2] = dp0;
        }
        return;
    }
    const float ay = MO(VTM_ANCHOR_Y), az = MO(VTM_ANCHOR_Z), d0 = MO(VTM_DEPTH0), c = MO(VTM_AXIS_C), s = MO(VTM_AXIS_S);
    float oa = MO(VTM_OFF_ALONG), oc = MO(VTM_OFF_ACROSS);
    const float span_along = table[(size_t)VTG_SPAN_ALONG * m + p], span_across = table[(size_t)VTG_SPAN_ACROSS * m + p];
    const bool exact = S.path == VINE_TRACK_EXACT;
    for (int k = 1; k < H; ++k) {
        if (exact) {
            target_path_advance(oa, va, span_along, S.cdt);
            if (MODE == VINE_TARGET_FREE) target_path_advance(oc, vc, span_across, S.cdt);
        } else {
            const float step_along = va * S.cdt;
            oa = oa + step_along;
            if (MODE == VINE_TARGET_FREE) {
                const float step_across = vc * S.cdt;
                oc = oc + step_across;
            }
        }
        float ty = ty0, tz = tz0, depth = dp0;
        target_path_words<MODE>(ay, az, d0, c, s, oa, oc, ty, tz, depth);
        out[k * WORDS + 0] = ty;
        out[k * WORDS + 1] = tz;
        out[k * WORDS + 2] = depth;
    }
#undef MO
}

__global__ __launch_bounds__(THREADS) void vine_mpc_track_node_kernel(const VineMpcTrackSpec S, const int n, const int glog,
                                                                      const unsigned long long* __restrict__ counters,
                                                                      float* __restrict__ st, const long long* __restrict__ window,
                                                                      const unsigned char* __restrict__ alive,
                                                                      const float* __restrict__ path,
                                                                      const unsigned char* __restrict__ live) {
    const long long c = (long long)vine_steps_completed(counters, glog);
    const long long k = c - window[0];
    if (k < 1 || k > (long long)S.horizon - 1) return;
    const int e = blockIdx.x * THREADS + (int)threadIdx.x;
    if (e >= n) return;
    const int p = e / S.samples;
    if (live[p] == 0 || alive[e] == 0) return;
    const float* const w = path + ((size_t)p * S.horizon + (int)k) * WORDS;
    st[(size_t)VF_TARGET_Y * n + e] = w[0];
    if (S.mode != VINE_TARGET_SHELF) st[(size_t)VF_TARGET_Z * n + e] = w[1];
    if (S.mode != VINE_TARGET_FREE) st[(size_t)VF_OBJ_DEPTH * n + e] = w[2];
}

// What both launches refuse of a spec before they look at a handle.
int check_spec(const VineMpcTrackSpec* spec) {
    if (spec->abi_version != VINE_MPC_TRACK_ABI_VERSION) return vine_invalid_arg("VineMpcTrackSpec.abi_version mismatch");
    if (spec->checked != 1u) return vine_invalid_arg("VineMpcTrackSpec was not filled by vine_mpc_track_spec");
    if (spec->num_plants < 1 || spec->samples < 2 || spec->horizon < 1 || spec->horizon > VINE_MPC_MAX_HORIZON)
        return vine_invalid_arg("VineMpcTrackSpec: num_plants, samples or horizon lies outside what vine_mpc_track_spec fills");
    return VINE_OK;
}

int check_mode(const VineMpcTrackSpec* spec, const VineHandleInfo& info) {
    if (spec->mode != target_path_mode_of(info.flags))
        return vine_invalid_arg("VineMpcTrackSpec.mode is not that of the handle's obstacle flags");
    return VINE_OK;
}

template <int MODE>
void launch_plan(const VineMpcTrackSpec& S, const VineHandleInfo& info, const int64_t* plant_reset, const uint8_t* fresh,
                 const float* table, const float* motion, float* path, uint8_t* live, hipStream_t stream) {
    hipLaunchKernelGGL(vine_mpc_track_plan_kernel<MODE>, dim3((S.num_plants + THREADS - 1) / THREADS), dim3(THREADS), 0, stream, S,
                       (const float*)info.state, (const long long*)plant_reset, fresh, table, motion, path, live);
}

}  // namespace

extern "C" {

int vine_mpc_track_spec_size(void) { return (int)sizeof(VineMpcTrackSpec); }

int vine_mpc_track_spec(const VineEnvTargetSpec* plant_spec, const VineMpcConfig* cfg, int path, VineMpcTrackSpec* out) {
    if (!plant_spec || !cfg || !out) return vine_invalid_arg("null argument to vine_mpc_track_spec");
    if (plant_spec->abi_version != VINE_ENV_TARGET_ABI_VERSION)
        return vine_invalid_arg("mpc track spec: VineEnvTargetSpec.abi_version mismatch");
    if (plant_spec->checked != 1u)
        return vine_invalid_arg("mpc track spec: the plant's VineEnvTargetSpec was not filled by vine_env_target_spec");
    if (plant_spec->mode != VINE_TARGET_FREE && plant_spec->mode != VINE_TARGET_SHELF && plant_spec->mode != VINE_TARGET_PIPE)
        return vine_invalid_arg("mpc track spec: the plant's VineEnvTargetSpec.mode is not a mode of this library");
    if (cfg->abi_version != VINE_MPC_ABI_VERSION) return vine_invalid_arg("mpc track spec: VineMpcConfig.abi_version mismatch");
    if (cfg->num_plants < 1) return vine_invalid_arg("mpc track spec: num_plants must be at least 1");
    if (cfg->samples < 2) return vine_invalid_arg("mpc track spec: samples must be at least 2");
    if ((long long)cfg->num_plants * cfg->samples > 0x7fffffffLL)
        return vine_invalid_arg("mpc track spec: num_plants * samples does not fit an int32");
    if (path != VINE_TRACK_EXACT && path != VINE_TRACK_LINEAR && path != VINE_TRACK_HELD) {
        char msg[120];
        snprintf(msg, sizeof msg, "mpc track spec: path %d is not exact (0), linear (1) or held (2)", path);
        return vine_invalid_arg(msg);
    }
    if (cfg->horizon < 1 || cfg->horizon > VINE_MPC_MAX_HORIZON)
        return vine_invalid_arg("mpc track spec: needs 1 <= horizon <= VINE_MPC_MAX_HORIZON (64)");
    VineMpcTrackSpec S;
    memset(&S, 0, sizeof S);
    S.abi_version = VINE_MPC_TRACK_ABI_VERSION;
    S.num_plants = cfg->num_plants;
    S.samples = cfg->samples;
    S.horizon = cfg->horizon;
    S.mode = plant_spec->mode;
    S.path = path;
    S.cdt = plant_spec->cdt;
    S.checked = 1u;
    *out = S;
    return VINE_OK;
}

int vine_mpc_track_plan(VineHandle* plant, const VineMpcTrackSpec* spec, const int64_t* plant_reset, const uint8_t* fresh,
                        const float* target_table, const float* motion, float* path, uint8_t* live, void* stream) {
    if (!plant || !spec || !plant_reset || !fresh || !target_table || !motion || !path || !live)
        return vine_invalid_arg("null argument to vine_mpc_track_plan");
    int rc = check_spec(spec);
    if (rc) return rc;
    VineHandleInfo info;
    rc = vine_handle_info(plant, &info);
    if (rc) return rc;
    if (info.n != spec->num_plants) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc track plan: the plant handle has %d envs, not num_plants = %d", info.n, spec->num_plants);
        return vine_invalid_arg(msg);
    }
    rc = check_mode(spec, info);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    const hipStream_t st = (hipStream_t)stream;
    switch (spec->mode) {
        case VINE_TARGET_FREE: launch_plan<VINE_TARGET_FREE>(*spec, info, plant_reset, fresh, target_table, motion, path, live, st); break;
        case VINE_TARGET_SHELF: launch_plan<VINE_TARGET_SHELF>(*spec, info, plant_reset, fresh, target_table, motion, path, live, st); break;
        default: launch_plan<VINE_TARGET_PIPE>(*spec, info, plant_reset, fresh, target_table, motion, path, live, st); break;
    }
    return vine_launch_status("vine_mpc_track_plan");
}

int vine_mpc_track_scheduled(VineHandle* model, const VineMpcTrackSpec* spec, const int64_t* window, const uint8_t* alive,
                             const float* path, const uint8_t* live, void* stream) {
    if (!model || !spec || !window || !alive || !path || !live) return vine_invalid_arg("null argument to vine_mpc_track_scheduled");
    int rc = check_spec(spec);
    if (rc) return rc;
    VineHandleInfo info;
    rc = vine_handle_info(model, &info);
    if (rc) return rc;
    if ((long long)info.n != (long long)spec->num_plants * spec->samples) {
        char msg[200];
        snprintf(msg, sizeof msg, "mpc track node: the model handle has %d envs, not num_plants * samples = %d * %d", info.n,
                 spec->num_plants, spec->samples);
        return vine_invalid_arg(msg);
    }
    rc = check_mode(spec, info);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    hipLaunchKernelGGL(vine_mpc_track_node_kernel, dim3((info.n + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream,
                       *spec, info.n, info.glog, info.counters, info.state, (const long long*)window, alive, path, live);
    return vine_launch_status("vine_mpc_track_scheduled");
}

}  // extern "C"
