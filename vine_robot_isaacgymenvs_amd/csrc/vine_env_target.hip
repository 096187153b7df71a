// vine_env_target.hip — per-env moving targets (ENV_TARGET) for MI355X (gfx950): include/vine_env_target.h states the
// semantics, utils/env_target.py target_replay is the same statement in numpy.
//
// One lane per env, VINE_ENV_TARGET_THREADS envs per workgroup, no LDS, no atomics.  A lane reads its env's four values, its
// progress word, reset word and fresh byte; on an episode's first frame it takes the anchor from the state block, else it
// reads its nine floats of motion state.  A lane whose env rests leaves there.  A moving lane issues its two observation
// loads before anything depends on one, adds the velocity, advances its offsets and stores two or three floats of the state
// block.  The launch is latency-bound at rollout sizes (profiles/env_push/node_cost.txt), not byte-bound.
//
// CONTRACTION IS OFF FOR THIS WHOLE TRANSLATION UNIT, by the pragma in front of everything it includes (native.py compiles it
// with -ffp-contract=fast-honor-pragmas; plain "fast" ignores the pragma): `obs + w * inv`, `off + vel * cdt` and
// `ay - off * c` must stay a multiply and an add, each rounded, as numpy forms them, and the draw of vine_named_draw.h
// must hold the host's bits.  The path step and the words of a point of the path are stated in vine_target_path.h, which
// vine_mpc_track.hip includes too.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/vine_env_target.h"
#include "vine_named_draw.h"
#include "vine_observer.h"
#include "vine_target_path.h"

namespace {

constexpr int THREADS = VINE_ENV_TARGET_THREADS;

template <int MODE>
__global__ __launch_bounds__(THREADS) void vine_env_target_kernel(const VineEnvTargetSpec S, const int n, const unsigned env_off,
                                                                  const unsigned long long* __restrict__ counters, const int glog,
                                                                  float* __restrict__ state, float* __restrict__ obs,
                                                                  const long long* __restrict__ reset,
                                                                  const long long* __restrict__ progress, float* __restrict__ table,
                                                                  float* __restrict__ motion, unsigned char* __restrict__ fresh,
                                                                  int* __restrict__ episode_index) {
    if (vine_steps_completed(counters, glog) == 0ull) return;
    const int e = blockIdx.x * THREADS + (int)threadIdx.x;
    if (e >= n) return;
#define ST(f) state[(size_t)(f) * n + e]
#define MO(r) motion[(size_t)(r) * n + e]

    const bool is_fresh = fresh[e] != 0;
    const bool first = progress[e] == 0 || is_fresh;
    const bool flagged = reset[e] != 0;
    float ay, az, d0, c = 1.0f, s = 0.0f, oa, oc, va, vc;
    if (first) {
        ay = ST(VF_TARGET_Y);
        az = ST(VF_TARGET_Z);
        d0 = MODE != VINE_TARGET_FREE ? ST(VF_OBJ_DEPTH) : 0.0f;
        if (MODE == VINE_TARGET_PIPE) sincosf(ST(VF_OBJ_ANGLE), &s, &c);
        oa = 0.0f;
        oc = 0.0f;
        va = table[(size_t)VTG_VEL_ALONG * n + e];
        vc = table[(size_t)VTG_VEL_ACROSS * n + e];
        MO(VTM_ANCHOR_Y) = ay;
        MO(VTM_ANCHOR_Z) = az;
        MO(VTM_DEPTH0) = d0;
        MO(VTM_AXIS_C) = c;
        MO(VTM_AXIS_S) = s;
        if (is_fresh) fresh[e] = 0;
    } else {
        ay = MO(VTM_ANCHOR_Y);
        az = MO(VTM_ANCHOR_Z);
        d0 = MO(VTM_DEPTH0);
        c = MO(VTM_AXIS_C);
        s = MO(VTM_AXIS_S);
        oa = MO(VTM_OFF_ALONG);
        oc = MO(VTM_OFF_ACROSS);
        va = MO(VTM_VEL_ALONG);
        vc = MO(VTM_VEL_ACROSS);
    }

    const bool moving = va != 0.0f || vc != 0.0f;
    if (moving) {
        if (S.vel_column >= 0) {
            float* const o = obs + (size_t)e * S.num_obs + S.vel_column;
            const float o_y = o[0], o_z = o[1];
            float wy, wz;
            if (MODE == VINE_TARGET_FREE) {
                wy = va;
                wz = vc;
            } else if (MODE == VINE_TARGET_SHELF) {
                wy = -va;
                wz = 0.0f;
            } else {
                wy = (-va) * c;
                wz = (-va) * s;
            }
            const float ty = wy * S.inv_obs_scale[0], tz = wz * S.inv_obs_scale[1];
            const float xy = o_y + ty, xz = o_z + tz;
            o[0] = fminf(fmaxf(xy, -S.clip_observations), S.clip_observations);
            o[1] = fminf(fmaxf(xz, -S.clip_observations), S.clip_observations);
        }
        target_path_advance(oa, va, table[(size_t)VTG_SPAN_ALONG * n + e], S.cdt);
        if (MODE == VINE_TARGET_FREE) target_path_advance(oc, vc, table[(size_t)VTG_SPAN_ACROSS * n + e], S.cdt);
        float ty = 0.0f, tz = 0.0f, depth = 0.0f;
        target_path_words<MODE>(ay, az, d0, c, s, oa, oc, ty, tz, depth);
        ST(VF_TARGET_Y) = ty;
        if (MODE != VINE_TARGET_SHELF) ST(VF_TARGET_Z) = tz;
        if (MODE != VINE_TARGET_FREE) ST(VF_OBJ_DEPTH) = depth;
    }
    if (first || moving) {
        MO(VTM_OFF_ALONG) = oa;
        MO(VTM_OFF_ACROSS) = oc;
        MO(VTM_VEL_ALONG) = va;
        MO(VTM_VEL_ACROSS) = vc;
    }

    if (S.per_episode && flagged) VINE_NAMED_REDRAW_ROWS(VTG_NAMES, S.name, 0u, S.values, S.seed, env_off, e, n, table, episode_index);
#undef ST
#undef MO
}

const char* const kNames[VTG_NAMES] = {"TARGET_VEL_ALONG", "TARGET_VEL_ACROSS", "TARGET_SPAN_ALONG", "TARGET_SPAN_ACROSS"};

int bad_name(int s, const char* why) { return named_refusal("env target spec", kNames[s], why); }

bool is_span(int s) { return s == VTG_SPAN_ALONG || s == VTG_SPAN_ACROSS; }

template <int MODE>
void launch(const VineEnvTargetSpec& S, const VineHandleInfo& info, unsigned env_off, float* obs, const int64_t* reset,
            const int64_t* progress, float* table, float* motion, uint8_t* fresh, int32_t* episode_index, hipStream_t stream) {
    const int blocks = (info.n + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(vine_env_target_kernel<MODE>, dim3(blocks), dim3(THREADS), 0, stream, S, info.n, env_off, info.counters,
                       info.glog, info.state, obs, (const long long*)reset, (const long long*)progress, table, motion, fresh,
                       episode_index);
}

int mode_of(unsigned flags) { return target_path_mode_of(flags); }

}  // namespace

extern "C" {

int vine_env_target_spec_size(void) { return (int)sizeof(VineEnvTargetSpec); }

int vine_env_target_spec(const VineConfig* cfg, const VineEnvRedrawName names[VTG_NAMES], const double* host_values,
                         const double* device_values, int num_values, int per_episode, VineEnvTargetSpec* out) {
    if (!cfg || !names || !out) return vine_invalid_arg("null argument to vine_env_target_spec");
    if (num_values < 0 || (num_values > 0 && (!host_values || !device_values)))
        return vine_invalid_arg("null argument to vine_env_target_spec: the value lists need a host and a device array");
    VineEnvTargetSpec S;
    memset(&S, 0, sizeof S);
    S.abi_version = VINE_ENV_TARGET_ABI_VERSION;
    S.num_values = num_values;
    S.seed = cfg->seed;
    S.values = device_values;
    S.per_episode = per_episode ? 1 : 0;
    if ((cfg->flags & VINE_FLAG_CREATE_SHELF) && (cfg->flags & VINE_FLAG_CREATE_PIPE))
        return vine_invalid_arg("env target spec: CREATE_SHELF together with CREATE_PIPE: VF_OBJ_DEPTH is the pipe's, the shelf "
                                "would not follow the target");
    S.mode = mode_of(cfg->flags);
    S.num_obs = vine_num_obs(cfg);
    switch (cfg->obs_type) {
        case VINE_OBS_POS_AND_FD_VEL_AND_OBJ_INFO:
        case VINE_OBS_TIP_AND_CART_AND_OBJ_INFO: S.vel_column = S.num_obs - 16 + 10; break;
        case VINE_OBS_POS_ONLY: S.vel_column = -1; break;
        case VINE_OBS_POS_AND_VEL:
        case VINE_OBS_POS_AND_FD_VEL:
        case VINE_OBS_POS_AND_PREV_POS: S.vel_column = 22; break;
        default: return vine_invalid_arg("env target spec: the configuration's observation type has no known layout");
    }
    if (S.num_obs < 1 || S.num_obs > VINE_MAX_OBS || S.vel_column + 1 >= S.num_obs)
        return vine_invalid_arg("env target spec: the configuration's observation type has no known column count");
    for (int j = 0; j < 2; ++j)
        S.inv_obs_scale[j] = S.vel_column >= 0 ? (float)(1.0 / (double)cfg->obs_scaling[S.vel_column + j]) : 1.0f;
    S.clip_observations = cfg->clip_observations;
    if (!(S.clip_observations > 0.0f)) return vine_invalid_arg("env target spec: clip_observations must be positive");
    S.cdt = cfg->dt * (float)cfg->control_freq_inv;
    if (!(S.cdt > 0.0f) || !std::isfinite(S.cdt)) return vine_invalid_arg("env target spec: dt * controlFrequencyInv must be positive");
    if (cfg->reward_weights[3] != 0.0f)
        return vine_invalid_arg("env target spec: VELOCITY_SUCCESS_REWARD_WEIGHT must be 0: the step's term assumes a resting target");

    // per name: the largest |value| and the smallest value it can give, as the float32 the table holds
    float max_abs[VTG_NAMES], min_val[VTG_NAMES];
    for (int s = 0; s < VTG_NAMES; ++s) {
        const VineEnvRedrawName& nm = names[s];
        S.name[s] = nm;
        const NamedCheck c = named_check(nm, host_values, num_values, false, any_value);
        if (c.why) return bad_name(s, c.why);
        const double lo = c.lo, hi = c.hi;
        if (is_span(s) && !(lo >= 0.0)) return bad_name(s, "must not be negative");
        if (!std::isfinite((float)lo) || !std::isfinite((float)hi)) return bad_name(s, "does not fit a float32");
        max_abs[s] = fmaxf(fabsf((float)lo), fabsf((float)hi));
        min_val[s] = (float)lo;
    }
    if (S.mode != VINE_TARGET_FREE) {
        if (max_abs[VTG_VEL_ACROSS] != 0.0f) return bad_name(VTG_VEL_ACROSS, "must be constant zero with an obstacle: the target moves along its depth axis only");
        if (max_abs[VTG_SPAN_ACROSS] != 0.0f) return bad_name(VTG_SPAN_ACROSS, "must be constant zero with an obstacle: the target moves along its depth axis only");
    }
    for (int a = 0; a < 2; ++a) {
        const int v = VTG_VEL_ALONG + a, sp = VTG_SPAN_ALONG + a;
        if (max_abs[v] == 0.0f) continue;
        const float step = max_abs[v] * S.cdt, room = 2.0f * min_val[sp];
        if (step > room || !(min_val[sp] > 0.0f))
            return bad_name(v, a == 0 ? "max|VEL| * cdt exceeds 2 * min SPAN_ALONG: one reflection would not keep the target on its path"
                                      : "max|VEL| * cdt exceeds 2 * min SPAN_ACROSS: one reflection would not keep the target on its path");
    }
    if (max_abs[VTG_VEL_ALONG] == 0.0f && max_abs[VTG_VEL_ACROSS] == 0.0f && !S.per_episode)
        return vine_invalid_arg("env target spec: TARGET_VEL_ALONG and TARGET_VEL_ACROSS are both constant zero: nothing to do");
    S.checked = 1u;
    *out = S;
    return VINE_OK;
}

int vine_env_target_scheduled(VineHandle* h, const VineEnvTargetSpec* spec, float* obs, const int64_t* reset,
                              const int64_t* progress, float* target_table, float* motion, uint8_t* fresh,
                              int32_t* episode_index, void* stream) {
    if (!h || !spec || !obs || !reset || !progress || !target_table || !motion || !fresh || !episode_index)
        return vine_invalid_arg("null argument to vine_env_target_scheduled");
    if (spec->abi_version != VINE_ENV_TARGET_ABI_VERSION) return vine_invalid_arg("VineEnvTargetSpec.abi_version mismatch");
    if (spec->checked != 1u) return vine_invalid_arg("VineEnvTargetSpec was not filled by vine_env_target_spec");
    if (spec->num_values > 0 && !spec->values) return vine_invalid_arg("VineEnvTargetSpec.values is NULL");
    if (spec->num_obs < 1 || spec->num_obs > VINE_MAX_OBS || spec->vel_column < -1 || spec->vel_column + 1 >= spec->num_obs)
        return vine_invalid_arg("VineEnvTargetSpec.vel_column lies outside the observation row");
    VineHandleInfo info;
    int rc = vine_handle_info(h, &info);
    if (rc) return rc;
    if (spec->mode != mode_of(info.flags)) return vine_invalid_arg("VineEnvTargetSpec.mode is not that of the handle's obstacle flags");
    const float *bound_params = nullptr, *bound_inertia = nullptr;
    unsigned env_off = 0;
    rc = vine_env_tables_of(h, &bound_params, &bound_inertia, &env_off);
    if (rc) return rc;
    VineDeviceScope scope(info.device);
    if (!scope.ok) return VINE_ERR_DEVICE;
    const hipStream_t st = (hipStream_t)stream;
    switch (spec->mode) {
        case VINE_TARGET_FREE: launch<VINE_TARGET_FREE>(*spec, info, env_off, obs, reset, progress, target_table, motion, fresh, episode_index, st); break;
        case VINE_TARGET_SHELF: launch<VINE_TARGET_SHELF>(*spec, info, env_off, obs, reset, progress, target_table, motion, fresh, episode_index, st); break;
        case VINE_TARGET_PIPE: launch<VINE_TARGET_PIPE>(*spec, info, env_off, obs, reset, progress, target_table, motion, fresh, episode_index, st); break;
        default: return vine_invalid_arg("VineEnvTargetSpec.mode is not a mode of this library");
    }
    return vine_launch_status("vine_env_target");
}

}  // extern "C"
