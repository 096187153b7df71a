// vine_mpc_shared.h — what the vine_mpc*.hip units state once.  For their kernels: the copy of a plant's state-block column
// onto a sample, the rebuild of the sample's delay ring from an action history, and the workgroup reduction's wave step.  For
// their launch functions (HOST, at the end): the unsupported status, the command constants of a handle, the deviate's scale
// and the refusals of a second handle that could not stand in for the plant.  Include it behind vine_observer.h
// (VineHandleInfo) and vine_task_shared.h (task_new_command, VF_*); that header keeps the contraction it was included under,
// whatever holds here.
#ifndef VINE_MPC_SHARED_H
#define VINE_MPC_SHARED_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

static_assert(VF_PIPE_Y == VF_FIFO0 + 2 * VINE_MAX_DELAY, "the ring is the fields VF_FIFO0 .. VF_PIPE_Y - 1");

// What task_new_command reads (vine_task_shared.h).
struct CommandParams {
    float clip_act, act_noise, rail_scale, fpam_span, fpam_min;
};

// Every field of column p of the block pst[VF_COUNT][m] but the delay ring, onto column e of st[VF_COUNT][n].  A macro, not a
// function: through a function, forced inline or not, the compiler turns two branches of vine_mpc_fork_kernel round (the same
// code, other words), and that kernel's code object is to stay what it was before this header existed.
#define MPC_COPY_COLUMN(pst, m, p, st, n, e)                                                                       \
    do {                                                                                                           \
        for (int f_ = 0; f_ < VF_FIFO0; ++f_) (st)[(size_t)f_ * (n) + (e)] = (pst)[(size_t)f_ * (m) + (p)];         \
        for (int f_ = VF_PIPE_Y; f_ < VF_COUNT; ++f_) (st)[(size_t)f_ * (n) + (e)] = (pst)[(size_t)f_ * (m) + (p)]; \
    } while (0)

// The delay ring of column e at step count c for a sample with delay d and command constants P: for k = 1 .. d the command of
// hist[k - 1] (the action handed k steps ago) goes to slot (c - k) mod d.  Slots d .. VINE_MAX_DELAY - 1 are not touched.
__device__ __forceinline__ void mpc_rebuild_ring(const CommandParams& P, int d, unsigned long long c,
                                                 const float2* hist, float* st, int n, int e) {
    if (d > 0) {
        const int cm = (int)(c % (unsigned long long)d);
        for (int k = 1; k <= d; ++k) {
            float rail, fpam;
            task_new_command<false>(P, hist[k - 1], 0.0f, 0.0f, rail, fpam);
            const int slot = (cm + d - k) % d;                    // (c - k) mod d, k <= d
            st[(size_t)(VF_FIFO0 + 2 * slot) * n + e] = rail;
            st[(size_t)(VF_FIFO0 + 2 * slot + 1) * n + e] = fpam;
        }
    }
}

// The sum (or the minimum) of one value per lane over a wave: a butterfly over its 64 lanes (every lane ends with the same
// bits: a + b == b + a).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}

// The integer of the eight-uniform deviate (include/vine_env_sensor.h, step 1): 2 S - 524280, S the sum of the eight 16-bit
// halves of one Philox call's words.
__device__ __forceinline__ int mpc_deviate_int(const unsigned w[4]) {
    const int sum = (int)((w[0] & 0xffffu) + (w[0] >> 16) + (w[1] & 0xffffu) + (w[1] >> 16) + (w[2] & 0xffffu) +
                          (w[2] >> 16) + (w[3] & 0xffffu) + (w[3] >> 16));
    return 2 * sum - 524280;
}

// ---- HOST: the launch functions' part
inline int unsupported(const char* msg) {
    vine_set_error(msg);
    return VINE_ERR_UNSUPPORTED;
}

// The command constants of a handle's configuration; a sample, a candidate and a predictor add no action noise.
inline CommandParams mpc_command_params(const VineHandleInfo& info) {
    return CommandParams{info.clip_act, 0.0f, info.rail_scale, info.fpam_span, info.fpam_min};
}

// 1 / sqrt(32 * (65536^2 - 1) / 12): the deviate's scale, in float64 (the statement of vine_env_sensor.hip)
inline double noise_scale() { return 1.0 / sqrt(32.0 * (65536.0 * 65536.0 - 1.0) / 12.0); }

// "This second handle (`role`: model, predictor) can stand in for that plant": it sits on the plant's device, does not
// randomize (`why`: what the launch needs that for), and has the plant's obstacles and episode length.  Refused in that order.
inline int mpc_refuse(int status, const char* format, const char* prefix, const char* role, const char* why = "") {
    char msg[200];
    snprintf(msg, sizeof msg, format, prefix, role, why);
    vine_set_error(msg);
    return status;
}
inline int mpc_same_device(const char* prefix, const char* role, const VineHandleInfo& pinfo, const VineHandleInfo& info) {
    if (info.device == pinfo.device) return VINE_OK;
    return mpc_refuse(VINE_ERR_INVALID_ARG, "%s: the %s handle sits on another device than the plant", prefix, role);
}
inline int mpc_stand_in(const char* prefix, const char* role, const char* why, const VineHandleInfo& pinfo,
                        const VineHandleInfo& info) {
    const unsigned obstacles = VINE_FLAG_CREATE_SHELF | VINE_FLAG_CREATE_PIPE;
    if (const int rc = mpc_same_device(prefix, role, pinfo, info)) return rc;
    if (info.flags & VINE_FLAG_VINE_RANDOMIZE)
        return mpc_refuse(VINE_ERR_UNSUPPORTED, "%s: a %s handle with vine_randomize is refused (%s)", prefix, role, why);
    if ((info.flags & obstacles) != (pinfo.flags & obstacles))
        return mpc_refuse(VINE_ERR_UNSUPPORTED, "%s: the %s handle's CREATE_SHELF / CREATE_PIPE differ from the plant's", prefix, role);
    if (info.max_len != pinfo.max_len)
        return mpc_refuse(VINE_ERR_INVALID_ARG, "%s: the %s handle's max_episode_length differs from the plant's", prefix, role);
    return VINE_OK;
}

#endif
