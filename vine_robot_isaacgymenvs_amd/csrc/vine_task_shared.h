// vine_task_shared.h — the pieces of the task that more than one translation unit of libvine_hip.so evaluates, stated once:
// the action -> command map of pre_physics_step (the step kernels of vine_hip.hip; the pin of vine_sysid.hip, which fills
// an env's delay ring with the commands a run through a log would have left) and the tip's forward kinematics from a JOINT
// state (the recorder of vine_record.hip; the pin and the scoring node of vine_sysid.hip).  Per-lane arithmetic on values
// the caller holds in registers: no memory access and no cross-lane operation in here.  Not part of the C ABI.
#ifndef VINE_TASK_SHARED_H
#define VINE_TASK_SHARED_H

#include <hip/hip_runtime.h>

#include "../../include/vine.h"

__device__ __forceinline__ float clampf(float v, float lim) { return fminf(fmaxf(v, -lim), lim); }

// VecTask.step's clamp (vec_task.py:333) and the first half of pre_physics_step (V5:922-934): the action, with its noise
// deviates n0, n1, becomes the command (new_rail, new_fpam).  Params: anything with the members clip_act, act_noise,
// rail_scale, fpam_span and fpam_min (the step kernels' DevParams; vine_sysid.hip's CommandParams).
template <bool RANDOMIZE, class Params>
__device__ __forceinline__ void task_new_command(const Params& P, float2 act, float n0, float n1, float& new_rail,
                                                 float& new_fpam) {
    float a0 = clampf(act.x, P.clip_act), a1 = clampf(act.y, P.clip_act);
    if (RANDOMIZE && P.act_noise != 0.0f) {
        a0 += P.act_noise * n0;
        a1 += P.act_noise * n1;
    }
    new_rail = a0 * P.rail_scale;
    new_fpam = (a1 + 1.0f) * 0.5f * P.fpam_span + P.fpam_min;   // /2 == *0.5 exactly
}

// Tip y, z, vy, vz from a joint state (q[0] cart y, q[1..5] the relative joint angles; qd likewise), in fp32 in the order the
// step kernels use: running sums th_k = q1 + .. + q(k+1), w_k likewise of qd; one sincosf(th_k) per link; the rotation by
// phi0 with (s0, c0) = (sin, cos)(phi0) rounded from double; the four sums accumulated link by link from
// (q0, joint1_z, qd0, 0).  L = link_length, z1 = joint1_z.  (include/vine_record.h documents the same sequence.)
__device__ __forceinline__ void tip_fk_joint(const float* q, const float* qd, float L, float z1, float s0, float c0,
                                             float (&tip)[4]) {
    float ty = q[0], tz = z1, tvy = qd[0], tvz = 0.0f, th = 0.0f, w = 0.0f;
#pragma unroll
    for (int j = 0; j < VINE_NUM_LINKS; ++j) {
        th += q[1 + j];
        w += qd[1 + j];
        float s, cth;
        sincosf(th, &s, &cth);
        const float sp = s0 * cth + c0 * s, cp = c0 * cth - s0 * s;
        ty -= L * sp; tz += L * cp;
        tvy -= L * w * cp; tvz -= L * w * sp;
    }
    tip[0] = ty; tip[1] = tz; tip[2] = tvy; tip[3] = tvz;
}

#endif
