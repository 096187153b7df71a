/*
 * vine_record.h — C ABI of the trajectory recorder (RECORD_TRAJECTORIES) for MI355X (gfx950).
 *
 * The reference replays a log of the real robot in the simulator (MAT_FILE: the keys cart_pos, Q, moving_target_pos,
 * target_vel, tip_pos, tip_vel; V5:947-982, V5 = isaacgymenvs/tasks/Vine5LinkMovingBase.py of the reference checkout).
 * This header is the way out: a kernel behind every env step copies one fixed-layout row per CHOSEN env from the SoA
 * state block of a VineHandle (include/vine.h) and from the step's outputs into a ring on the device, either into an
 * explicit slot (vine_record) or as a node that decides ON THE DEVICE, from the handle's step counter, whether the step
 * just finished belongs to a recording window (vine_record_scheduled): that form can sit inside a captured hipGraph.
 * It is the numeric twin of include/vine_render.h and follows the same schedule.
 *
 * Only libvine_hip.so exports this header (the CPU oracle does not: it is why these declarations are not in vine.h).
 * Errors, streams and ownership as in vine.h: 0 = ok, negative = VineStatus, message via vine_last_error(); every entry
 * point enqueues on the caller's stream and does not synchronise; the caller owns every buffer.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * THE ROW.  VINE_RECORD_FIELDS = 32 floats (128 bytes) per env and step, VineRecordField below:
 *
 *   0-5    q       VF_Q0 .. +5: cart y and the five relative joint angles
 *   6-11   qd      VF_QD0 .. +5
 *   12-15  tip y, z, vy, vz: forward kinematics of the q, qd of THIS row, evaluated by the recorder in fp32 in the order
 *          the step kernels use (running sums th_k = q1 + .. + q(k+1), w_k likewise of qd; one sincosf(th_k) per link;
 *          the rotation by phi0 with (sin, cos)(phi0) rounded from double; y -= L sin, z += L cos, vy -= L w cos,
 *          vz -= L w sin accumulated link by link from (q0, joint1_z, qd0, 0))
 *   16-17  target y, z                                 VF_TARGET_Y, VF_TARGET_Z
 *   18-19  the two action columns AS HANDED TO THE STEP (before the env's clamp to +-clip_actions, before the delay FIFO)
 *   20     smoothed_u_fpam                             VF_SMOOTHED_U
 *   21     reward                                      rew[e]
 *   22     reset flag, 0 or 1                          reset[e] != 0
 *   23     time-out flag, 0 or 1                       timeouts[e] != 0
 *   24     progress                                    (float)progress[e]
 *   25-26  obj_depth, obj_angle                        VF_OBJ_DEPTH, VF_OBJ_ANGLE
 *   27     contact force norm                          VF_CONTACT with CREATE_SHELF, else 0
 *   28-31  zero (reserved)
 *
 * SEMANTICS.  A row is the state the step LEFT BEHIND, and its reward, flags and progress are what that step wrote.  As
 * in the reference, the step that ends an episode raises the env's reset flag and the NEXT step consumes it in its post
 * phase, after its physics (vine.h, vine_step; V5:1111-1116): the row with reset = 1 is the last state of an episode, and
 * the row after it is the new episode's initial state itself (progress = 0), not that state advanced by a step.
 * The tip fields are computed, not copied: the four-lanes-per-env step kernel stores VF_TIP_* only with
 * VINE_FLAG_INTROSPECT, so the state block's copies are not valid in general.  They therefore DIFFER from the
 * reference's rigid-body tensors in the one step after a reset, where the reference still holds the stale body state of
 * the old episode (V5:796-797, VINE_FLAG_STALE_BODY_STATE_AFTER_RESET): the recorder always gives the kinematics of the
 * recorded joint state.
 * Only fields every step kernel stores unconditionally are copied from the state block.  VF_U_FPAM / VF_U_RAIL (the
 * delayed, clamped controls) are introspection-only and deliberately not in the row: the action columns and
 * smoothed_u_fpam are.
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_RECORD_H
#define VINE_RECORD_H

#include <stdint.h>

#include "vine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_RECORD_ABI_VERSION 1
#define VINE_RECORD_FIELDS 32
#define VINE_RECORD_MAX_ENVS 64

typedef enum VineRecordField {
    VRF_Q0 = 0,
    VRF_QD0 = 6,
    VRF_TIP_Y = 12,
    VRF_TIP_Z = 13,
    VRF_TIP_VY = 14,
    VRF_TIP_VZ = 15,
    VRF_TARGET_Y = 16,
    VRF_TARGET_Z = 17,
    VRF_ACTION0 = 18,
    VRF_SMOOTHED_U = 20,
    VRF_REWARD = 21,
    VRF_RESET = 22,
    VRF_TIMEOUT = 23,
    VRF_PROGRESS = 24,
    VRF_OBJ_DEPTH = 25,
    VRF_OBJ_ANGLE = 26,
    VRF_CONTACT = 27,
    VRF_RESERVED0 = 28
} VineRecordField;

typedef struct VineRecordConfig {
    int32_t abi_version;   /* must be VINE_RECORD_ABI_VERSION */
    int32_t record_every;  /* a window opens at every multiple of this many steps; default 1000 */
    int32_t num_steps;     /* rows per window and env, = slots of the ring; 1 .. record_every; default 500 */
    int32_t num_envs;      /* K, the number of recorded envs; 1 .. VINE_RECORD_MAX_ENVS; default 1 */
} VineRecordConfig;

int vine_record_config_default(VineRecordConfig* cfg);
int vine_record_config_size(void);        /* sizeof(VineRecordConfig): checked by the ctypes mirror */

/* Bytes of the ring: num_steps * num_envs * VINE_RECORD_FIELDS floats; negative = VineStatus. */
int64_t vine_record_ring_bytes(const VineRecordConfig* cfg);

/* Write the row of the step just finished into slot `slot` (0 .. num_steps - 1) of `ring`, unconditionally, and the
 * handle's step index s = steps completed - 1 (-1 before the first step) into steps[slot].
 * envs      device int32[num_envs]; an index outside [0, N) is the caller's error: the task class checks its list on the
 *           host at set-up, and the kernel writes a row of zeros for such an entry (nothing is read out of bounds)
 * actions   device float[N, 2]: the action buffer the step consumed (for vine_step_rollout / vine_step_eval their
 *           action_out)
 * rew, reset, progress, timeouts   the step's output buffers (vine.h, vine_step)
 * ring      device float[num_steps][num_envs][VINE_RECORD_FIELDS]
 * steps     device int64[num_steps] */
int vine_record(VineHandle* h, const VineRecordConfig* cfg, int32_t slot, const int32_t* envs, const float* actions,
                const float* rew, const int64_t* reset, const int64_t* progress, const uint8_t* timeouts, float* ring,
                int64_t* steps, void* stream);

/* The graph node.  Enqueued behind a step launch on the same stream, it reads the handle's device step counter
 * c = steps completed exactly as vine_render_scheduled does; the step just finished has index s = c - 1 and its rows go to
 * slot s % record_every of `ring` (and s to steps[slot]) iff that is < num_steps.  Otherwise (and when c == 0) the launch
 * touches nothing but the two counters.  Nothing that changes from step to step is a kernel argument, so a captured
 * launch replays correctly. */
int vine_record_scheduled(VineHandle* h, const VineRecordConfig* cfg, const int32_t* envs, const float* actions,
                          const float* rew, const int64_t* reset, const int64_t* progress, const uint8_t* timeouts,
                          float* ring, int64_t* steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_RECORD_H */
