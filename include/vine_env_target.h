/*
 * vine_env_target.h — a target that moves during the episode (ENV_TARGET; product library only): per-env target velocities
 * along a bounded path, advanced on the device.
 *
 * vine_env_target_scheduled is a launch behind every step (a step observer, like vine_env_push_scheduled) that carries each
 * env's target one control step along its path and puts the target's velocity into the observation the step has just
 * written.  The step kernels read the target from the state block on every step (VF_TARGET_Y/Z, and VF_OBJ_DEPTH for the
 * observation), so moving those floats between steps changes the next step's distance, reward, success test and
 * observation; the step kernels are not touched.  Rewards, flags and progress are never written here: they change only
 * through what the step reads.
 *
 * PER-ENV VALUES.  Env e with global id g = env_id_offset + e runs episode k with four values, held in the device table
 * target[VTG_NAMES][N] (float32): VEL_ALONG and VEL_ACROSS (m/s, signed) and SPAN_ALONG and SPAN_ACROSS (m, >= 0: the path is
 * the offsets [-SPAN, +SPAN] about where the reset put the target).  Each is the draw of include/vine_env_redraw.h
 * (`redraw_value`) under the name keys of "TARGET_VEL_ALONG", "TARGET_VEL_ACROSS", "TARGET_SPAN_ALONG" and "TARGET_SPAN_ACROSS":
 * a pure function of (seed, key, g, k), formed in float64 and rounded once to float32.  Episode 0's table is built by the
 * host.  With per_episode, a lane that sees reset[e] != 0 behind a step -- after it has handled that step -- increments
 * episode_index[e] and writes the four values of the new k: the moment the sensor, the push and the redraw act, so with
 * several of them on their ordinals are equal.  Envs reset from outside the step keep their values and ordinal.
 *
 * PATH.  The mode is the configuration's: VINE_TARGET_FREE (no obstacle): `along` is +y and `across` is +z.
 * VINE_TARGET_SHELF (CREATE_SHELF): `along` is the shelf's depth axis, -y.  VINE_TARGET_PIPE (CREATE_PIPE): `along` is the
 * pipe's axis, -(c, s) with (c, s) = (cos, sin) of VF_OBJ_ANGLE.  In the two obstacle modes a positive offset increases
 * VF_OBJ_DEPTH -- the target moves deeper into the obstacle -- and `across` must be constant zero.  The obstacle stays where
 * the reset put it: it is world geometry, its pose fields (VF_SHELF_Y/Z, VF_PIPE_Y/Z, VF_OBJ_ANGLE) are never written, and the
 * pose a reset would derive from the moved target, the moved depth and the stored angle is the stored pose (vine_hip.hip
 * task_obstacle_poses: shelf_y = ty + (depth - 0.2); pipe_y = ty + depth c + R s, pipe_z = tz + depth s - R c).
 *
 * PER-ENV STATE, the observer's own: motion[VTM_COUNT][N] (float32) -- ANCHOR_Y/Z (where the reset put the target), DEPTH0,
 * AXIS_C/S (pipe: sincosf of VF_OBJ_ANGLE, taken once per episode; else 1, 0), OFF_ALONG/ACROSS, VEL_ALONG/ACROSS (the current
 * signed velocities, flipped at a reflection) --, episode_index[N] and fresh[N] (as the sensor's).
 *
 * Behind a step, for env e, with cdt = dt * controlFrequencyInv the float32 control period of the step kernels:
 *   1. first = progress[e] == 0 (the step kernels leave that behind exactly the steps that consumed the env's reset) or
 *      fresh[e] != 0 (set for every env at set-up, and by the host for envs reset from outside the step).  On first: ANCHOR
 *      takes (VF_TARGET_Y, VF_TARGET_Z) from the state, DEPTH0 takes VF_OBJ_DEPTH (obstacle modes; else 0), AXIS takes the
 *      sincosf (pipe), OFF becomes (0, 0), VEL takes the table's two velocities, fresh[e] is cleared.  So the target of an
 *      episode's first frame is the reset's own, in every bit.
 *   2. an env whose two current velocities are both exactly zero stores nothing more: no field of the state block and no
 *      observation column.  A static env keeps every bit, a -0 included.
 *   3. the target's velocity as it stands now goes into the observation the step wrote:
 *          obs[j] = clamp(obs[j] + w * inv_obs_scale[j], +-clip_observations)        (one float32 multiply, one float32 add)
 *      for j the y and z columns of the target-velocity block (num_obs - 16 + 10 and + 11 in the two scaled layouts, 22 and 23
 *      in the 26-column family, none in POS_ONLY), inv_obs_scale[j] = float32(1 / float64(obs_scaling[j])), the words the step
 *      multiplies by, and the world velocity w = (v_along, v_across) in free space, (-v_along, 0) at the shelf,
 *      ((-v_along) * c, (-v_along) * s) in the pipe.  An add and not a store: with vine_randomize and OBSERVATION_NOISE_STD != 0
 *      the step has already put its noise into those columns; without noise 0 + x is x.
 *   4. advance, per axis (along; across in free space only): n = off + vel * cdt; if n > S: n = S - (n - S), vel = -vel; else
 *      if n < -S: n = -S - (n + S), vel = -vel.  float32 multiplies, adds, subtracts and compares, without contraction.  The
 *      spec check (below) makes one reflection suffice.  OFF and VEL are stored.
 *   5. the target of the next step goes into the state block: each component one multiply where a direction is not exact,
 *      then one add or subtract from the anchor.
 *          free space:  TY = ay + off_along,      TZ = az + off_across
 *          shelf:       TY = ay - off_along,                               VF_OBJ_DEPTH = depth0 + off_along
 *          pipe:        TY = ay - off_along * c,  TZ = az - off_along * s,  VF_OBJ_DEPTH = depth0 + off_along
 *      Nothing else of the state block is ever written.  The depth may leave MIN/MAX_TARGET_DEPTH_IN_OBSTACLE: SPAN is the
 *      user's bound.
 *
 * TIME.  The state holds the target of time k + 1 while the policy decides at time k: step k + 1 compares the tip at k + 1
 * with the target at k + 1 and writes that target, and the depth, into its own observation; the launch behind it therefore
 * adds only the velocity.
 *
 * The kernel: one lane per env, 256 lanes per workgroup, no LDS, no atomics; a lane is the only writer of its env's
 * entries.  Nothing that changes from step to step is a launch argument: a captured launch replays.  The translation unit is
 * compiled without floating-point contraction.
 */
#ifndef VINE_ENV_TARGET_H
#define VINE_ENV_TARGET_H

#include "vine_env_redraw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_ENV_TARGET_ABI_VERSION 1
#define VINE_ENV_TARGET_THREADS 256

/* The names of a spec and the rows of the target table, in this order (the mixed radix of value lists counts in it too). */
typedef enum VineEnvTargetSlot { VTG_VEL_ALONG = 0, VTG_VEL_ACROSS, VTG_SPAN_ALONG, VTG_SPAN_ACROSS, VTG_NAMES = 4 } VineEnvTargetSlot;

/* The rows of the observer's own per-env state. */
typedef enum VineEnvTargetRow {
    VTM_ANCHOR_Y = 0, VTM_ANCHOR_Z, VTM_DEPTH0, VTM_AXIS_C, VTM_AXIS_S, VTM_OFF_ALONG, VTM_OFF_ACROSS, VTM_VEL_ALONG, VTM_VEL_ACROSS,
    VTM_COUNT = 9
} VineEnvTargetRow;

typedef enum VineEnvTargetMode { VINE_TARGET_FREE = 0, VINE_TARGET_SHELF = 1, VINE_TARGET_PIPE = 2 } VineEnvTargetMode;

typedef struct VineEnvTargetSpec {
    int32_t abi_version;            /* VINE_ENV_TARGET_ABI_VERSION */
    int32_t num_values;             /* doubles in the values array */
    uint64_t seed;
    const double* values;           /* DEVICE array of the value lists, the caller's; may be NULL when num_values == 0 */
    VineEnvRedrawName name[VTG_NAMES];      /* every one present: a number, a range or a value list */
    int32_t mode;                   /* VineEnvTargetMode, from the configuration's obstacle flags */
    int32_t num_obs;                /* columns of the configuration's observation */
    int32_t vel_column;             /* the y column of the target-velocity block (z follows it); -1: the layout has none */
    int32_t per_episode;            /* 0: the table is held; 1: redrawn at every reset raised by the step */
    float cdt;                      /* dt * controlFrequencyInv, as the step kernels form it */
    float clip_observations;
    float inv_obs_scale[2];         /* float32(1 / float64(obs_scaling[j])) of the two columns */
    uint32_t checked;               /* set by vine_env_target_spec; vine_env_target_scheduled refuses a spec without it */
    uint32_t reserved;
} VineEnvTargetSpec;

int vine_env_target_spec_size(void);

/* Host only.  Fills *out from the configuration (seed, obstacle flags, observation layout and scaling, dt, controlFrequencyInv,
 * clip_observations, reward weights), the caller's four per-name entries, the value lists (host_values: read for the check;
 * device_values: the same numbers in device memory, only stored) and per_episode.  Refused by name (VINE_ERR_INVALID_ARG,
 * vine_last_error() names TARGET_VEL_ALONG / TARGET_VEL_ACROSS / TARGET_SPAN_ALONG / TARGET_SPAN_ACROSS /
 * VELOCITY_SUCCESS_REWARD_WEIGHT): an absent or unknown form, a non-finite end or value, lo > hi, an extent outside the values
 * array, a radix below 1, a negative SPAN; on an axis whose velocity is not constant zero, max|VEL| * cdt > 2 * min SPAN, both
 * sides formed in float32 from the float32 of the values (one reflection then suffices; this also refuses a moving axis with
 * zero span); with an obstacle, a VEL_ACROSS or SPAN_ACROSS that is not constant zero; CREATE_SHELF together with CREATE_PIPE
 * (VF_OBJ_DEPTH is then the pipe's, and the shelf would not follow); all velocities constant zero with per_episode 0 (nothing
 * to do); a non-zero VELOCITY_SUCCESS_REWARD_WEIGHT (the step's term still assumes a resting target). */
int vine_env_target_spec(const VineConfig* cfg, const VineEnvRedrawName names[VTG_NAMES], const double* host_values,
                         const double* device_values, int num_values, int per_episode, VineEnvTargetSpec* out);

/* Enqueue the target's move behind the step just enqueued on `stream`.  obs: the buffer that step wrote, float [N, num_obs] (it
 * may differ from step to step on the host side; a captured launch keeps the one it was captured with); reset, progress: the
 * step's buffers (int64 [N]); target_table: float [VTG_NAMES, N]; motion: float [VTM_COUNT, N]; fresh: uint8 [N], ones before
 * the first step; episode_index: int32 [N], zeros before the first step.  All on the handle's device.  The state block is the
 * handle's.  VINE_ERR_INVALID_ARG: a null pointer; a spec vine_env_target_spec did not fill, or one whose mode is not that of
 * the handle's obstacle flags. */
int vine_env_target_scheduled(VineHandle* h, const VineEnvTargetSpec* spec, float* obs, const int64_t* reset,
                              const int64_t* progress, float* target_table, float* motion, uint8_t* fresh,
                              int32_t* episode_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_ENV_TARGET_H */
