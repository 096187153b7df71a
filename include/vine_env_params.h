/*
 * vine_env_params.h — per-env physical parameters of the env step (extension of include/vine.h; product library only).
 *
 * A handle steps every env with the one VineConfig it was created with.  A bound table gives each env its own value of the
 * parameters a plant differs by -- joint damping, the FPAM torque constants, the command smoothing, the rail controller and
 * the action delay -- held in device memory as [VP_COUNT][num_envs] floats, the same struct-of-arrays as the state block
 * (parameter p of env e at table[p * num_envs + e]: a wave reads 28 contiguous 256-B segments).
 *
 * The one-lane-per-env kernel (vine_step_kernel) forms each lane's constants from the launch's and the env's column.  The
 * four-lanes-per-env kernel does not read a table, so a handle with a table bound routes like a handle with an obstacle
 * beyond the quad kernel's reach: vine_step_kernel_name says "vine_step_kernel", vine_step_rollout_blocks and
 * vine_step_eval_rows return 0, vine_step_rollout and vine_step_eval return VINE_ERR_UNSUPPORTED.  After unbinding the handle
 * behaves as if it had never been bound.
 *
 * What cannot be overridden per env, and why:
 *   - the cart's and the links' masses and inertias: not in THIS table.  include/vine_env_inertia.h binds a second table
 *     beside it that holds them per env, with the composites the step reads (the constant coefficients a_ij, b_i, g b_i of
 *     the absolute-angle Lagrangian) formed from them in double on the host, as they are when a handle is created;
 *   - lengths, gravity, dt: they reach the kinematics, the contact geometry, the renderer and the recorder, or are
 *     per-launch constants of the substep (the reciprocals);
 *   - STIFFNESS and the link angular damping: whether they are zero selects the substep instantiation of the whole launch;
 *   - the physics-mode flags (implicit joint damping, held FPAM damping, stale body state): they select code paths of the
 *     whole launch as well.
 * No other kernel of the library (init, reset_idx, refresh, stats, render, record, episodes) reads an overridable field.
 */
#ifndef VINE_ENV_PARAMS_H
#define VINE_ENV_PARAMS_H

#include "vine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows of the table; the names are the task YAML's keys (TY:45-58, 100; V5:1045-1048). */
typedef enum VineEnvParam {
    VP_DAMPING = 0,                 /* TY:49 joint damping of all six DOFs */
    VP_SMOOTHING_ALPHA_INFLATE,     /* TY:29, in [0, 1] */
    VP_SMOOTHING_ALPHA_DEFLATE,     /* TY:30, in [0, 1] */
    VP_RAIL_VELOCITY_SCALE,         /* TY:47 */
    VP_RAIL_P_GAIN,                 /* TY:56 */
    VP_RAIL_D_GAIN,                 /* TY:57 */
    VP_RAIL_ACCELERATION,           /* TY:58, >= 0 */
    VP_ACTION_DELAY,                /* TY:100, integer-valued float, 0..VINE_MAX_DELAY: every env has its own FIFO ring */
    VP_FPAM_K0 = 8,                 /* V5:1045, joints 0..4 at VP_FPAM_K0 + j */
    VP_FPAM_C0 = 13,                /* V5:1046 */
    VP_FPAM_b0 = 18,                /* V5:1047 */
    VP_FPAM_B0 = 23,                /* V5:1048 */
    VP_COUNT = 28
} VineEnvParam;

/* Host only.  row[p] = the configuration's own value of parameter p: a table filled with this row in every column
 * reproduces the handle without a table, bit for bit. */
int vine_env_params_row(const VineConfig* cfg, float row[VP_COUNT]);

/* Host only.  host_table: [VP_COUNT][num_envs] floats in host memory.  Every value finite, the alphas in [0, 1], the
 * delay an integer in [0, VINE_MAX_DELAY], RAIL_ACCELERATION >= 0; otherwise VINE_ERR_INVALID_ARG, and vine_last_error()
 * names the parameter and the env.  cfg may be NULL (nothing of it is needed for these conditions today). */
int vine_env_params_check(const VineConfig* cfg, const float* host_table, int num_envs);

/* Bind a table on the handle's device: [VP_COUNT][cfg.num_envs] floats, borrowed (the same ownership rule as
 * vine_bind_reset_values: it must stay valid while bound); NULL unbinds.  The contents are the caller's to check
 * (vine_env_params_check on a host copy) and may be rewritten between steps; a step already captured in a hipGraph keeps
 * the pointer it was captured with and reads whatever the table holds at replay.  Binding or unbinding may change which
 * kernel steps the handle: call it outside a graph capture (it synchronises the device when it does). */
int vine_bind_env_params(VineHandle* h, const float* device_table);

/* 1 while a table is bound, else 0 (0 for a NULL handle). */
int vine_env_params_bound(VineHandle* h);

#ifdef __cplusplus
}
#endif
#endif /* VINE_ENV_PARAMS_H */
