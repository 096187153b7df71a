/*
 * vine_sysid.h — C ABI of system identification (SYSID) for MI355X (gfx950): score every env of a handle against ONE
 * recorded trajectory, on the device.
 *
 * A batch of N envs with a bound per-env parameter table (include/vine_env_params.h) is N candidate plants stepping in one
 * launch.  This header puts all of them onto a row of a log (vine_sysid_pin), feeds them the log's actions from the device
 * and sums, behind every step, each env's squared distance from the log's next row (vine_sysid_scheduled: a node that can
 * sit inside a captured hipGraph, like vine_record_scheduled).  The search over the table is the host's
 * (vine_robot_isaacgymenvs_amd/utils/sysid.py).
 *
 * Only libvine_hip.so exports this header.  Errors, streams and ownership as in vine.h: 0 = ok, negative = VineStatus,
 * message via vine_last_error(); every entry point enqueues on the caller's stream and does not synchronise, allocates
 * nothing and uses no atomics; the caller owns every buffer.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * THE LOG.  log[T][VINE_RECORD_FIELDS] floats on the handle's device: the recorder's rows of ONE env in the VRF_* layout
 * (include/vine_record.h).  Row t is the state step t left behind; its action columns are the action step t consumed.
 * A candidate put onto row r and handed the action of row r + 1 therefore produces its own version of row r + 1.
 *
 * THE PIN.  vine_sysid_pin puts EVERY env of the handle onto log row `row`, as a reset to a given pose (L = the log row):
 *
 *   VF_Q0 .. +5, VF_QD0 .. +5      L[VRF_Q0 ..], L[VRF_QD0 ..]
 *   VF_TIP_Y, _Z, _VY, _VZ         forward kinematics of that q, qd, in the recorder's order of operations (one device
 *                                  function for both: tip_fk_joint of csrc/vine_task_shared.h), NOT the row's tip columns
 *   VF_CART_Y, VF_CART_VY          q0, qd0 (the cart body is the first DOF)
 *   VF_PREV_Q0 .. +5               q
 *   VF_PREV_TIP_Y, _Z              the tip just computed
 *   VF_SMOOTHED_U                  L[VRF_SMOOTHED_U]
 *   VF_PREV_CART_VEL               qd0
 *   VF_PREV_CART_VEL_ERR           0
 *   VF_PREV_U_RAIL                 0
 *   VF_AGG_REW                     0
 *   VF_TARGET_Y, _Z                L[VRF_TARGET_Y], L[VRF_TARGET_Z]
 *   VF_FIFO0 + 2 s, + 2 s + 1      s = 0 .. d - 1, see below; slots d .. VINE_MAX_DELAY - 1 are not touched
 *   rew[e], reset[e], progress[e]  0
 *   actions[e]                     the action of row `row` + 1
 *   window[0], window[1]           c (the handle's device step counter, steps completed) and `row`
 *
 * Every other field of the state block keeps its value (VF_U_FPAM, VF_U_RAIL, VF_RAIL_FORCE, VF_OBJ_*, VF_CONTACT*,
 * VF_SHELF_*, VF_PIPE_*).
 *
 * The delay ring is filled per env.  d is the env's own ACTION_DELAY and the constants of the action -> command map
 * (rail_scale; clip_actions and the FPAM span) are the env's own: from the bound parameter table when one is bound
 * (d clamped to 0 .. VINE_MAX_DELAY as the step clamps it), else from the configuration.  For k = 1 .. d the command of
 * log row (row + 1 - k)'s action goes to slot (c - k) mod d, so that the next d steps read exactly the commands a run
 * through those rows would have left; a row before row 0 gives the command (0, 0), which is what a fresh handle's ring
 * holds.  The command is task_new_command<false> of csrc/vine_task_shared.h, the function the step kernels call.
 *
 * What a row does not hold, and the pin therefore cannot restore: the rail controller's two
 * memories (VF_PREV_CART_VEL of the LAST control iteration, VF_PREV_CART_VEL_ERR) and actions older than the log.  A log
 * that itself began at a pinned row is reproduced exactly from that row.
 *
 * The pin is refused (VINE_ERR_UNSUPPORTED) with VINE_FLAG_CREATE_SHELF / VINE_FLAG_CREATE_PIPE -- obstacle poses are not in
 * a row: sysid is free space only -- and with VINE_FLAG_VINE_RANDOMIZE; and (VINE_ERR_INVALID_ARG) when `row` or
 * `row` + horizon lies outside the log.
 *
 * THE NODE.  vine_sysid_scheduled is enqueued behind a step launch on the same stream.  It reads c and the two window
 * words; k = c - window[0].  For 1 <= k <= horizon (and window[1] + k inside the log) and every env e:
 *   - if alive[e]: when the step raised reset[e], or a compared value of the env is not finite, alive[e] = 0 (the
 *     candidate left the log's episode; nothing is added, the host reports its error as +inf); otherwise
 *     err[e] += sum over the fields f = 0 .. 15 with weights[f] != 0, in that order, of
 *     (double)weights[f] * ((double)x_f - (double)log[window[1] + k][f])^2, the sum formed first and added once.
 *     x_0..11 = VF_Q0 .. VF_QD0 + 5 of the env; x_12..15 = the forward kinematics above (evaluated only when one of
 *     weights[12..15] is not zero).  Without a tip weight, joint fields of weight 0 are not read and need not be finite.
 *     With one, all twelve joint fields are read, because the kinematics needs them: a non-finite q or qd then reaches
 *     the weighted tip fields and ends the env, whatever its own weight.
 *   - actions[e] = the action of log row min(window[1] + k + 1, window[1] + horizon): past the window's end the same
 *     row is written again.
 * Outside 1 .. horizon the launch touches nothing.  Nothing that changes from step to step is a kernel argument, so a
 * captured launch replays correctly.
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_SYSID_H
#define VINE_SYSID_H

#include <stdint.h>

#include "vine.h"
#include "vine_record.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_SYSID_ABI_VERSION 1
#define VINE_SYSID_FIELDS 16       /* the compared row fields: VRF_Q0 .. VRF_TIP_VZ */

typedef struct VineSysidConfig {
    int32_t abi_version;   /* must be VINE_SYSID_ABI_VERSION */
    int32_t num_rows;      /* T, rows of the log; >= 2 */
    int32_t horizon;       /* H, steps per window; 1 .. T - 1; default 50 */
    int32_t reserved;      /* 0 */
    float weights[VINE_SYSID_FIELDS];   /* one per row field 0..15; finite, >= 0; default 1 on the six q, 0 elsewhere */
} VineSysidConfig;

int vine_sysid_config_default(VineSysidConfig* cfg);   /* num_rows = 0: the caller sets it */
int vine_sysid_config_size(void);        /* sizeof(VineSysidConfig): checked by the ctypes mirror */

/* Put every env onto log row `row` (see THE PIN).
 * log       device float[num_rows][VINE_RECORD_FIELDS]
 * actions   device float[N, 2]: the action buffer the next step consumes
 * rew, reset, progress   the step's buffers (vine.h, vine_step)
 * window    device int64[2] */
int vine_sysid_pin(VineHandle* h, const VineSysidConfig* cfg, const float* log, int64_t row, float* actions, float* rew,
                   int64_t* reset, int64_t* progress, int64_t* window, void* stream);

/* The graph node (see THE NODE).
 * reset     the step's reset buffer
 * err       device double[N]
 * alive     device uint8[N] */
int vine_sysid_scheduled(VineHandle* h, const VineSysidConfig* cfg, const float* log, const int64_t* window, float* actions,
                         const int64_t* reset, double* err, uint8_t* alive, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_SYSID_H */
