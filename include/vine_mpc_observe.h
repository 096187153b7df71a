/*
 * vine_mpc_observe.h — C ABI of a sensing path for the predictive controller of vine_mpc.h, for MI355X (gfx950): the
 * controller receives the state of each plant some control steps late, with noise and dropped frames, puts a model copy of the
 * plant onto that measurement, replays the actions it has sent since then and plans from the predicted "now".  All of it on
 * the device.
 *
 * Only libvine_hip.so exports this header.  Errors, streams and ownership as in vine.h and vine_mpc.h: 0 = ok, negative =
 * VineStatus, message via vine_last_error(); every entry point enqueues on the caller's stream and does not synchronise,
 * allocates nothing and uses no atomics; the caller owns every buffer.  Neither the step kernels nor the launches of
 * vine_mpc.h are touched.  Nothing that changes from step to step is a kernel argument, so all three launches replay from a
 * captured hipGraph.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * HANDLES.  The PLANT handle (M envs) and the MODEL handle (N = M * K envs) of vine_mpc.h, and a third, the PREDICTOR: M
 * envs, env p the model's copy of plant p.  A per-env parameter table may be bound to it: that table IS the predictor's plant.
 * The catch-up below runs on the predictor, not on the N samples -- all K samples of a plant would compute the same thing.
 * Behind the catch-up vine_mpc_fork is called with the predictor in the plant's place (predictor handle, predictor progress
 * buffer) and the controller's ordinary history, nominal and tick; vine_mpc_update still gets the real plant's reset buffer.
 * The predictor is refused by vine_mpc_observe_pin and vine_mpc_observe_catchup when it has not num_plants envs
 * (VINE_ERR_INVALID_ARG), sits on another device than the plant (VINE_ERR_INVALID_ARG), has VINE_FLAG_VINE_RANDOMIZE
 * (VINE_ERR_UNSUPPORTED: a replayed step must be a deterministic one), when its VINE_FLAG_CREATE_SHELF / VINE_FLAG_CREATE_PIPE
 * flags differ from the plant's (VINE_ERR_UNSUPPORTED) and when its max_episode_length differs from the plant's
 * (VINE_ERR_INVALID_ARG).  One rank: the global env id of plant p is p.
 *
 * PER-PLANT VALUES.  table[VMO_NAMES][M] float32: DELAY (whole control steps, 0 .. VINE_MAX_DELAY), HOLD (probability per
 * step that no new frame arrives, [0, 1)), NOISE_Q and NOISE_QD (>= 0, in the units of VF_Q* and VF_QD*).  Built once by the
 * host and held for the run.  The kernels clamp DELAY to 0 .. VINE_MAX_DELAY where it indexes.
 *
 * CONTROLLER STATE.  All the caller's, on the handles' device; S = VINE_MPC_OBSERVE_SLOTS = VINE_MAX_DELAY + 1:
 *   snap[S][VF_COUNT][M]                  float32   ring of frames, indexed by the plant step's index mod S (the PLANT handle's
 *                                                   step count read on the device, as the sensor's ring is)
 *   act_log[M][2 * VINE_MAX_DELAY][2]     float32   the actions the plant consumed, most recent first (sensor delay plus action
 *                                                   delay <= 16 entries are ever read)
 *   age[M]                                int32     plant steps since the episode's first frame, saturating at VINE_MAX_DELAY
 *   fresh[M]                              uint8     ones before the first step, and set by the host for plants reset from
 *                                                   outside the step
 *   lag[M]                                int32     a diagnostic: the d of the last pin
 * A frame is a whole state-block column but the delay ring VF_FIFO0 .. VF_PIPE_Y - 1: those entries of snap are never written
 * and never read -- a real plant's ring could not be.  The twelve joint fields carry the sensor's noise; everything else is
 * recorded as it was behind that step: the controller's own memories (VF_SMOOTHED_U, VF_U_*, VF_PREV_U_RAIL,
 * VF_PREV_CART_VEL_ERR, VF_RAIL_FORCE), target and obstacle poses.
 *
 * 1. THE MEASUREMENT.  vine_mpc_observe_measure, one lane per plant, enqueued behind every plant step.  c = the plant
 * handle's steps completed; with c == 0 the launch touches nothing.  s = c - 1, the index of the step just done.
 *   Frame.  The frame is the plant's column.  Where NOISE_Q[p] != 0, for i = 0 .. 5
 *       frame[VF_Q0 + i] = q_i + z * c_q            (one float32 multiply, one float32 add, no contraction)
 *       c_q = float32(float64(NOISE_Q[p]) * K0),  K0 = 1 / sqrt(32 * (65536^2 - 1) / 12) in float64
 *       z = float32(2 * S8 - 524280), S8 the integer sum of the eight 16-bit halves of one Philox-4x32-10 call (the deviate
 *       of include/vine_env_sensor.h, step 1) with counter (p, (unsigned)s, VINE_MPC_OBSERVE_RNG_NOISE | (s >> 32) << 8, i)
 *       and the two words of cfg->seed as its key.
 *   Where NOISE_QD[p] != 0, frame[VF_QD0 + i] is formed likewise from qd_i, c_qd and the counter's last word 6 + i.
 *   Purpose words 10 and 11 are the next free ones: the step kernels' own stop at 4, the sensor has 5 and 6, the push 7, the
 *   controller's noise 8, the adaptation's candidates 9.
 *   Derived fields.  Where either noise value of the plant is non-zero, the fields a joint state determines are formed anew
 *   from the noisy q, qd exactly as vine_sysid_pin forms them: (VF_TIP_Y, VF_TIP_Z, VF_TIP_VY, VF_TIP_VZ) = tip_fk_joint of
 *   csrc/vine_task_shared.h; VF_CART_Y = q0, VF_CART_VY = qd0; VF_PREV_Q0 + i = q_i; (VF_PREV_TIP_Y, VF_PREV_TIP_Z) = that
 *   tip; VF_PREV_CART_VEL = qd0.  A noise-free frame keeps the column's own bits.
 *   Ring.  first = plant_progress[p] == 0 (the step consumed the plant's reset) or fresh[p] != 0.
 *     first: the frame goes into every slot, age[p] = 0, fresh[p] = 0.
 *     else:  held = u < HOLD[p] (float32) with u = (w >> 8) * 2^-24, w = word 0 of the Philox call with counter
 *            (p, (unsigned)s, VINE_MPC_OBSERVE_RNG_HOLD | (s >> 32) << 8, 0) -- the sensor's step 4;
 *            slot s % S = held ? slot (s - 1) % S : the frame;  age[p] = min(age[p] + 1, VINE_MAX_DELAY).
 *   Action log.  act_log[p] moves back by one entry with plant_actions[p] (what that step consumed) at its front: the move
 *   vine_mpc_update makes on history, only deeper.
 *
 * 2. THE PIN.  vine_mpc_observe_pin, one lane per plant, enqueued in front of the catch-up; it is also the re-pin the
 * catch-up node applies (one device function for both).  c_p = the plant handle's steps completed, s = c_p - 1, c = the
 * predictor handle's.  C = cfg->catchup.
 *   known = fresh[p] != 0 or c_p == 0: no frame of this plant has been measured since it was put on a state from outside the
 *   step (set-up, reset_idx).  That state is the controller's own doing, so the plant's column itself is delivered, dd = 0.
 *   Otherwise dd = min(DELAY[p], age[p]) and the delivered frame is snap[(s - dd) % S].
 *   d = cfg->compensate ? min(dd, C) : 0.  With compensate off the stale frame is still what is delivered; it is just not
 *   predicted forward.  (The host refuses C below the table's largest DELAY, so min(dd, C) = dd.)
 *   Every field of the delivered frame but the ring is written onto predictor column p.
 *   progress[p] = plant_progress[p] - dd: RECOVERED, not carried in the ring -- between an episode's first frame and now the
 *   plant's progress grows by one per step, and dd never reaches behind the first frame.
 *   reset[p] = 0, rew[p] = 0, lag[p] = d.
 *   The predictor's delay ring is rebuilt with mpc_rebuild_ring of csrc/vine_mpc_shared.h from act_log[p] offset by d: for
 *   k = 1 .. a the command of act_log[p][d + k - 1] goes to slot (c - k) mod a; a is the predictor env's own ACTION_DELAY and
 *   the constants of the action -> command map its own (from the predictor's bound table when one is bound, else from its
 *   configuration), as vine_mpc_fork reads the sample's.  Slots a .. VINE_MAX_DELAY - 1 are not touched.
 *   actions[p] = the next action of 3. with i = 0.
 *
 * 3. THE CATCH-UP NODE.  vine_mpc_observe_catchup(step_index = i) is enqueued behind the i-th of the C predictor steps,
 * i = 1 .. C.  The d real steps of a plant are the last d of the C; d is formed as the pin formed it (table, age and fresh do
 * not change in between; lag is written, never read).
 *   i <= C - d   the step just run did not count: the plant is pinned again (2., with the predictor's step count as it is
 *                now).
 *   i >  C - d   a real step: reset[p] = 0.  The real plant is known to be inside its episode, or `first` would have held.
 *   Next action, for i < C (and for the pin, i = 0): actions[p] = i >= C - d ? act_log[p][C - i - 1] : (0, 0).  Behind the
 *   last step no action is written.  With C = 0 no step and no node is issued.
 * The step index is the launch's place in the control step, the same at every replay of a captured graph.
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_MPC_OBSERVE_H
#define VINE_MPC_OBSERVE_H

#include <stdint.h>

#include "vine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_MPC_OBSERVE_ABI_VERSION 1
#define VINE_MPC_OBSERVE_THREADS 256
#define VINE_MPC_OBSERVE_SLOTS (VINE_MAX_DELAY + 1)
#define VINE_MPC_OBSERVE_LOG (2 * VINE_MAX_DELAY)    /* entries of act_log per plant */
#define VINE_MPC_OBSERVE_RNG_NOISE 10u               /* the purpose words of the two Philox streams */
#define VINE_MPC_OBSERVE_RNG_HOLD 11u

/* The rows of the per-plant table, in this order (the mixed radix of value lists counts in it too). */
typedef enum VineMpcObserveSlot { VMO_DELAY = 0, VMO_HOLD, VMO_NOISE_Q, VMO_NOISE_QD, VMO_NAMES = 4 } VineMpcObserveSlot;

typedef struct VineMpcObserveConfig {
    int32_t abi_version;   /* must be VINE_MPC_OBSERVE_ABI_VERSION */
    int32_t num_plants;    /* M; >= 1; the caller sets it (default 0) */
    int32_t catchup;       /* C; predictor steps per control step; 0 .. VINE_MAX_DELAY; default 0 */
    int32_t compensate;    /* 0 or 1; default 1 */
    uint64_t seed;         /* key of the noise and hold streams; default 0 */
} VineMpcObserveConfig;

int vine_mpc_observe_config_default(VineMpcObserveConfig* cfg);
int vine_mpc_observe_config_size(void);      /* sizeof(VineMpcObserveConfig): checked by the ctypes mirror */

/* See 1. THE MEASUREMENT.  table: float[VMO_NAMES, M]; plant_progress: the plant handle's progress buffer, int64[M];
 * plant_actions: float[M, 2], what the step just done consumed; act_log and plant_actions 8-byte aligned. */
int vine_mpc_observe_measure(VineHandle* plant, const VineMpcObserveConfig* cfg, const float* table,
                             const int64_t* plant_progress, const float* plant_actions, float* snap, float* act_log,
                             int32_t* age, uint8_t* fresh, void* stream);

/* See 2. THE PIN.  actions: float[M, 2], 8-byte aligned, the action buffer the predictor's next step consumes; rew, reset,
 * progress: the PREDICTOR handle's step buffers (vine.h, vine_step). */
int vine_mpc_observe_pin(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* cfg, const float* table,
                         const int64_t* plant_progress, const float* snap, const float* act_log, const int32_t* age,
                         const uint8_t* fresh, float* actions, float* rew, int64_t* reset, int64_t* progress, int32_t* lag,
                         void* stream);

/* See 3. THE CATCH-UP NODE.  step_index: 1 .. cfg->catchup; the other arguments as the pin's. */
int vine_mpc_observe_catchup(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* cfg, int32_t step_index,
                             const float* table, const int64_t* plant_progress, const float* snap, const float* act_log,
                             const int32_t* age, const uint8_t* fresh, float* actions, float* rew, int64_t* reset,
                             int64_t* progress, int32_t* lag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_MPC_OBSERVE_H */
