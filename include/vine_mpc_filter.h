/*
 * vine_mpc_filter.h — C ABI of a fixed-gain corrector (a Luenberger observer, alpha-beta style) over the frames of
 * vine_mpc_observe.h, for MI355X (gfx950): per plant an estimate of the whole state-block column, advanced once per control
 * step by one step of the predictor and pulled towards the frame of that step by two gains.  All of it on the device.
 *
 * Only libvine_hip.so exports this header.  Errors, streams and ownership as in vine.h and vine_mpc_observe.h: 0 = ok,
 * negative = VineStatus, message via vine_last_error(); every entry point enqueues on the caller's stream and does not
 * synchronise, allocates nothing and uses no atomics; the caller owns every buffer.  Neither the step kernels nor the launches
 * of vine_mpc.h and vine_mpc_observe.h are touched.  Nothing that changes from step to step is a kernel argument, so both
 * launches replay from a captured hipGraph.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * HANDLES, CONFIGURATION, TABLE.  The PLANT and the PREDICTOR handle, the VineMpcObserveConfig and the per-plant table of
 * vine_mpc_observe.h, unchanged; a predictor vine_mpc_observe_pin refuses is refused here for the same reason, by name, in
 * front of any launch: the plant handle has not num_plants envs, the predictor handle has not num_plants envs, sits on
 * another device, has VINE_FLAG_VINE_RANDOMIZE, differs in CREATE_SHELF / CREATE_PIPE or in max_episode_length.
 *
 * NOTATION.  At a launch the plant handle has completed c_p steps; s = c_p - 1 is the index of the plant step just done.
 *   known = fresh[p] != 0 or c_p == 0                  (the pin's definition, vine_mpc_observe.h 2.)
 *   dd    = known ? 0 : min(DELAY[p], age[p])          (both clamped to 0 .. VINE_MAX_DELAY)
 *   e     = s - dd                                     the plant step the delivered frame belongs to
 * The filter keeps xhat(e), its estimate of the plant's column behind step e, in a ring of its own with the shape of snap.
 * vine_mpc_observe_pin and vine_mpc_observe_catchup then run UNCHANGED with that ring passed in snap's place: they deliver the
 * estimate instead of the raw frame and predict it forward as before.  So the two launches here only advance xhat(e - 1) to
 * xhat(e), once per control step.
 *
 * FILTER STATE.  All the caller's, on the handles' device; S = VINE_MPC_OBSERVE_SLOTS:
 *   gain[VMF_NAMES][M]       float32   rows GAIN_Q and GAIN_QD, each in [0, 1]; built once by the host and held for the run
 *   est[S][VF_COUNT][M]      float32   the estimate ring, indexed by e mod S; as in snap, the delay-ring fields
 *                                      VF_FIFO0 .. VF_PIPE_Y - 1 are never written and never read
 *   est_index[M]             int64     the e of the estimate last written; -1: none
 *   innov[2][M]              float32   a diagnostic: the sums of squares of the last correction's six q innovations (row 0) and
 *                                      six qd innovations (row 1), added in the order i = 0 .. 5 in float32 without contraction
 *
 * 1. THE PIN.  vine_mpc_filter_pin, one lane per plant, the first launch of a control step.  It prepares one predictor step
 * from xhat(e - 1).  c = the predictor handle's steps completed.
 *   A plant ADVANCES when it is not known, age[p] != 0 and est_index[p] == e - 1 (with est_index[p] >= 0: -1 matches nothing).
 *   An advancing plant:
 *     predictor column p = est[(e - 1) mod S], every field but the delay ring;
 *     progress[p] = plant_progress[p] - dd - 1 (the progress in front of step e, recovered as the observe pin recovers its own);
 *     reset[p] = 0, rew[p] = 0;
 *     the predictor's delay ring is rebuilt with mpc_rebuild_ring of csrc/vine_mpc_shared.h from act_log[p] offset by dd + 1:
 *     for k = 1 .. a the command of act_log[p][dd + k] goes to slot (c - k) mod a, a and the constants of the action -> command
 *     map the predictor env's own, read exactly as the observe pin reads them.  Entries of act_log[p] at or beyond
 *     VINE_MPC_OBSERVE_LOG read as (0, 0) (the host refuses a run in which one could be reached);
 *     actions[p] = act_log[p][dd], the action step e consumed.
 *   Any other plant: its column is put on a valid state -- est[e mod S] when it is not known and est_index[p] == e, else the
 *   plant's own column (every field but the delay ring) -- and actions[p] = (0, 0).  Nothing else of it is written: the step's
 *   result is discarded, and the observe pin behind the correction writes ring, progress, reset and rew of every plant.
 *
 * Then ONE step of the predictor on `actions`.
 *
 * 2. THE CORRECTION.  vine_mpc_filter_correct, one lane per plant, behind that step.  Exactly one case per plant, the first
 * that holds:
 *   a. known:               est_index[p] = -1, nothing else.
 *   b. age[p] == 0          (the frame of step s is an episode's first): the frame snap[s mod S] goes into every slot of est (as
 *                           the measurement fills snap), est_index[p] = s, innov[.][p] = 0.
 *   c. est_index[p] == e:   nothing.
 *   d. advancing:           xminus = predictor column p, y = the frame snap[e mod S].
 *        held(e) = u < HOLD[p] with u the hold draw of the measurement behind step e: a pure function of p, e and cfg->seed, the
 *        Philox call of vine_mpc_observe.h 1. with e in s's place.  The filter draws nothing of its own; it reads that draw
 *        again (purpose word VINE_MPC_FILTER_HOLD_PURPOSE, the measurement's).
 *        held:                xhat = xminus whole -- a dropped frame is predicted through, not delivered again; innov[.][p] = 0.
 *        otherwise the twelve innovations v_i = y_i - xminus_i (one float32 subtract each) and their two sums of squares are
 *        formed and innov[.][p] written, and
 *          both gains exactly 1:  xhat = y whole, its own bits;
 *          all twelve v_i == 0:   xhat = y, but the twelve joint fields and the derived fields keep xminus's own words (the joint
 *                                 values are equal as numbers; a negative zero keeps its sign);
 *          else:                  joint field i: xhat_i = xminus_i + G * v_i, one float32 multiply and one float32 add, G the
 *                                 plant's GAIN_Q for VF_Q0 + i and GAIN_QD for VF_QD0 + i; the derived fields ("Derived fields"
 *                                 of vine_mpc_observe.h 1.: tip and its velocity, cart position and velocity, the previous q,
 *                                 tip and cart velocity) are formed anew from those joint values exactly as the measurement
 *                                 forms them; every other field is y's: the controller's own memories, target and obstacle
 *                                 poses are recorded exactly.
 *        Written to est[e mod S]; est_index[p] = e.
 *   e. anything else        (not reached in a steady run): est[e mod S] = the frame snap[e mod S], est_index[p] = e.
 *
 * 3. THE REST OF THE CONTROL STEP is vine_mpc_observe.h's with est in snap's place: pin, C x (step + catch-up node), the fork
 * from the predictor, horizon, update, plant step, measurement (which keeps writing snap).  The predictor takes C + 1 steps
 * per control step.
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_MPC_FILTER_H
#define VINE_MPC_FILTER_H

#include <stdint.h>

#include "vine.h"
#include "vine_mpc_observe.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_MPC_FILTER_ABI_VERSION 1
#define VINE_MPC_FILTER_THREADS 256
#define VINE_MPC_FILTER_HOLD_PURPOSE VINE_MPC_OBSERVE_RNG_HOLD    /* the measurement's hold draw, read again; no stream of its own */

/* The rows of the gain table, in this order (the mixed radix of value lists counts in it too). */
typedef enum VineMpcFilterSlot { VMF_GAIN_Q = 0, VMF_GAIN_QD, VMF_NAMES = 2 } VineMpcFilterSlot;

int vine_mpc_filter_abi_version(void);       /* VINE_MPC_FILTER_ABI_VERSION: checked by the ctypes mirror */

/* See 1. THE PIN.  table, plant_progress, act_log, age, fresh: as vine_mpc_observe_pin takes them; est: float[S, VF_COUNT, M];
 * est_index: int64[M]; actions: float[M, 2], the action buffer the predictor's next step consumes; actions and act_log 8-byte
 * aligned; rew, reset, progress: the PREDICTOR handle's step buffers. */
int vine_mpc_filter_pin(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* cfg, const float* table,
                        const int64_t* plant_progress, const float* est, const int64_t* est_index, const float* act_log,
                        const int32_t* age, const uint8_t* fresh, float* actions, float* rew, int64_t* reset, int64_t* progress,
                        void* stream);

/* See 2. THE CORRECTION.  gain: float[VMF_NAMES, M]; snap: the measurement's ring; innov: float[2, M]. */
int vine_mpc_filter_correct(VineHandle* plant, VineHandle* predictor, const VineMpcObserveConfig* cfg, const float* table,
                            const float* gain, const float* snap, const int32_t* age, const uint8_t* fresh, float* est,
                            int64_t* est_index, float* innov, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_MPC_FILTER_H */
