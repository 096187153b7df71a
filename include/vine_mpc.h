/*
 * vine_mpc.h — C ABI of sampling-based model-predictive control (MPC, in the MPPI form) for MI355X (gfx950): K noisy action
 * sequences per plant, rolled H steps through the step kernels, weighted by their costs and averaged, on the device.
 *
 * Only libvine_hip.so exports this header.  Errors, streams and ownership as in vine.h: 0 = ok, negative = VineStatus,
 * message via vine_last_error(); every entry point enqueues on the caller's stream and does not synchronise, allocates
 * nothing and uses no atomics; the caller owns every buffer.  The step kernels are not touched: the three launches below ride
 * in front of, behind and after the model handle's ordinary vine_step launches, and can sit inside a captured hipGraph.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * HANDLES.  Two handles on one device.
 *   The PLANT handle has M envs (M = num_plants): what is being controlled.  Any configuration; its observers run as usual.
 *   The MODEL handle has N = M * K envs (K = samples): env p * K + j is sample j of plant p.
 * The model handle is refused by vine_mpc_fork when it has VINE_FLAG_VINE_RANDOMIZE (VINE_ERR_UNSUPPORTED: a sample must be a
 * deterministic plant), when its VINE_FLAG_CREATE_SHELF / VINE_FLAG_CREATE_PIPE flags differ from the plant's
 * (VINE_ERR_UNSUPPORTED: the obstacle fields of the state block would mean something else), when its max_episode_length
 * differs from the plant's (VINE_ERR_INVALID_ARG: the copied progress would time out elsewhere), when the plant has not
 * num_plants envs or N != M * K (VINE_ERR_INVALID_ARG), and when it sits on another device (VINE_ERR_INVALID_ARG).
 * vine_mpc_scheduled and vine_mpc_update see the model handle only and refuse N != M * K.
 * A per-env parameter table or inertia table may be bound to either handle: the model's table IS the model's plant.
 *
 * CONTROLLER STATE.  All the caller's, on the handles' device:
 *   nominal[M][H][2]              float32   the action sequence the samples are drawn around
 *   history[M][VINE_MAX_DELAY][2] float32   the last actions handed to each plant, most recent first
 *   tick[M]                       int64     control steps done per plant
 *   cost[N]                       float64
 *   alive[N]                      uint8
 *   window[1]                     int64
 *   actions[N][2]                 float32   the model handle's action buffer
 *   plant_actions[M][2]           float32   what the plant's next step consumes
 *
 * NOISE.  The deviate is the sensor's (include/vine_env_sensor.h, step 1): z = float32(2 S - 524280), S the integer sum of
 * the eight 16-bit halves of one Philox-4x32-10 call, scaled by c_a = float32(float64(sigma[a]) * K0),
 * K0 = 1 / sqrt(32 * (65536^2 - 1) / 12) in float64.  The call's counter is
 *   (p * K + j, (unsigned)tick[p], VINE_MPC_RNG_NOISE | (tick[p] >> 32) << 8, 2 k + a)
 * and its key the two words of cfg->seed.  Purpose word 8 is free: the step kernels' own stop at 4, the sensor has 5 and 6,
 * the push 7, the policy head's two are four-letter words.  Sample 0 of every plant has z = 0.
 *
 * The action of sample j at horizon step k, component a:
 *   u[j][k][a] = clamp(nominal[p][k][a] + z * c_a, +-clip_actions of the MODEL handle)
 * one float32 multiply, one float32 add, no contraction.  It is a pure function of (seed, p, j, tick[p], k, a, nominal) and is
 * never stored: the fork, the node and the update each recompute what they need of it.
 *
 * THE FORK.  vine_mpc_fork, one lane per model env e = p * K + j.  Every field of plant p's state-block column is copied to
 * the sample's, except the delay ring VF_FIFO0 .. VF_FIFO0 + 2 * VINE_MAX_DELAY - 1.  Then
 *   progress[e] = the plant's progress[p];  reset[e] = 0;  rew[e] = 0;  cost[e] = 0;  alive[e] = 1;
 *   window[0] = c, the MODEL handle's step count read on the device (steps completed, as every observer reads it).
 * The delay ring is rebuilt as vine_sysid_pin rebuilds it -- not copied: the two handles have different step counts, the
 * model may have another delay, and a real plant's ring could not be read.  d is the sample's own ACTION_DELAY and the
 * constants of the action -> command map the sample's own (from the model's bound parameter table when one is bound, d
 * clamped to 0 .. VINE_MAX_DELAY as the step clamps it, else from the model's configuration).  For k = 1 .. d the command of
 * history[p][k - 1] goes to slot (c - k) mod d; the command is task_new_command<false> of csrc/vine_task_shared.h, the
 * function the step kernels call.  Slots d .. VINE_MAX_DELAY - 1 are not touched.
 *   actions[e] = u[j][0].
 *
 * THE NODE.  vine_mpc_scheduled is enqueued behind every step launch of the model handle on the same stream.  It reads the
 * model's step count c; k = c - window[0].  For 1 <= k <= H and every sample e with alive[e]:
 *   r = rew[e];  if r is not finite: cost[e] = +inf, alive[e] = 0;
 *   else cost[e] += -(double)r, and if the step raised reset[e], alive[e] = 0 after the addition: the step that ends an
 *   episode still counts, which keeps the success reward and the rail penalty.
 * For k < H every sample, alive or not, gets actions[e] = u[j][k].  Outside 1 .. H the launch touches nothing.  Nothing that
 * changes from step to step is a kernel argument, so a captured launch replays correctly.
 *
 * THE UPDATE.  vine_mpc_update, one workgroup of VINE_MPC_THREADS lanes per plant p, no atomics, a fixed reduction order
 * (lane t sums its samples j = t, t + 256, .. in ascending j; the 64 lanes of a wave are combined by a butterfly, the four
 * wave sums added in wave order), so two runs give the same bits.  The workgroup reads nominal[p] into LDS first, then
 *   1. beta = min over j of cost[p * K + j];
 *   2. w_j = exp(-(cost_j - beta) / lambda) in float64 (a +inf cost: weight 0);
 *   3. new[k][a] = float32(sum_j w_j * (double)u[j][k][a] / sum_j w_j);
 *   4. if no cost is finite, new = nominal[p].
 * For a plant whose reset flag (plant_reset[p], the plant handle's reset buffer) is raised -- its next step only consumes the
 * reset -- plant_actions[p] = (0, 0) and nominal[p] becomes zeros.  Otherwise plant_actions[p] = new[0],
 * nominal[p][k] = new[k + 1] and the last entry is repeated: nominal[p][H - 1] = new[H - 1].
 * In both cases history[p] moves back by one entry with the action at its front, and tick[p] += 1.
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_MPC_H
#define VINE_MPC_H

#include <stdint.h>

#include "vine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_MPC_ABI_VERSION 1
#define VINE_MPC_THREADS 256
#define VINE_MPC_MAX_HORIZON 64
#define VINE_MPC_RNG_NOISE 8u      /* the purpose word of the noise stream */

typedef struct VineMpcConfig {
    int32_t abi_version;   /* must be VINE_MPC_ABI_VERSION */
    int32_t num_plants;    /* M; >= 1; the caller sets it (default 0) */
    int32_t samples;       /* K; >= 2; default 256 */
    int32_t horizon;       /* H; 1 .. VINE_MPC_MAX_HORIZON; default 20 */
    double lambda;         /* temperature of the weights; > 0, finite; default 0.05 */
    float sigma[2];        /* noise amplitude per action component; >= 0, finite; default 0.5 */
    uint64_t seed;         /* key of the noise stream; default 0 */
} VineMpcConfig;

int vine_mpc_config_default(VineMpcConfig* cfg);
int vine_mpc_config_size(void);          /* sizeof(VineMpcConfig): checked by the ctypes mirror */

/* Put every sample onto its plant's state (see THE FORK).
 * plant_progress            the plant handle's progress buffer, int64[M]
 * nominal, history, tick    the controller state, read only
 * actions                   device float[N, 2], 8-byte aligned: the action buffer the model's next step consumes
 * rew, reset, progress      the MODEL handle's step buffers (vine.h, vine_step)
 * cost, alive, window       double[N], uint8[N], int64[1] */
int vine_mpc_fork(VineHandle* plant, VineHandle* model, const VineMpcConfig* cfg, const int64_t* plant_progress,
                  const float* nominal, const float* history, const int64_t* tick, float* actions, float* rew,
                  int64_t* reset, int64_t* progress, double* cost, uint8_t* alive, int64_t* window, void* stream);

/* The graph node behind every model step (see THE NODE).  rew, reset: the model handle's step buffers. */
int vine_mpc_scheduled(VineHandle* model, const VineMpcConfig* cfg, const float* nominal, const int64_t* tick,
                       const int64_t* window, float* actions, const float* rew, const int64_t* reset, double* cost,
                       uint8_t* alive, void* stream);

/* Weights, new nominal, the plant's action, the shift (see THE UPDATE).
 * plant_reset      the plant handle's reset buffer, int64[M]
 * plant_actions    device float[M, 2]
 * weights          device double[N] or NULL: where given, w_j of every sample is stored too (0 where no cost of its plant
 *                  is finite) -- a diagnostic, nothing reads it back */
int vine_mpc_update(VineHandle* model, const VineMpcConfig* cfg, const double* cost, const int64_t* plant_reset,
                    float* nominal, float* history, int64_t* tick, float* plant_actions, double* weights, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_MPC_H */
