/*
 * vine_mpc_ensemble.h — the predictive controller scores every action sequence on several candidate plants (MPC_ENSEMBLE;
 * product library only): the K samples of a plant are G sequences times E members, the members of a sequence share one
 * perturbation and differ in the model's plant, and the update weights a sequence by a risk over its members' costs.
 *
 * include/vine_mpc.h plans through one model per plant: every sample of plant p is rolled through the same parameters.  A
 * controller that knows only the RANGE of its plant has to ask of every sequence what it costs on each plant of that range.
 * This header adds exactly that and nothing else: the fork, the node and the step kernels are not touched, vine_mpc.hip is not
 * edited.  The model handle's parameter and inertia tables carry the members (the model's table IS the model's plant, and the
 * fork rebuilds every sample's delay ring from the sample's own ACTION_DELAY); what is added on the device is the common
 * perturbation and the reduction over members.  Two launches: one behind the fork and behind every base node overwrites the
 * white action the base launch left with the group's, and an update that reduces over members before it reduces over
 * sequences takes vine_mpc_update's place.
 *
 * Errors, streams and ownership as in vine_mpc.h: every entry point enqueues on the caller's stream and does not synchronise,
 * allocates nothing and uses no atomics; the caller owns every buffer; M = num_plants, K = samples, H = horizon, N = M * K of
 * the VineMpcConfig passed beside the VineMpcEnsembleConfig.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * THE LAYOUT.  K = G * E, E = members, G = K / E the number of sequences (groups) per plant.  Sample j of plant p is member
 * m = j mod E of group g = j / E: a group's members are E consecutive model envs, p * K + g * E .. p * K + g * E + E - 1, and
 * member m of every group of a plant is meant to be the same candidate plant (the caller's tables say so; nothing here reads
 * them).
 *
 * THE CONFIGURATION.  VineMpcEnsembleConfig:
 *   members   E, 1 .. VINE_MPC_ENSEMBLE_MAX_MEMBERS, a divisor of cfg->samples; 1: the controller of include/vine_mpc.h
 *   risk      VINE_MPC_RISK_MEAN, VINE_MPC_RISK_MAX or VINE_MPC_RISK_ENTROPIC: how a group's member costs become its cost
 *   theta     with VINE_MPC_RISK_ENTROPIC: the risk aversion, finite and > 0 (towards 0 the mean, towards infinity the
 *             maximum); ignored otherwise
 * Refused with VINE_ERR_INVALID_ARG, vine_last_error() naming the field: members outside 1 .. 16; members that do not divide
 * samples; a risk that is none of the three; with ENTROPIC, a theta that is not finite or not > 0.  Every entry point also
 * refuses what vine_mpc.hip refuses of the VineMpcConfig, null arguments, float2 buffers that are not 8-byte aligned, and a
 * model handle without N = M * K envs, in vine_mpc.hip's words.
 *
 * THE PERTURBATION OF A GROUP.  The base deviate of include/vine_mpc.h, NOISE, under the same key and the counter
 *   (p * G + g, (unsigned)tick[p], VINE_MPC_RNG_NOISE | (tick[p] >> 32) << 8, 2 k + a)
 * The first word is the group's index in a controller of G samples, not the leader's model env p * K + g * E: an ensemble of
 * identical members then draws the words a plain controller with samples = G draws, and is that controller.  Group 0 of
 * every plant has z = 0.  The action of group g at horizon step k, component a:
 *   u_g[k][a] = clamp(nominal[p][k][a] + z * c_a, +-clip_actions of the MODEL handle)
 * c_a of include/vine_mpc.h; one float32 multiply, one float32 add, no contraction.  It is never stored per group: the node
 * and the update each recompute what they need of it.
 *
 * 1. THE NODE.  vine_mpc_ensemble_scheduled, one lane per model env, enqueued once behind vine_mpc_fork and once behind every
 * vine_mpc_scheduled of the horizon on the same stream.  It reads the MODEL handle's step count c as every observer reads it;
 * k = c - window[0].  For 0 <= k < H every sample, alive or not, gets
 *   actions[e] = u_g[k],   g = (e mod K) / E
 * Outside that window the launch touches nothing.  Nothing that changes from step to step is a kernel argument, so a captured
 * launch replays correctly.  The base fork and node stay in the chain unchanged -- the state copy, the ring rebuild and the
 * cost sums are theirs -- and this launch overwrites the white action they left.  With E = 1 it stores the words that were
 * there.
 *
 * 2. THE UPDATE.  vine_mpc_ensemble_update, in place of vine_mpc_update; one workgroup of VINE_MPC_THREADS lanes per plant, a
 * fixed reduction order (lane t takes its groups g = t, t + 256, .. in ascending g; the 64 lanes of a wave are combined by a
 * butterfly, the four wave values in wave order), so two runs give the same bits.  With c_m = cost[p * K + g * E + m] the
 * cost of group g is
 *   any c_m not finite   C_g = +inf: a sequence that breaks any candidate plant is discarded
 *   MEAN                 C_g = (c_0 + c_1 + .. in ascending m) / E
 *   MAX                  C_g = max_m c_m
 *   ENTROPIC             C_g = cmax + log((sum_m exp(theta * (c_m - cmax)), in ascending m) / E) / theta,   cmax = max_m c_m
 * all in float64, each operation rounded (no contraction).  Then the statement of include/vine_mpc.h, THE UPDATE, word for
 * word with the groups in the place of the samples and u_g in the place of u: beta = min_g C_g; w_g = exp(-(C_g - beta) /
 * lambda) in float64 (+inf: weight 0); new = float32(sum_g w_g u_g / sum_g w_g); new = nominal[p] where no group cost is
 * finite; the reset branch; the shift; the history; the tick.  Optional outputs, each NULL or given:
 *   weights[N]         w_g, stored into every member of the group (0 where no group cost of the plant is finite)
 *   group_cost[M * G]  C_g
 * diagnostics, nothing reads them back.  With E = 1 every risk gives C_g = c_g in every bit (x / 1, max of one, and
 * cmax + log(exp(0) / 1) / theta = cmax + 0), so the launch is vine_mpc_update's.
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_MPC_ENSEMBLE_H
#define VINE_MPC_ENSEMBLE_H

#include "vine_mpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_MPC_ENSEMBLE_ABI_VERSION 1
#define VINE_MPC_ENSEMBLE_MAX_MEMBERS 16
#define VINE_MPC_RISK_MEAN 0
#define VINE_MPC_RISK_MAX 1
#define VINE_MPC_RISK_ENTROPIC 2

typedef struct VineMpcEnsembleConfig {
    int32_t abi_version;   /* must be VINE_MPC_ENSEMBLE_ABI_VERSION */
    int32_t members;       /* E; 1 .. VINE_MPC_ENSEMBLE_MAX_MEMBERS, a divisor of the VineMpcConfig's samples; default 4 */
    int32_t risk;          /* VINE_MPC_RISK_*; default VINE_MPC_RISK_MEAN */
    double theta;          /* with VINE_MPC_RISK_ENTROPIC: > 0, finite; default 1 */
} VineMpcEnsembleConfig;

int vine_mpc_ensemble_config_default(VineMpcEnsembleConfig* ecfg);
int vine_mpc_ensemble_config_size(void);    /* sizeof(VineMpcEnsembleConfig): checked by the ctypes mirror */

/* The launch behind the fork and behind every base node (see 1. THE NODE).  nominal, tick, window: the controller's, read
 * only; actions: device float[N, 2], the model handle's action buffer. */
int vine_mpc_ensemble_scheduled(VineHandle* model, const VineMpcConfig* cfg, const VineMpcEnsembleConfig* ecfg,
                                const float* nominal, const int64_t* tick, const int64_t* window, float* actions, void* stream);

/* In place of vine_mpc_update (see 2. THE UPDATE); its arguments, and group_cost: device double[M * G] or NULL. */
int vine_mpc_ensemble_update(VineHandle* model, const VineMpcConfig* cfg, const VineMpcEnsembleConfig* ecfg, const double* cost,
                             const int64_t* plant_reset, float* nominal, float* history, int64_t* tick, float* plant_actions,
                             double* weights, double* group_cost, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_MPC_ENSEMBLE_H */
