/*
 * vine_mpc_noise.h — the predictive controller's sample distribution (MPC_NOISE; product library only): perturbations that are
 * correlated over the horizon, and an amplitude per plant that follows the spread of the samples the weights preferred.
 *
 * include/vine_mpc.h draws every sample's perturbation white: independent at every horizon step, with one amplitude sigma[a]
 * for all plants and the whole run.  Every command of this plant passes a first-order low-pass and a delay ring before it
 * moves the chain, so a white perturbation is mostly filtered away.  This header replaces the perturbation and nothing else:
 * the fork, the node and the step kernels are not touched, vine_mpc.hip is not edited.  Three launches are added around the
 * base controller's: a table of perturbations is drawn in front of the fork, a launch behind the fork and behind every base
 * node overwrites the white action the base launch left, and an update that reads the table takes vine_mpc_update's place.
 *
 * Errors, streams and ownership as in vine_mpc.h: every entry point enqueues on the caller's stream and does not synchronise,
 * allocates nothing and uses no atomics; the caller owns every buffer; M = num_plants, K = samples, H = horizon, N = M * K of
 * the VineMpcConfig passed beside the VineMpcNoiseConfig.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * CONTROLLER STATE, beside that of include/vine_mpc.h.  The caller's, on the handles' device:
 *   eps[H][N][2]     float32   the perturbation of sample e = p * K + j at horizon step k, component a, in units of the base
 *                              deviate (not yet scaled).  k is the outermost index: the draw, the node and the update all
 *                              touch 64 consecutive samples of one k per wave.
 *   sigma_p[M][2]    float32   the amplitude of plant p; the caller initialises it to cfg->sigma
 *
 * THE CONFIGURATION.  VineMpcNoiseConfig:
 *   beta[a]        the correlation of successive horizon steps, in [0, 1); 0: white, the words of include/vine_mpc.h
 *   adapt          0: sigma_p is read and never written; otherwise the update adapts it
 *   rate           with adapt: the weight of the new estimate, in (0, 1]
 *   sigma_min[a], sigma_max[a]    the bounds sigma_p[p][a] is clamped to; sigma_min[a] <= cfg->sigma[a] <= sigma_max[a]
 * Refused with VINE_ERR_INVALID_ARG, vine_last_error() naming the field: a beta outside [0, 1) or not finite; with adapt, a
 * rate outside (0, 1] (or not finite); a sigma_min below 0 or not finite; a sigma_max not finite; a setting where
 * sigma_min[a] <= cfg->sigma[a] <= sigma_max[a] does not hold.  Every entry point also refuses what vine_mpc.hip refuses of
 * the VineMpcConfig, null arguments, float2 buffers that are not 8-byte aligned, and a model handle without N = M * K envs,
 * in vine_mpc.hip's words.
 *
 * 1. THE DRAW.  vine_mpc_noise_draw, enqueued once per control step in front of vine_mpc_fork; one lane per (sample,
 * component).  For sample e = p * K + j and component a:
 *   z_k    = the base deviate of include/vine_mpc.h, NOISE, under the same counter and key:
 *            (e, (unsigned)tick[p], VINE_MPC_RNG_NOISE | (tick[p] >> 32) << 8, 2 k + a), the two words of cfg->seed
 *   eps[0] = z_0
 *   eps[k] = fl32(fl32(b_a * eps[k - 1]) + fl32(g_a * z_k)),   k = 1 .. H - 1
 *   b_a    = beta[a];   g_a = float32(sqrt(1 - (double)b_a * (double)b_a)), formed on the host
 * two float32 multiplies and one float32 add, no contraction.  Sample 0 of every plant is all zeros.  The stationary variance
 * is the base deviate's (eps[0] has it, and b^2 + g^2 = 1 keeps it); the correlation of eps[k] and eps[k + 1] is b_a.  With
 * beta = 0 the table holds the base deviate's words exactly: 0 * x + 1 * z is z in every bit.
 *
 * 2. THE NODE.  vine_mpc_noise_scheduled, one lane per model env, enqueued once behind vine_mpc_fork and once behind every
 * vine_mpc_scheduled of the horizon on the same stream.  It reads the MODEL handle's step count c as every observer reads it;
 * k = c - window[0].  For 0 <= k < H every sample, alive or not, gets
 *   actions[e][a] = u'[j][k][a] = clamp(nominal[p][k][a] + eps[k][e][a] * c_p[a], +-clip_actions of the MODEL handle)
 *   c_p[a]        = float32((double)sigma_p[p][a] * K0), formed on the device; K0 of include/vine_mpc.h in float64
 * one float32 multiply, one float32 add, no contraction.  Outside that window the launch touches nothing.  Nothing that
 * changes from step to step is a kernel argument, so a captured launch replays correctly.  The base fork and node stay in the
 * chain unchanged -- the state copy, the ring rebuild and the cost sums are theirs -- and this launch overwrites the white
 * action they left.  With beta = 0 and sigma_p = cfg->sigma it stores the words that were there.
 *
 * 3. THE UPDATE.  vine_mpc_noise_update, in place of vine_mpc_update: the statement of include/vine_mpc.h, THE UPDATE, word for
 * word -- beta, the float64 weights, new = float32(sum w u / sum w), the branch without a finite cost, the reset branch, the
 * shift, the history and the tick; one workgroup of VINE_MPC_THREADS lanes per plant; the same fixed reduction order; the
 * optional weights output -- with u' of step 2, read from eps and sigma_p, in the place of u.
 * With adapt it also forms, per component a,
 *   q_a = sum_j sum_k w_j * (d * d),   d = (double)u'[j][k][a] - (double)nominal[p][k][a]     (after the clamp)
 * accumulated per lane in the order of that loop (k outer, j ascending), then combined over the wave and in wave order like
 * the other sums, and
 *   v_a           = q_a / (sum_j w_j * H)
 *   sigma_p[p][a] = float32(clamp(sqrt((1 - rate) * s * s + rate * v_a), sigma_min[a], sigma_max[a])),   s = (double)sigma_p[p][a]
 * the weighted mean square of the perturbations the weights preferred, mixed into the old variance.  A plant whose reset is
 * consumed (plant_reset[p] != 0) gets sigma_p[p] = cfg->sigma; otherwise, where no cost is finite, sigma_p[p] keeps its bits.
 * Without adapt sigma_p is never written.  nominal[p] is the sequence as it stood before the launch.
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_MPC_NOISE_H
#define VINE_MPC_NOISE_H

#include "vine_mpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_MPC_NOISE_ABI_VERSION 1
#define VINE_MPC_NOISE_THREADS 256

typedef struct VineMpcNoiseConfig {
    int32_t abi_version;   /* must be VINE_MPC_NOISE_ABI_VERSION */
    float beta[2];         /* correlation of successive horizon steps per action component; in [0, 1); default 0 */
    int32_t adapt;         /* 0: sigma_p is fixed; otherwise the update adapts it; default 0 */
    double rate;           /* with adapt: in (0, 1]; default 0.2 */
    float sigma_min[2];    /* >= 0, finite; default 0 */
    float sigma_max[2];    /* finite; default FLT_MAX: every sigma of a VineMpcConfig lies inside the default bounds */
} VineMpcNoiseConfig;

int vine_mpc_noise_config_default(VineMpcNoiseConfig* ncfg);
int vine_mpc_noise_config_size(void);    /* sizeof(VineMpcNoiseConfig): checked by the ctypes mirror */

/* Fill the table (see 1. THE DRAW).  tick: the controller's, int64[M], read only; eps: device float[H, N, 2], 8-byte aligned. */
int vine_mpc_noise_draw(VineHandle* model, const VineMpcConfig* cfg, const VineMpcNoiseConfig* ncfg, const int64_t* tick,
                        float* eps, void* stream);

/* The launch behind the fork and behind every base node (see 2. THE NODE).  nominal, window: the controller's, read only;
 * eps, sigma_p: read only; actions: device float[N, 2], the model handle's action buffer. */
int vine_mpc_noise_scheduled(VineHandle* model, const VineMpcConfig* cfg, const VineMpcNoiseConfig* ncfg, const float* nominal,
                             const int64_t* window, const float* eps, const float* sigma_p, float* actions, void* stream);

/* In place of vine_mpc_update (see 3. THE UPDATE); its arguments, and eps (read only) and sigma_p (device float[M, 2], written
 * with adapt only). */
int vine_mpc_noise_update(VineHandle* model, const VineMpcConfig* cfg, const VineMpcNoiseConfig* ncfg, const double* cost,
                          const int64_t* plant_reset, const float* eps, float* nominal, float* history, int64_t* tick,
                          float* plant_actions, float* sigma_p, double* weights, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_MPC_NOISE_H */
