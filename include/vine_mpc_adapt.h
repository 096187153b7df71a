/*
 * vine_mpc_adapt.h — C ABI of online model adaptation for the predictive controller of vine_mpc.h, for MI355X (gfx950): every
 * few control steps the K samples of each plant become K candidate plants drawn around that plant's current belief, are put
 * back onto the plant's state of a few steps ago, fed the actions the plant received and scored against what the plant did;
 * the belief moves to the weighted mean and the planner plans with it from then on.  All of it on the device.
 *
 * Only libvine_hip.so exports this header.  Errors, streams and ownership as in vine.h and vine_mpc.h: 0 = ok, negative =
 * VineStatus, message via vine_last_error(); every entry point enqueues on the caller's stream and does not synchronise,
 * allocates nothing and uses no atomics; the caller owns every buffer.  Neither the step kernels nor the three launches of
 * vine_mpc.h are touched.  Nothing that changes from step to step is a kernel argument, so all five launches replay from a
 * captured hipGraph.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * HANDLES.  The PLANT handle (M envs) and the MODEL handle (N = M * K envs, env p * K + j = sample j of plant p) of
 * vine_mpc.h.  The model handle must have a per-env parameter table bound (vine_bind_env_params): that table is what is
 * adapted, and vine_mpc_adapt_pin and vine_mpc_adapt_estimate WRITE its rows.  A model handle without one is refused
 * (VINE_ERR_UNSUPPORTED).
 *
 * DIMENSIONS.  The belief has D dimensions.  A dimension {first_row, num_rows, lo, hi, std_floor} is either one scalar row of
 * the VP_* table (num_rows = 1; the value is the row's) or one FPAM vector (num_rows = 5, first_row one of VP_FPAM_K0,
 * VP_FPAM_C0, VP_FPAM_b0, VP_FPAM_B0; the value is a factor on the model configuration's five constants cfg->base_rows, as in
 * the ENV_PARAMS spec).  Refused by name:
 *   ACTION_DELAY                         (VINE_ERR_UNSUPPORTED) an integer: its belief is not Gaussian and a weighted mean of
 *                                        delays is no delay;
 *   CART_MASS, LINK_MASS, TIP_LINK_MASS  they live in the inertia table (vine_env_inertia.h), whose derived rows need the
 *                                        composites formed in double on the host; they are no row of this table at all, so a
 *                                        descriptor cannot name them: utils/mpc_adapt.py adapt_config refuses the names.
 * Overlapping dimensions are refused (VINE_ERR_INVALID_ARG).
 *
 * ADAPTATION STATE.  All the caller's, on the handles' device:
 *   mean[M][D], std[M][D]                 float64   the belief
 *   prior_mean[M][D], prior_std[M][D]     float64   what the belief returns to when it forgets
 *   passes[M]                             int64     estimates done per plant: the counter of the candidates' stream
 *   anchor_state[VF_COUNT][M]             float32   the plants' state block at the anchor
 *   anchor_history[M][VINE_MAX_DELAY][2]  float32   the controller's history at the anchor
 *   anchor_progress[M], anchor_count[1]   int64     the plants' progress, the PLANT handle's step count at the anchor
 *   trace_actions[M][W][2]                float32   the action each traced plant step consumed
 *   trace_rows[M][W][12]                  float32   VF_Q0 .. VF_Q0 + 5 and VF_QD0 .. VF_QD0 + 5 behind each traced step
 *   trace_len[M]                          int32
 *   trace_open[M], episode_ended[M]       uint8
 *   err[N]                                float64
 *   alive[N]                              uint8
 *   window[1]                             int64
 *
 * CANDIDATES.  The value of sample e = p * K + j in dimension d during pass passes[p] is
 *   theta = min(max(mean[p][d] + (double)z * std[p][d], lo_d), hi_d)
 * formed in float64: one multiply, one add, no contraction.  z = float32((double)zi * K0), zi = 2 S - 524280 with S the
 * integer sum of the eight 16-bit halves of one Philox-4x32-10 call (the deviate of vine_mpc.h) and
 * K0 = 1 / sqrt(32 * (65536^2 - 1) / 12) in float64.  The call's counter is
 *   (p * K + j, (unsigned)passes[p], VINE_MPC_ADAPT_RNG | (passes[p] >> 32) << 8, d)
 * and its key the two words of cfg->seed.  Purpose word 9 is the next free one: the step kernels' own stop at 4, the sensor
 * has 5 and 6, the push 7, the controller's noise 8.  Candidate 0 of every plant has z = 0: the current belief is always among
 * the candidates.  The table value is float32(theta) for a scalar row and float32((double)base_row * theta) for each FPAM row,
 * the rounding of env_params.set_rows.  theta is a pure function of (seed, p, j, passes[p], d, mean, std) and is never
 * stored: the pin and the estimate each recompute it.
 *
 * A CYCLE is: anchor, E x (one control step of vine_mpc.h + the trace node), pin, W x (model step + score node), estimate.
 *
 * 1. THE ANCHOR.  vine_mpc_adapt_anchor, one lane per plant, in front of the cycle's first control step.  It copies plant p's
 * state-block column to anchor_state, history[p] to anchor_history[p], the plant's progress to anchor_progress[p], writes the
 * PLANT handle's step count to anchor_count[0], and sets trace_len[p] = 0, trace_open[p] = (plant_reset[p] == 0),
 * episode_ended[p] = 0.  A plant whose next step only consumes a reset is not traced this cycle: its samples would not stay
 * the plant.
 *
 * 2. THE TRACE NODE.  vine_mpc_adapt_trace, one lane per plant, behind every plant step.  s = plant step count -
 * anchor_count[0].  For 1 <= s <= W and trace_open[p]: trace_actions[p][s - 1] = plant_actions[p] (what that step consumed),
 * trace_rows[p][s - 1] = the plant's twelve joint fields, trace_len[p] = s; if the step raised plant_reset[p] the trace closes
 * after that row is stored (the step that ends an episode is still a valid row).  At every s >= 1 a raised reset sets
 * episode_ended[p], and, where `returns` is given, returns[p] += (double)plant_rew[p].
 *
 * 3. THE PIN.  vine_mpc_adapt_pin, one lane per model env.  The lane first writes its candidate rows into the model's bound
 * table, then copies every field of anchor_state's column p but the delay ring, sets progress[e] = anchor_progress[p] and
 * rebuilds the ring from anchor_history[p] as vine_mpc_fork does from history[p] (csrc/vine_mpc_shared.h states both once),
 * with the sample's own delay and RAIL_VELOCITY_SCALE read from the table AFTER the candidate rows were written -- that row
 * may itself be a dimension.  Then actions[e] = trace_actions[p][0], rew[e] = 0, reset[e] = 0, err[e] = 0, alive[e] = 1 and
 * window[0] = the MODEL handle's step count.  Table rows outside the dimensions are not touched.
 *
 * 4. THE SCORE NODE.  vine_mpc_adapt_scheduled, one lane per model env, behind each of the W model steps that follow.
 * k = model step count - window[0].  Outside 1 .. W the launch touches nothing.  For 1 <= k <= trace_len[p] and alive[e]:
 *   a compared value (a field with a non-zero weight) that is not finite: err[e] = +inf, alive[e] = 0;
 *   else err[e] += sum_f (double)w_f * ((double)x_f - (double)trace_rows[p][k - 1][f])^2, the sum over the weighted fields in
 *   order formed first and added once (the statement of vine_sysid.h); and if the candidate raised reset[e] at k <
 *   trace_len[p] it left the episode before the plant did: err[e] = +inf, alive[e] = 0, after the addition.
 * While trace_len[p] > 0 every sample, alive or not, gets actions[e] = trace_actions[p][min(k, trace_len[p] - 1)].
 *
 * 5. THE ESTIMATE.  vine_mpc_adapt_estimate, one workgroup of VINE_MPC_THREADS lanes per plant, the reduction order of
 * vine_mpc_update (lane t goes through j = t, t + 256, .. in ascending j; a butterfly over each wave; the four wave values
 * through LDS, combined in wave order), so two runs give the same bits.  mean[p] and std[p] are read into LDS before anything
 * is written.
 *   If cfg->forget_on_reset and episode_ended[p]: mean[p] = prior_mean[p], std[p] = prior_std[p] (the plant may have been
 *   redrawn).
 *   Else if trace_len[p] < min_steps or no err of the plant is finite: the belief is unchanged.
 *   Else beta = min err, ebar = the mean of the finite errs (their sum in the order above over their count),
 *   tau = temperature * (ebar - beta), w_j = exp(-(err_j - beta) / tau) where tau > 0 and 1 otherwise, for a finite err_j; 0
 *   for +inf;  m_d = sum w theta / sum w;  v_d = sum w (theta - m_d)^2 / sum w;
 *   mean <- (1 - rate) mean + rate m;  std <- max((1 - rate) std + rate sqrt(v), std_floor).
 * In every case the planning value -- the candidates' statement at z = 0 on the new mean, in the candidates' rounding -- is
 * then written into the table rows of all K samples of p, and passes[p] += 1.  Where `weights` is given, w_j of every sample
 * is stored too (0 where the belief was not estimated): a diagnostic, nothing reads it back.
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_MPC_ADAPT_H
#define VINE_MPC_ADAPT_H

#include <stdint.h>

#include "vine.h"
#include "vine_mpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_MPC_ADAPT_ABI_VERSION 1
#define VINE_MPC_ADAPT_MAX_WINDOW 32
#define VINE_MPC_ADAPT_MAX_DIMS 8
#define VINE_MPC_ADAPT_FIELDS 12        /* q0..5 and qd0..5 */
#define VINE_MPC_ADAPT_BASE_ROWS 20     /* the four FPAM vectors: table rows VP_FPAM_K0 .. VP_COUNT - 1 */
#define VINE_MPC_ADAPT_RNG 9u           /* the purpose word of the candidates' stream */

typedef struct VineMpcAdaptDim {
    int32_t first_row;     /* a VP_* row */
    int32_t num_rows;      /* 1: that scalar row; 5: the FPAM vector that starts there */
    double lo;             /* lo <= hi, both finite */
    double hi;
    double std_floor;      /* >= 0, finite */
} VineMpcAdaptDim;

typedef struct VineMpcAdaptConfig {
    int32_t abi_version;       /* must be VINE_MPC_ADAPT_ABI_VERSION */
    int32_t num_plants;        /* M; >= 1; the caller sets it (default 0) */
    int32_t samples;           /* K; >= 2; default 256 */
    int32_t window;            /* W; 1 .. VINE_MPC_ADAPT_MAX_WINDOW; default 8 */
    int32_t every;             /* E; control steps per cycle; >= W; default 8 */
    int32_t num_dims;          /* D; 1 .. VINE_MPC_ADAPT_MAX_DIMS; the caller sets it (default 0) */
    int32_t min_steps;         /* 1 .. W; default 4 */
    int32_t forget_on_reset;   /* 0 or 1; default 0 */
    double temperature;        /* > 0, finite; default 0.1 */
    double rate;               /* 0 < rate <= 1; default 0.5 */
    uint64_t seed;             /* key of the candidates' stream; default 0 */
    float weights[VINE_MPC_ADAPT_FIELDS];        /* >= 0, finite; default 1 on the six q, 0 on the six qd */
    float base_rows[VINE_MPC_ADAPT_BASE_ROWS];   /* the MODEL configuration's vine_env_params_row()[VP_FPAM_K0 ..]; finite */
    VineMpcAdaptDim dims[VINE_MPC_ADAPT_MAX_DIMS];
} VineMpcAdaptConfig;

int vine_mpc_adapt_config_default(VineMpcAdaptConfig* cfg);
int vine_mpc_adapt_config_size(void);    /* sizeof(VineMpcAdaptConfig): checked by the ctypes mirror */

/* See 1. THE ANCHOR.  plant_progress, plant_reset: the plant handle's step buffers, int64[M]; history: the controller's. */
int vine_mpc_adapt_anchor(VineHandle* plant, const VineMpcAdaptConfig* cfg, const int64_t* plant_progress,
                          const int64_t* plant_reset, const float* history, float* anchor_state, float* anchor_history,
                          int64_t* anchor_progress, int64_t* anchor_count, int32_t* trace_len, uint8_t* trace_open,
                          uint8_t* episode_ended, void* stream);

/* See 2. THE TRACE NODE.  plant_actions: float[M, 2], what the step just done consumed; plant_rew: float[M], the plant
 * handle's reward buffer; returns: double[M] or NULL. */
int vine_mpc_adapt_trace(VineHandle* plant, const VineMpcAdaptConfig* cfg, const float* plant_actions,
                         const int64_t* plant_reset, const float* plant_rew, const int64_t* anchor_count, float* trace_actions,
                         float* trace_rows, int32_t* trace_len, uint8_t* trace_open, uint8_t* episode_ended, double* returns,
                         void* stream);

/* See 3. THE PIN.  actions: float[N, 2], 8-byte aligned; rew, reset, progress: the MODEL handle's step buffers. */
int vine_mpc_adapt_pin(VineHandle* model, const VineMpcAdaptConfig* cfg, const double* mean, const double* std,
                       const int64_t* passes, const float* anchor_state, const float* anchor_history,
                       const int64_t* anchor_progress, const float* trace_actions, float* actions, float* rew, int64_t* reset,
                       int64_t* progress, double* err, uint8_t* alive, int64_t* window, void* stream);

/* See 4. THE SCORE NODE.  reset: the MODEL handle's reset buffer. */
int vine_mpc_adapt_scheduled(VineHandle* model, const VineMpcAdaptConfig* cfg, const float* trace_actions,
                             const float* trace_rows, const int32_t* trace_len, const int64_t* window, float* actions,
                             const int64_t* reset, double* err, uint8_t* alive, void* stream);

/* See 5. THE ESTIMATE.  weights: double[N] or NULL. */
int vine_mpc_adapt_estimate(VineHandle* model, const VineMpcAdaptConfig* cfg, const double* err, const int32_t* trace_len,
                            const uint8_t* episode_ended, double* mean, double* std, const double* prior_mean,
                            const double* prior_std, int64_t* passes, double* weights, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_MPC_ADAPT_H */
