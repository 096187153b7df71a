/*
 * vine_mpc_policy.h — C ABI of policy-guided MPC for MI355X (gfx950): every sample of include/vine_mpc.h rolls the trained
 * policy closed-loop on its own model state, the controller's sequence is a RESIDUAL on the policy's mean, and the critic may
 * close the horizon.  With sigma = 0 and a zero residual the controller is the policy; with a useless policy it is still a
 * planner.
 *
 * Only libvine_hip.so exports this header.  Errors, streams and ownership as in vine.h and vine_mpc.h: 0 = ok, negative =
 * VineStatus, message via vine_last_error(); every entry point enqueues on the caller's stream and does not synchronise,
 * allocates nothing and uses no atomics; the caller owns every buffer.  Nothing that changes between replays of a captured
 * hipGraph is a kernel argument: the horizon step is k = (MODEL handle's step count) - window[0], read on the device, with
 * window[0] as vine_mpc_fork left it.  vine_mpc_fork, vine_mpc_scheduled and vine_mpc_update are used as they are.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * THE CONTROL STEP.  M plants, K samples, H horizon, N = M * K, env e = p * K + j (include/vine_mpc.h).  nominal[M][H][2] is
 * now the residual; what the fork and the node write into the model's action buffer, d = clamp(nominal + z c, +-clip), is a
 * perturbation that vine_mpc_policy_act turns into an action just before each model step:
 *
 *   vine_mpc_fork                      state columns, ring from history, cost = 0, actions = d[j][0]
 *   vine_mpc_policy_fork               plant observation and plant LSTM state -> the K samples of each plant
 *   for k = 0 .. H - 1:
 *       the policy's trunk on the model's observation buffer, N rows, LSTM state committed  (vine_ppo.h: the split MLP and
 *                                                                                             the split LSTM step)
 *       vine_mpc_policy_act            actions[e] = clamp(mu_e + actions[e], +-clip);  at k == 0 also THE KEEP
 *       vine_step of the model handle
 *       vine_mpc_scheduled             cost, alive, actions = d[j][k + 1]
 *   [terminal_value != 0:  the trunk once more, LSTM state NOT committed;  vine_mpc_policy_terminal]
 *   vine_mpc_update                    on the residual; writes the residual's first entry to plant_actions / history[p][0]
 *   vine_mpc_policy_compose            plant_actions = clamp(mu0 + residual), history[p][0] = the same
 *   vine_step of the plant handle
 *
 * THE NETWORK.  The default one: LSTM of VINE_MPC_POLICY_UNITS = 256 units with a LayerNorm behind it, two actions, one
 * value.  y [N][256] float32 is the LSTM output (the h state the trunk returns); hw [3][256] and hc [3] are
 * vine_rollout_head_prep's products (vine_ppo.h): the LayerNorm folded into the rows mu_0, mu_1, value.  The head of row e is
 * quad_ln_heads<3> of csrc/vine_policy_head.h, the function the four-lanes-per-env step kernel calls: one quad of lanes per
 * model env, lane t holding units {16 i + 4 t .. + 3 : i < 16}; out[r] = rstd * (hw[r] . (y - mean)) + hc[r].
 * N must be a multiple of 512 (the trunk's kernels' shape), else VINE_ERR_INVALID_ARG.
 *
 * CONTROLLER STATE, beyond vine_mpc.h's.  All the caller's, on the handles' device:
 *   plant_h[M][256], plant_c[M][256]  float32   the policy's LSTM state per plant
 *   mu0[M][2]                         float32   the policy's mean on the plant's observation, this control step
 *
 * THE FORK.  vine_mpc_policy_fork, one quad per model env e of plant p:
 *   row p of the plant's observation buffer -> row e of the model's observation buffer (obs_width floats; this is what the
 *     plant's step and its observers left, so a sensor model on the plant shows);
 *   plant_h[p] -> row e of h_state and row e of the operand copy of h (h_op, rows h_op_stride floats apart, as
 *     quad_clear_lstm_rows of csrc/vine_policy_head.h takes them);
 *   plant_c[p] -> row e of c_state.
 * Nothing else is written: columns of the operand buffer in front of h_op, and rows beyond N, stay.
 * Refused: a plant or model row width that differs from cfg->obs_width (VINE_ERR_INVALID_ARG, "observation width").
 *
 * THE ACT.  vine_mpc_policy_act, one quad per model env, 0 <= k < H (outside: the launch touches nothing):
 *   (mu_e[0], mu_e[1], v) = the head of row e of y;
 *   actions[e][a] = clamp(mu_e[a] + actions[e][a], +-clip_actions of the MODEL handle)      one float32 add, the step's clamp.
 * No inner clamp is applied to mu, so a model handle with clip_actions > 1 is refused (VINE_ERR_UNSUPPORTED), as the device
 * player refuses it.  mu_out (optional) receives mu_e for every env: a diagnostic, nothing reads it back.
 * THE KEEP.  When k == 0 the quad of sample 0 of each plant p also writes
 *   mu0[p] = mu_e;  plant_h[p] = row e of h_state;  plant_c[p] = row e of c_state
 * -- the policy's state after seeing the plant's observation; all K rows are equal there.  If plant_reset[p] (the plant
 * handle's reset buffer) is raised, zeros are written to all three instead: the plant's next step only consumes the reset,
 * and the policy starts the new episode from zero state.
 *
 * THE TERMINAL VALUE.  vine_mpc_policy_terminal, same layout, k == H only (else the launch touches nothing):
 *   V_e = the value row of the head; un-normalised when value_mean / value_var (the value normaliser's float64 statistics,
 *         both or neither) are given: clamp(v, +-5) * sqrt(float(var) + value_eps) + float(mean)  (unnormalize_value) -- a
 *         row that is not finite stays as it is (the clamp would turn a NaN into -5);
 *   for a sample with alive[e]:  cost[e] = cost[e] - terminal_value * (double)V_e   one float64 multiply, one subtract;
 *   a non-finite V_e: cost[e] = +inf, alive[e] = 0.  A sample that is not alive is not touched.
 * value_out (optional) receives V_e of every env.
 *
 * THE COMPOSITION.  vine_mpc_policy_compose, one lane per plant, behind vine_mpc_update:
 *   plant_reset[p] raised: nothing changes (the update wrote (0, 0));
 *   else a = clamp(mu0[p] + plant_actions[p], +-clip_actions of the MODEL handle) goes to plant_actions[p] and history[p][0]:
 *   the history holds what the plant really received, and the next fork rebuilds the delay ring from it.
 *
 * REFUSALS common to the entry points, each by name: a NULL or mismatching configuration, obs_width outside
 * 1 .. VINE_MAX_OBS, ln_eps or value_eps not finite or negative, terminal_value not finite or negative, a NULL argument,
 * row pointers that are not 16-byte aligned (y, hw, h_state, c_state, h_op, plant_h, plant_c; h_op_stride a multiple of 4
 * and at least 256) or pair pointers that are not 8-byte aligned (actions, mu0, mu_out, plant_actions, history),
 * N != M * K, N not a multiple of 512.
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_MPC_POLICY_H
#define VINE_MPC_POLICY_H

#include <stdint.h>

#include "vine.h"
#include "vine_mpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_MPC_POLICY_ABI_VERSION 1
#define VINE_MPC_POLICY_UNITS 256       /* the LSTM's width: the one quad_ln_heads serves */
#define VINE_MPC_POLICY_ROWS 512        /* N must be a multiple of it */

typedef struct VineMpcPolicyConfig {
    int32_t abi_version;     /* must be VINE_MPC_POLICY_ABI_VERSION */
    int32_t obs_width;       /* columns of both observation buffers; 1 .. VINE_MAX_OBS; the caller sets it (default 0) */
    float ln_eps;            /* the LayerNorm's eps; >= 0, finite; default 1e-5 */
    float value_eps;         /* the value normaliser's eps; >= 0, finite; default 1e-5 */
    double terminal_value;   /* weight w of the critic's value behind the horizon; >= 0, finite; default 0 */
} VineMpcPolicyConfig;

int vine_mpc_policy_config_default(VineMpcPolicyConfig* pcfg);
int vine_mpc_policy_config_size(void);          /* sizeof(VineMpcPolicyConfig): checked by the ctypes mirror */

/* See THE FORK.  plant_obs float[M, plant_obs_width], model_obs float[N, model_obs_width]; h_state, c_state float[N, 256];
 * h_op: address of column 0 of the operand copy of h in row 0. */
int vine_mpc_policy_fork(VineHandle* plant, VineHandle* model, const VineMpcConfig* cfg, const VineMpcPolicyConfig* pcfg,
                         const float* plant_obs, int32_t plant_obs_width, float* model_obs, int32_t model_obs_width,
                         const float* plant_h, const float* plant_c, float* h_state, float* c_state, float* h_op,
                         int64_t h_op_stride, void* stream);

/* See THE ACT and THE KEEP.  window: vine_mpc_fork's; plant_reset: the plant handle's reset buffer, int64[M];
 * mu_out: device float[N, 2] or NULL. */
int vine_mpc_policy_act(VineHandle* model, const VineMpcConfig* cfg, const VineMpcPolicyConfig* pcfg, const float* y,
                        const float* hw, const float* hc, const int64_t* window, const int64_t* plant_reset,
                        const float* h_state, const float* c_state, float* actions, float* mu0, float* plant_h,
                        float* plant_c, float* mu_out, void* stream);

/* See THE TERMINAL VALUE.  value_mean, value_var: device double[1] each, or both NULL; value_out: device float[N] or NULL. */
int vine_mpc_policy_terminal(VineHandle* model, const VineMpcConfig* cfg, const VineMpcPolicyConfig* pcfg, const float* y,
                             const float* hw, const float* hc, const double* value_mean, const double* value_var,
                             const int64_t* window, double* cost, uint8_t* alive, float* value_out, void* stream);

/* See THE COMPOSITION. */
int vine_mpc_policy_compose(VineHandle* model, const VineMpcConfig* cfg, const VineMpcPolicyConfig* pcfg, const float* mu0,
                            const int64_t* plant_reset, float* plant_actions, float* history, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_MPC_POLICY_H */
