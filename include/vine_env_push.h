/*
 * vine_env_push.h — external disturbances (ENV_PUSH; product library only): per-env random impulses on the chain, applied on
 * the device.
 *
 * vine_env_push_scheduled is a launch behind every step (a step observer, like vine_env_sensor_scheduled) that, for the envs
 * a draw selects, adds to the six generalised velocities of the state block what an instantaneous impulse P (N s, in the
 * vine's y-z plane) at a point of the chain does to them: dqd = M(q)^-1 J^T P, with the mass matrix the step itself uses.
 * An impulse moves nothing: positions, body fields, the observation the step has just written, rewards, flags and progress
 * keep every bit; the policy sees the push one step later, as it would on the robot.  The step kernels are not touched.
 *
 * PER-ENV VALUES.  Env e with global id g = env_id_offset + e runs episode k with two values, held in the device table
 * push[VPU_NAMES][N] (float32): RATE (probability per control step that the env is pushed, [0, 1]) and IMPULSE (largest
 * impulse component, N s, >= 0).  Each is the draw of include/vine_env_redraw.h (`redraw_value`) under the name keys of
 * "PUSH_RATE" and "PUSH_IMPULSE": a pure function of (seed, key, g, k), formed in float64 and rounded once to float32.
 * Episode 0's table is built by the host.  With per_episode, a lane that sees reset[e] != 0 behind a step increments
 * episode_index[e] and writes the two values of the new k: the moment the redraw and the sensor act, so with several of them
 * on their ordinals are equal.  Envs reset from outside the step keep their values and ordinal.
 *
 * POINTS.  Point 0 is the cart; point m (1 .. 5) is the distal end of link m - 1; point 5 is the tip.
 *
 * Behind the step with index s (s = steps completed - 1), for env e with values (p, I):
 *   1. one Philox-4x32-10 call keyed as the step kernels and the sensor key theirs: counter
 *      (g, s, VINE_PUSH_RNG | (s >> 32) << 8, 0), key = the seed's words; it gives the words w0 .. w3.
 *   2. the env is pushed iff reset[e] == 0 and u < p (float32), u = (w3 >> 8) * 2^-24.  An env whose reset flag the step
 *      has just raised is never pushed: its state is about to be replaced.
 *   3. a_y = float32((w0 >> 8) * 2^-23) - 1.0f, a_z likewise from w1 (both exact in float32, in [-1, 1));
 *      P_y = I * a_y, P_z = I * a_z (one float32 multiply each).
 *   4. the point is points[((w2 >> 8) * num_points) >> 24], in integer arithmetic.
 *   5. the generalised impulse in the absolute coordinates (ydot, w_1 .. w_5), th_i = q_1 + .. + q_{i+1}, phi_i = phi0 + th_i,
 *      sin phi_i = s0 cos th_i + c0 sin th_i, cos phi_i = c0 cos th_i - s0 sin th_i:
 *          Q_0 = P_y;   Q_{i+1} = -L (cos phi_i P_y + sin phi_i P_z) for links i < m, else 0.
 *   6. M_00 = mtot, M_0,i+1 = -b_i cos phi_i, M_i+1,j+1 = a_ij cos(th_i - th_j) (a_ii = ADIAG_i, a_ij = AOFF_max(i,j); AOFF_0
 *      never occurs), the composites of the env's column of the bound inertia table, or the configuration's own derived rows
 *      (VineEnvPushSpec.composites) where none is bound.  D = M^-1 Q by a Cholesky factorisation M = G G^T, row by row, a
 *      forward and a backward substitution.  Back to the relative coordinates: dqd_0 = D_0, dqd_1 = D_1, dqd_{k+1} = D_{k+1} - D_k.
 *   7. state[VF_QD0 + k][e] = qd_k + dqd_k for k = 0 .. 5, and push_count[e] += 1.  Where I == 0 the impulse is zero and the
 *      six velocities are not stored (qd + 0 would turn a -0 into +0); the env still counts as pushed.
 * Nothing else of the state block is ever written, and nothing at all for an env that is not pushed (but, per episode, the
 * two table entries and the ordinal of a flagged env).  All arithmetic of 3 to 7 is float32, without contraction.
 *
 * The kernel: one lane per env, 256 lanes per workgroup, no LDS, no atomics; a lane is the only writer of its env's six
 * velocities, table entries, ordinal and count.
 */
#ifndef VINE_ENV_PUSH_H
#define VINE_ENV_PUSH_H

#include "vine_env_redraw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_ENV_PUSH_ABI_VERSION 1
#define VINE_ENV_PUSH_THREADS 256
#define VINE_PUSH_MAX_POINTS 6
#define VINE_PUSH_COMPOSITES 20                         /* = VI_COUNT - VI_MTOT: the derived rows of vine_env_inertia.h */
/* The purpose word of the Philox stream; the step kernels' own stop at 4 (vine_hip.hip), the sensor uses 5 and 6. */
#define VINE_PUSH_RNG 7u

/* The names of a spec and the rows of the push table, in this order (the mixed radix of value lists counts in it too). */
typedef enum VineEnvPushSlot { VPU_RATE = 0, VPU_IMPULSE, VPU_NAMES = 2 } VineEnvPushSlot;

typedef struct VineEnvPushSpec {
    int32_t abi_version;            /* VINE_ENV_PUSH_ABI_VERSION */
    int32_t num_values;             /* doubles in the values array */
    uint64_t seed;
    const double* values;           /* DEVICE array of the value lists, the caller's; may be NULL when num_values == 0 */
    VineEnvRedrawName name[VPU_NAMES];      /* both present: a number, a range or a value list */
    int32_t num_points;             /* 1 .. VINE_PUSH_MAX_POINTS */
    int32_t per_episode;            /* 0: the table is held; 1: redrawn at every reset raised by the step */
    int32_t points[VINE_PUSH_MAX_POINTS];   /* the first num_points: point indices 0 .. 5 without duplicates */
    float composites[VINE_PUSH_COMPOSITES]; /* rows VI_MTOT .. VI_COUNT - 1 of the configuration's own inertia row */
    uint32_t checked;               /* set by vine_env_push_spec; vine_env_push_scheduled refuses a spec without it */
    uint32_t reserved;
} VineEnvPushSpec;

int vine_env_push_spec_size(void);

/* Host only.  Fills *out from the configuration (seed; its derived inertia rows, through vine_env_inertia_row), the caller's
 * two per-name entries, the value lists (host_values: read for the check; device_values: the same numbers in device memory,
 * only stored), the point list and per_episode.  Refused by name (VINE_ERR_INVALID_ARG, vine_last_error() names PUSH_RATE /
 * PUSH_IMPULSE / POINTS): an absent or unknown form, a non-finite end or value, lo > hi, an extent outside the values array,
 * a radix below 1, a RATE outside [0, 1], a negative IMPULSE, a point list that is empty, longer than VINE_PUSH_MAX_POINTS,
 * holds an index outside 0 .. 5 or one twice, and -- with per_episode 0 -- a RATE or an IMPULSE that is constant zero
 * (nothing to do). */
int vine_env_push_spec(const VineConfig* cfg, const VineEnvRedrawName names[VPU_NAMES], const double* host_values,
                       const double* device_values, int num_values, const int32_t* points, int num_points, int per_episode,
                       VineEnvPushSpec* out);

/* Enqueue the push behind the step just enqueued on `stream`.  reset: the step's buffer (int64 [N]); push_table: float
 * [VPU_NAMES, N]; episode_index: int32 [N], zeros before the first step; push_count: int32 [N].  All on the handle's device.
 * The state block, the bound inertia table and the geometry are the handle's.  Nothing that changes from step to step is an
 * argument: a captured launch replays.  VINE_ERR_INVALID_ARG: a null pointer; a spec vine_env_push_spec did not fill. */
int vine_env_push_scheduled(VineHandle* h, const VineEnvPushSpec* spec, const int64_t* reset, float* push_table,
                            int32_t* episode_index, int32_t* push_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_ENV_PUSH_H */
