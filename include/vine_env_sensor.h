/*
 * vine_env_sensor.h — a sensing path that is not ideal (ENV_SENSOR; product library only): per-env observation delay, dropped
 * frames and per-frame noise, on the device.
 *
 * vine_env_sensor_scheduled is a launch behind every step (a step observer, like vine_env_redraw_scheduled) that rewrites, in
 * place, the observation the step has just written.  The step writes its observation straight into the slot the next
 * inference and the update read, so what the policy sees and what the dataset holds change together.  The step kernels are
 * not touched and nothing but the observation buffer and the observer's own state is ever written: state block, rewards,
 * flags and progress of a run with the sensor are those of a run without it fed the same actions.
 *
 * PER-ENV VALUES.  Env e with global id g = env_id_offset + e runs episode k with three values, held in the device table
 * sensor[VSN_NAMES][N] (float32): DELAY (whole control steps, 0 .. VINE_SENSOR_MAX_DELAY), HOLD (probability per step that no
 * new frame arrives, [0, 1)) and NOISE_STD (>= 0, in the units of the observation as the step wrote it).  Each is the draw of
 * include/vine_env_redraw.h (`redraw_value`) under the name keys of "SENSOR_DELAY", "SENSOR_HOLD" and "SENSOR_NOISE_STD": a pure
 * function of (seed, key, g, k), formed in float64 and rounded once to float32; DELAY is the integer name.  Episode 0's table is
 * built by the host.  With per_episode, a lane that sees reset[e] != 0 behind a step -- after it has handled that step's
 * frame -- increments episode_index[e] and writes the three values of the new k: the moment the redraw acts, so with both on
 * the two ordinals are equal.  Envs reset from outside the step keep their values and ordinal.
 *
 * RING.  Env e has a ring of VINE_SENSOR_SLOTS frames of num_obs floats, ring[slot][e][column]; slots are indexed by the
 * device's step count modulo VINE_SENSOR_SLOTS (vine_steps_completed, as every observer reads it): no per-env cursor, and
 * nothing that changes from step to step is a launch argument.  A ring frame is a whole row; in the columns outside
 * column_mask it holds the observation as written, and those columns of the observation buffer are never stored to.
 *
 * Behind the step with index s (s = steps completed - 1), for env e with values (d, p, std):
 *   1. frame = the observation as written; if std != 0, in every masked column j
 *          frame[j] = clamp(obs[j] + z * c, +-clip_observations)            (one float32 multiply, one float32 add)
 *          c = float32(float64(std) * K),   K = 1 / sqrt(32 * (65536^2 - 1) / 12)  in float64
 *          z = float32(2 * S - 524280),     S = the integer sum of the eight 16-bit halves of one Philox-4x32-10 call keyed
 *          as the step kernels key theirs: counter (g, s, VINE_SENSOR_RNG_NOISE | (s >> 32) << 8, j), key = the seed's words.
 *      z is a zero-mean, unit-variance sum of eight uniforms (support +-4.9 sigma), not a Box-Muller normal: an exact
 *      integer sum and an exact conversion, so that numpy reproduces a frame bit for bit.
 *   2. first = progress[e] == 0 (the step kernels leave that behind exactly the steps that consumed the env's reset) or
 *      fresh[e] != 0 (set for every env at set-up, and by the host for envs reset from outside the step).
 *   3. first: the frame goes into every slot of the env's ring and is delivered as is; fresh[e] is cleared.
 *   4. else: held = u < p (float32) with u = (w >> 8) * 2^-24, w = word 0 of the Philox call with counter
 *      (g, s, VINE_SENSOR_RNG_HOLD | (s >> 32) << 8, 0); pushed = held ? ring[(s - 1) % SLOTS] : frame;
 *      ring[s % SLOTS] = pushed; delivered = ring[(s - d) % SLOTS] (d == 0: pushed itself).
 *   5. the masked columns of the delivered frame overwrite those of the observation buffer (no store where the delivered
 *      frame IS the observation: std == 0 and (first or (not held and d == 0))).
 * So no frame of an earlier episode is delivered in a later one, for the first d steps of an episode the policy sees its
 * first frame, and with d = p = std = 0 the buffer keeps every bit.
 *
 * The kernel: one lane per env, 256 lanes per workgroup, no LDS, no atomics; a lane is the only writer of its env's table
 * entries, ring, fresh byte and episode_index.  Rows move as 16-byte vectors where num_obs is a multiple of four (28), else as
 * 8-byte ones (14, 18, 26).  The translation unit is compiled without floating-point contraction.
 */
#ifndef VINE_ENV_SENSOR_H
#define VINE_ENV_SENSOR_H

#include "vine_env_redraw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_ENV_SENSOR_ABI_VERSION 1
#define VINE_ENV_SENSOR_THREADS 256
#define VINE_SENSOR_MAX_DELAY 8                         /* = VINE_MAX_DELAY */
#define VINE_SENSOR_SLOTS (VINE_SENSOR_MAX_DELAY + 1)
/* The purpose words of the two Philox streams; the step kernels' own stop at 4 (vine_hip.hip). */
#define VINE_SENSOR_RNG_NOISE 5u
#define VINE_SENSOR_RNG_HOLD 6u

/* The names of a spec and the rows of the sensor table, in this order (the mixed radix of value lists counts in it too). */
typedef enum VineEnvSensorSlot { VSN_DELAY = 0, VSN_HOLD, VSN_NOISE_STD, VSN_NAMES = 3 } VineEnvSensorSlot;

typedef struct VineEnvSensorSpec {
    int32_t abi_version;            /* VINE_ENV_SENSOR_ABI_VERSION */
    int32_t num_values;             /* doubles in the values array */
    uint64_t seed;
    const double* values;           /* DEVICE array of the value lists, the caller's; may be NULL when num_values == 0 */
    VineEnvRedrawName name[VSN_NAMES];      /* every one present: a number, a range or a value list */
    int32_t num_obs;                /* columns of the configuration's observation */
    uint32_t column_mask;           /* bit j: the model applies to column j */
    float clip_observations;
    int32_t per_episode;            /* 0: the table is held; 1: redrawn at every reset raised by the step */
    uint32_t checked;               /* set by vine_env_sensor_spec; vine_env_sensor_scheduled refuses a spec without it */
    uint32_t reserved;
} VineEnvSensorSpec;

int vine_env_sensor_spec_size(void);

/* Host only.  Fills *out from the configuration (seed, num_obs, clip_observations), the caller's three per-name entries, the
 * value lists (host_values: read for the check; device_values: the same numbers in device memory, only stored), the column
 * mask and per_episode.  Refused by name (VINE_ERR_INVALID_ARG, vine_last_error() names SENSOR_DELAY / SENSOR_HOLD /
 * SENSOR_NOISE_STD / COLUMNS): an absent or unknown form, a non-finite end or value, lo > hi, an extent outside the values
 * array, a radix below 1, a DELAY that is not an integer in 0 .. VINE_SENSOR_MAX_DELAY, a HOLD outside [0, 1), a negative
 * NOISE_STD, an empty mask or one with a bit at or above num_obs, and -- with per_episode 0 -- three values that are
 * constant zero (nothing to do). */
int vine_env_sensor_spec(const VineConfig* cfg, const VineEnvRedrawName names[VSN_NAMES], const double* host_values,
                         const double* device_values, int num_values, uint32_t column_mask, int per_episode,
                         VineEnvSensorSpec* out);

/* Enqueue the sensor behind the step just enqueued on `stream`.  obs: the buffer that step wrote, float [N, num_obs] (it
 * may differ from step to step on the host side; a captured launch keeps the one it was captured with); reset, progress:
 * the step's buffers (int64 [N]); sensor_table: float [VSN_NAMES, N]; ring: float [VINE_SENSOR_SLOTS, N, num_obs]; fresh:
 * uint8 [N], ones before the first step; episode_index: int32 [N], zeros before the first step.  All on the handle's device.
 * VINE_ERR_INVALID_ARG: a null pointer; a spec vine_env_sensor_spec did not fill; obs or ring not aligned to the row
 * vector (16 bytes where num_obs is a multiple of four, else 8). */
int vine_env_sensor_scheduled(VineHandle* h, const VineEnvSensorSpec* spec, float* obs, const int64_t* reset,
                              const int64_t* progress, float* sensor_table, float* ring, uint8_t* fresh,
                              int32_t* episode_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_ENV_SENSOR_H */
