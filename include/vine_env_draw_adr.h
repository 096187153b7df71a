/*
 * vine_env_draw_adr.h — automatic domain randomisation of the sensor's, the push's and the target's named draws
 * (ENV_DRAW_ADR; extension of include/vine_env_sensor.h, vine_env_push.h and vine_env_target.h; product library only).
 *
 * Each of those three observers redraws an env's values from fixed [lo, hi] ranges whenever its episode ends, as the last
 * statement of its launch, and none of them reads the new row in the launch that writes it.  Here the ranges of the names
 * under ADR start at START = [start_lo, start_hi] inside those ranges, which become the LIMITS, and each of their two
 * boundaries moves by whole STEPs, by the rule of include/vine_env_adr.h: a share of the redrawn episodes is pinned to one
 * boundary of one name (it PROBES that boundary), and when QUEUE probing episodes of a boundary have finished, the boundary
 * moves one STEP outward if at least WIDEN_AT of them reached the target, one STEP back (never inside START) if at most
 * NARROW_AT did.  It happens in two launches that run behind the three observers' in the same step and replace the rows
 * those have just drawn for a flagged env; neither the step kernels nor the observers' kernels are touched.
 *
 * The nine names, in slot order: SENSOR_DELAY, SENSOR_HOLD, SENSOR_NOISE_STD (group 0, the sensor's table, rows 0..2),
 * PUSH_RATE, PUSH_IMPULSE (group 1, the push's table, rows 0..1), TARGET_VEL_ALONG, TARGET_VEL_ACROSS, TARGET_SPAN_ALONG,
 * TARGET_SPAN_ACROSS (group 2, the target's table, rows 0..3).  SENSOR_DELAY ranges over the integers.
 *
 * State, all integers, all the caller's device buffers (zeroed before the first step, probe filled with -1):
 *   widen   int32 [9][2]             steps taken outward per boundary (side 0 = lo, 1 = hi).  The range in force is
 *                                      lo = max(limit_lo, start_lo - widen_lo * step)
 *                                      hi = min(limit_hi, start_hi + widen_hi * step)
 *                                    one multiply and one add in float64 from the integers, without contraction: the host
 *                                    (utils/env_draw_adr.py draw_adr_replay) forms the same bits.
 *   counts  int32 [9][2][2]          per boundary: probing episodes finished since its last decision, and how many reached
 *   reached int32 [N]                the OR over the running episode's steps of reward-matrix column 2 != 0
 *   probe   int32 [N]                the boundary the env's running episode is pinned to, 2 * slot + side, or -1
 *   episode_index int32 [N]          this observer's own count of the env's episodes; it equals the three observers'
 *   history int32 [capacity][4]      a ring of (step index, boundary, new widen, 0), one row per change
 *   cursor  int64 [1]                rows appended so far
 *
 * Launch 1 (decide): one wave, lane b = boundary b of 18; the rule, the ballot-ordered history rows and the cursor update
 * are those of vine_env_adr_decide_kernel (csrc/vine_adr_shared.h states them once).
 *
 * Launch 2 (redraw): one lane per env, 256 per workgroup.  Every lane ORs rm[e][2] != 0 into reached[e]; a workgroup
 * without a flagged lane leaves.  A flagged lane (reset[e] != 0)
 *   - with probe[e] >= 0 adds (1, reached[e]) to counts[probe[e]] (LDS integer atomics, then at most 36 global integer
 *     atomics per workgroup: the sums do not depend on the order);
 *   - clears reached[e], increments episode_index[e] to k;
 *   - with g the global env id draws u_p = u(seed, key("DRAW_ADR_PROBE"), g, k); if u_p < boundary_fraction,
 *     u_w = u(seed, key("DRAW_ADR_WHICH"), g, k) picks boundary j = min(floor(u_w * 2A), 2A - 1) of the A names under ADR in
 *     slot order, lo before hi, and probe[e] = 2 * slot + side; else probe[e] = -1;
 *   - for every name under ADR: v = redraw_value(nm', integer, values, seed, g, k) with nm' the observer's own checked
 *     VineEnvRedrawName, lo and hi replaced by the range in force -- the key is the observer's, so u is the one its tail has
 *     just used --; a probed name gets exactly its boundary; (float)v is stored at table[group][row * N + e].
 * Nothing else is written: no row of a name that is not under ADR, no table of a group without a name under ADR, nothing of
 * the state block or the observation.
 *
 * Episode 0 is the host's: the rows of the names under ADR hold episode 0's draw from START.  Envs reset from outside the
 * step raise no flag and keep their values; the caller sets their reached = 0 and probe = -1.
 */
#ifndef VINE_ENV_DRAW_ADR_H
#define VINE_ENV_DRAW_ADR_H

#include "vine_env_adr.h"
#include "vine_env_push.h"
#include "vine_env_sensor.h"
#include "vine_env_target.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_ENV_DRAW_ADR_ABI_VERSION 1
#define VINE_ENV_DRAW_ADR_THREADS 256
#define VINE_ENV_DRAW_ADR_HISTORY_WORDS 4
#define VINE_ENV_DRAW_ADR_KEY_PROBE 0x13605cadb5285d5eull    /* the 64-bit key (see VineEnvRedrawName.key) of "DRAW_ADR_PROBE" */
#define VINE_ENV_DRAW_ADR_KEY_WHICH 0x5ce5f9cbbb3b47a7ull    /* ... of "DRAW_ADR_WHICH" */

/* The groups: whose table a name's row lies in. */
typedef enum VineEnvDrawAdrGroup { VDA_SENSOR = 0, VDA_PUSH = 1, VDA_TARGET = 2, VDA_GROUPS = 3 } VineEnvDrawAdrGroup;

/* The names, in slot order. */
typedef enum VineEnvDrawAdrSlotIndex {
    VDA_SENSOR_DELAY = 0, VDA_SENSOR_HOLD, VDA_SENSOR_NOISE_STD, VDA_PUSH_RATE, VDA_PUSH_IMPULSE, VDA_TARGET_VEL_ALONG,
    VDA_TARGET_VEL_ACROSS, VDA_TARGET_SPAN_ALONG, VDA_TARGET_SPAN_ACROSS, VDA_NAMES = 9
} VineEnvDrawAdrSlotIndex;

typedef struct VineEnvDrawAdrSlot {
    VineEnvAdrName adr;             /* on, START, STEP as the caller stated them; all 0 for a name that is not under ADR */
    int32_t max_widen[2];           /* steps between START and the limit per side, as VineEnvAdrSpec.max_widen */
    int32_t group;                  /* VineEnvDrawAdrGroup */
    int32_t row;                    /* the name's row in its group's table */
    int32_t integer;                /* 1: the range is over the integers (SENSOR_DELAY) */
    int32_t reserved;
    VineEnvRedrawName limits;       /* the observer's own checked name: its [lo, hi] are the limits, its key the draw's */
} VineEnvDrawAdrSlot;

typedef struct VineEnvDrawAdrSpec {
    int32_t abi_version;            /* VINE_ENV_DRAW_ADR_ABI_VERSION */
    int32_t num_adr;                /* A: names under ADR */
    int32_t queue;                  /* finished probing episodes per boundary before a decision */
    int32_t history_capacity;       /* rows of the history ring */
    double boundary_fraction;       /* share of redrawn episodes that probe a boundary, in [0, 1) */
    double widen_at, narrow_at;     /* reached rates, narrow_at < widen_at */
    uint64_t seed;
    VineEnvDrawAdrSlot slot[VDA_NAMES];
    int32_t adr_slot[VDA_NAMES];    /* the slots of the A names under ADR, ascending; the rest -1 */
    uint32_t checked;               /* set by vine_env_draw_adr_spec; vine_env_draw_adr_scheduled refuses a spec without it */
} VineEnvDrawAdrSpec;

int vine_env_draw_adr_spec_size(void);

/* Host only.  Fills *out from the three observers' checked specs (NULL for an observer that is off; the limits and the keys
 * are copied from them) and the caller's per-name entries.  VINE_ERR_INVALID_ARG, vine_last_error() naming the name or the
 * key: a null cfg, names or out; an ABI mismatch of any struct; an observer spec that was not checked; a name under ADR
 * whose observer spec is NULL, whose observer is not per_episode or whose form is not a [lo, hi] range; START not finite,
 * outside the limits or with lo > hi; STEP not finite or <= 0; a non-integer START or STEP for SENSOR_DELAY; a non-zero
 * START or STEP on a name that is off; no name on; boundary_fraction outside [0, 1); queue < 1; narrow_at >= widen_at (or
 * either not finite); history_capacity < 1; more than 2^30 steps between START and a limit. */
int vine_env_draw_adr_spec(const VineConfig* cfg, const VineEnvSensorSpec* sensor, const VineEnvPushSpec* push,
                           const VineEnvTargetSpec* target, const VineEnvAdrName names[VDA_NAMES], double boundary_fraction,
                           int queue, double widen_at, double narrow_at, int history_capacity, VineEnvDrawAdrSpec* out);

/* Enqueue the two launches behind the step just enqueued on `stream`, and behind the three observers' launches of that
 * step.  reset: the step's buffer (int64 [N]); tables[VDA_GROUPS]: the sensor's, the push's and the target's tables (float
 * [rows, N]; NULL allowed for a group without a name under ADR); values: the device array of value lists redraw_value takes
 * (no name under ADR reads it: may be NULL); the rest: the state above.  Nothing is allocated, nothing synchronises, and no
 * argument changes from step to step: a captured pair replays.  VINE_ERR_INVALID_ARG: a null pointer, the table of a group
 * with a name under ADR included; a spec vine_env_draw_adr_spec did not fill; no reward matrix bound to the handle
 * (vine_bind_reward_matrix). */
int vine_env_draw_adr_scheduled(VineHandle* h, const VineEnvDrawAdrSpec* spec, const int64_t* reset,
                                float* const tables[VDA_GROUPS], const double* values, int32_t* widen, int32_t* counts,
                                int32_t* reached, int32_t* probe, int32_t* episode_index, int32_t* history, int64_t* cursor,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_ENV_DRAW_ADR_H */
