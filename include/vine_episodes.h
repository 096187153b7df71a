/*
 * vine_episodes.h — C ABI of the per-episode task log (EPISODE_LOG) for MI355X (gfx950).
 *
 * This is a reaching task: what its users ask is how often the tip reaches the target, from where, how fast, and why the
 * other episodes ended.  vine_step_eval (include/vine_ppo.h) answers with twelve sums, and only on the four-lanes-per-env
 * kernel in evaluation mode.  This header is the observer form of that accounting, the per-episode twin of
 * include/vine_record.h: a launch BEHIND any step launch (vine_step, vine_step_rollout, vine_step_eval; both step kernels)
 * keeps each env's running episode, and when the step has raised the env's reset flag it adds the finished episode to
 * float64 totals and appends one row to a ring on the device.
 *
 * Only libvine_hip.so exports this header (the CPU oracle does not).  Errors, streams and ownership as in vine.h: 0 = ok,
 * negative = VineStatus, message via vine_last_error(); every entry point enqueues on the caller's stream and does not
 * synchronise; the caller owns every buffer.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * THE SOURCE.  The task's own tests are READ from the step's reward-matrix row (vine.h, vine_bind_reward_matrix: [N,13]
 * row-major, written by both step kernels in all three modes), not re-derived from the state:
 *
 *     dist = -rm[0]     reached = rm[2] != 0     limit_hit = rm[9] != 0     tip_limit_hit = rm[11] != 0
 *     contact = rm[12] < 0
 *
 * They are what the step's reward and reset were built from -- including the stale body state of the step after a reset
 * (VINE_FLAG_STALE_BODY_STATE_AFTER_RESET) -- so the log cannot disagree with the reset the step requested.  A reward
 * matrix must therefore be bound to the handle (which arms VINE_FLAG_INTROSPECT) before the first logged step.
 *
 * THE ACCUMULATORS.  episode[VINE_EVAL_EPISODE_FIELDS][N] fp32, struct of arrays, started by the caller at
 * (0, 0, +inf, 0); the definitions are vine_step_eval's VINE_EVAL_EP_*: return (sum of the raw rew, added step by step
 * in fp32), length, smallest dist, 1-based step of the first reach (0 = not yet).  An env whose reset flag is set after
 * the step has finished its episode: the accumulators return to their start values.  A caller that resets envs from
 * outside the step (vine_reset_idx) returns those envs' accumulators to the start values itself: no row.
 *
 * THE TOTALS.  totals[vine_episodes_rows(h)][VINE_EVAL_NUM_TOTALS] float64 (in/out; the caller zeroes it): the twelve
 * columns and meanings of vine_step_eval's totals (END_* count a reason only if its reset switch is armed; the rail
 * limit always is).  A workgroup adds its finished episodes, summed in float64 in a fixed order, to its own row, and
 * only in a step in which it finished one.  No float atomics: the totals are bit-reproducible.
 *
 * THE ROW.  VINE_EPISODES_WORDS = 16 32-bit words (64 bytes) per finished episode, VineEpisodeWord below:
 *
 *   0      i32  env
 *   1      i32  index of the step that ended the episode (steps completed - 1, as vine_record.h counts)
 *   2      f32  length
 *   3      f32  return
 *   4      f32  reached_ever, 0 or 1
 *   5      f32  reached_at_end, 0 or 1
 *   6      f32  first_reach (0 = never)
 *   7      f32  final_dist
 *   8      f32  min_dist
 *   9      i32  end-reason bits VINE_EPISODES_END_*: timeout, rail limit, tip limit, contact (armed reasons only)
 *   10-13  f32  target y, target z, obj_depth, obj_angle: VF_TARGET_Y/Z, VF_OBJ_DEPTH/ANGLE -- still the finished
 *               episode's own, since the NEXT step consumes the reset
 *   14-15       zero
 *
 * SLOTS.  cursor[0] (device int64, the caller zeroes it) counts every row ever appended; row k lives in slot
 * k % capacity of table[capacity][VINE_EPISODES_WORDS].  One returning integer atomic per wave that finished an episode
 * hands out k; a wave's rows are consecutive in lane (= env) order, the order of the waves within a step is unspecified.
 * The row SET and every value are bit-reproducible; a reader sorts by (end step, env).  Rows the writer laps before
 * the reader has copied them are lost and COUNTED: dropped = max(0, cursor - harvested - capacity), harvested = the
 * cursor at the reader's last copy.  What survives is the newest `capacity` rows in append order: every row of the steps
 * after the lapped one, and of the step in which the lap happened an unspecified subset of the right size.
 * With capacity < num_envs one step can append more rows than the ring holds, and two waves would write one slot.  For
 * such a ring the launch is one workgroup that walks the envs in order: the rows of a step are then appended in env
 * order, a row that the same step would lap is not written at all, and the survivors are exactly the newest `capacity`
 * rows by (end step, env).  That form is for small rings in tests and tools; it is serial in the env count.
 * table == NULL and cursor == NULL together: totals only.
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_EPISODES_H
#define VINE_EPISODES_H

#include <stdint.h>

#include "vine.h"
#include "vine_ppo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_EPISODES_ABI_VERSION 1
#define VINE_EPISODES_WORDS 16
#define VINE_EPISODES_THREADS 256      /* envs per workgroup = envs per row of the totals */

typedef enum VineEpisodeWord {
    VEW_ENV = 0,
    VEW_END_STEP = 1,
    VEW_LENGTH = 2,
    VEW_RETURN = 3,
    VEW_REACHED_EVER = 4,
    VEW_REACHED_AT_END = 5,
    VEW_FIRST_REACH = 6,
    VEW_FINAL_DIST = 7,
    VEW_MIN_DIST = 8,
    VEW_END_REASON = 9,
    VEW_TARGET_Y = 10,
    VEW_TARGET_Z = 11,
    VEW_OBJ_DEPTH = 12,
    VEW_OBJ_ANGLE = 13,
    VEW_RESERVED0 = 14
} VineEpisodeWord;

enum {
    VINE_EPISODES_END_TIMEOUT = 1,
    VINE_EPISODES_END_RAIL_LIMIT = 2,
    VINE_EPISODES_END_TIP_LIMIT = 4,
    VINE_EPISODES_END_CONTACT = 8
};

typedef struct VineEpisodesConfig {
    int32_t abi_version;   /* must be VINE_EPISODES_ABI_VERSION */
    int32_t reserved;      /* 0 */
    int64_t capacity;      /* rows of the ring; >= 1; default 1048576 */
} VineEpisodesConfig;

int vine_episodes_config_default(VineEpisodesConfig* cfg);
int vine_episodes_config_size(void);      /* sizeof(VineEpisodesConfig): checked by the ctypes mirror */

/* Rows of `totals`: one per VINE_EPISODES_THREADS envs; negative = VineStatus. */
int vine_episodes_rows(VineHandle* h);

/* Bytes of the ring: capacity * VINE_EPISODES_WORDS * 4; negative = VineStatus. */
int64_t vine_episodes_table_bytes(const VineEpisodesConfig* cfg);

/* The graph node.  Enqueued behind a step launch on the same stream, it reads the handle's device step counter
 * c = steps completed exactly as vine_record_scheduled does; the step just finished has index c - 1 (with c == 0 the
 * launch touches nothing).  Nothing that changes from step to step is a kernel argument, so a captured launch replays
 * correctly.
 * rew, reset, progress, timeouts   the step's output buffers (vine.h, vine_step).  progress is not read: an episode's
 *           length is the accumulator's, which a caller that reset the env from outside has started over
 * episode   device float[VINE_EVAL_EPISODE_FIELDS][N], in/out
 * totals    device double[vine_episodes_rows(h)][VINE_EVAL_NUM_TOTALS], in/out
 * table     device uint32[capacity][VINE_EPISODES_WORDS], 16-byte aligned, or NULL
 * cursor    device int64[1], in/out, or NULL (with table)
 * VINE_ERR_INVALID_ARG for a null pointer, a bad config, and when no reward matrix is bound to the handle. */
int vine_episodes_scheduled(VineHandle* h, const VineEpisodesConfig* cfg, const float* rew, const int64_t* reset,
                            const int64_t* progress, const uint8_t* timeouts, float* episode, double* totals,
                            uint32_t* table, int64_t* cursor, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_EPISODES_H */
