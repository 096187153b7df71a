/*
 * vine_env_adr.h — automatic domain randomisation of the per-episode plant (ENV_PARAMS_ADR; extension of
 * include/vine_env_redraw.h; product library only).
 *
 * vine_env_redraw_scheduled redraws an env's plant from fixed [lo, hi] ranges whenever its episode ends.  Here the ranges of
 * the names under ADR start at START = [start_lo, start_hi] inside those ranges, which become the LIMITS, and each of their
 * two boundaries moves by whole STEPs: a share of the redrawn episodes is pinned to one boundary of one name (it PROBES that
 * boundary), and when QUEUE probing episodes of a boundary have finished, the boundary moves one STEP outward if at least
 * WIDEN_AT of them reached the target, one STEP back (never inside START) if at most NARROW_AT did, and their count starts
 * anew either way.  All of it happens in two launches behind every step (a step observer, in the place of the redraw's); the
 * step kernels are not touched.
 *
 * State, all integers, all the caller's device buffers (zeroed before the first step, probe filled with -1):
 *   widen   int32 [VR_NAMES][2]      steps taken outward per boundary (side 0 = lo, 1 = hi).  The range in force is
 *                                      lo = max(limit_lo, start_lo - widen_lo * step)
 *                                      hi = min(limit_hi, start_hi + widen_hi * step)
 *                                    one multiply and one add in float64 from the integers: nothing accumulates, the host
 *                                    (utils/env_params.py adr_replay) forms the same bits.
 *   counts  int32 [VR_NAMES][2][2]   per boundary: probing episodes finished since its last decision, and how many reached
 *   reached int32 [N]                the env's running episode has reached the target: the OR over its steps of
 *                                    reward-matrix column 2 != 0, the term vine_episodes.h reads `reached_ever` from
 *   probe   int32 [N]                the boundary the env's running episode is pinned to, 2 * slot + side, or -1
 *   episode_index int32 [N]          as in vine_env_redraw.h
 *   history int32 [capacity][4]      a ring of (step index, boundary, new widen, 0), one row per change; `step index` is the
 *   cursor  int64 [1]                index of the step the launch rides behind (steps completed - 1); rows appended so far
 *
 * Launch 1 (decide): one wave, lane b = boundary b.  A boundary with counts.n >= queue is judged: reached >= widen_at * n
 * (both sides in float64) moves widen to min(widen + 1, max_widen); else reached <= narrow_at * n moves it to
 * max(widen - 1, 0); the counts are cleared either way.  A boundary whose widen CHANGED appends a history row; the rows of
 * one launch take consecutive slots in boundary order (a ballot's prefix count, not arrival).
 *
 * Launch 2 (redraw): one lane per env, 256 per workgroup.  Every lane ORs rm[e][2] != 0 into reached[e]; a lane whose
 * reset[e] == 0 then leaves.  A flagged lane
 *   - with probe[e] >= 0 adds (1, reached[e]) to counts[probe[e]] (integer adds: the sums do not depend on the order; an
 *     episode drawn before its boundary moved still counts);
 *   - clears reached[e], increments episode_index[e] to k;
 *   - draws every name of the redraw spec as vine_env_redraw_kernel does, the names under ADR from the range in force;
 *   - draws u_p = u(seed, key("ADR_PROBE"), g, k); if u_p < boundary_fraction, u_w = u(seed, key("ADR_WHICH"), g, k) picks
 *     boundary j = min(floor(u_w * 2A), 2A - 1) of the A names under ADR in slot order, lo before hi: that name's value
 *     becomes exactly the boundary and probe[e] = 2 * slot + side; else probe[e] = -1;
 *   - writes the columns and zeroes the delay ring where the delay changed, exactly as vine_env_redraw_kernel does.
 * The columns lie inside the limits, which vine_env_redraw_spec has put through the table checks at both ends.
 *
 * Envs reset from outside the step raise no flag and keep their plant; the caller sets their reached = 0 and probe = -1, so
 * their discarded episode is not counted (the episode log writes no row for it either).
 */
#ifndef VINE_ENV_ADR_H
#define VINE_ENV_ADR_H

#include "vine_env_redraw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_ENV_ADR_ABI_VERSION 1
#define VINE_ENV_ADR_THREADS 256
#define VINE_ENV_ADR_HISTORY_WORDS 4
#define VINE_ENV_ADR_KEY_PROBE 0x32006ca9afc13c78ull    /* the 64-bit key (see VineEnvRedrawName.key) of "ADR_PROBE" */
#define VINE_ENV_ADR_KEY_WHICH 0x25473c155fa82938ull    /* ... of "ADR_WHICH" */

/* What the caller states per name; `on` == 0: the name is not under ADR and the other fields must be 0. */
typedef struct VineEnvAdrName {
    int32_t on;
    int32_t reserved;               /* must be 0 */
    double start_lo, start_hi;      /* where the range begins; narrowing never crosses it */
    double step;                    /* what one decision moves a boundary by */
} VineEnvAdrName;

typedef struct VineEnvAdrSpec {
    int32_t abi_version;            /* VINE_ENV_ADR_ABI_VERSION */
    int32_t num_adr;                /* A: names under ADR */
    int32_t queue;                  /* finished probing episodes per boundary before a decision */
    int32_t history_capacity;       /* rows of the history ring */
    double boundary_fraction;       /* share of redrawn episodes that probe a boundary, in [0, 1) */
    double widen_at, narrow_at;     /* reached rates, narrow_at < widen_at */
    VineEnvAdrName name[VR_NAMES];
    int32_t max_widen[VR_NAMES][2]; /* ceil((start_lo - limit_lo) / step), ceil((limit_hi - start_hi) / step); one more where
                                       the rounded quotient would leave the last step an ulp inside the limit */
    int32_t adr_slot[VR_NAMES];     /* the slots of the A names under ADR, ascending; the rest -1 */
    uint32_t checked;               /* set by vine_env_adr_spec; vine_env_adr_scheduled refuses a spec without it */
    uint32_t reserved;
    VineEnvRedrawSpec redraw;       /* the redraw's spec: its ranges are the limits */
} VineEnvAdrSpec;

int vine_env_adr_spec_size(void);

/* Host only.  Fills *out from a spec vine_env_redraw_spec has filled (its ranges are the limits, already put through the
 * table checks at both ends) and the caller's per-name entries.  VINE_ERR_INVALID_ARG, vine_last_error() naming the name or
 * the key: a null pointer; a redraw spec that was not checked; no name under ADR; a name under ADR that is not a [lo, hi]
 * range of the redraw spec; START not finite, outside the limits or with lo > hi; STEP not finite or <= 0; a non-integer
 * START or STEP for ACTION_DELAY; boundary_fraction outside [0, 1); queue < 1; narrow_at >= widen_at (or either not
 * finite); history_capacity < 1; more than 2^30 steps between START and a limit. */
int vine_env_adr_spec(const VineConfig* cfg, const VineEnvRedrawSpec* redraw, const VineEnvAdrName names[VR_NAMES],
                      double boundary_fraction, int queue, double widen_at, double narrow_at, int history_capacity,
                      VineEnvAdrSpec* out);

/* Enqueue the two launches behind the step just enqueued on `stream`.  reset, params_table, inertia_table, episode_index:
 * as for vine_env_redraw_scheduled; widen, counts, reached, probe, history, cursor: the state above.  Nothing that changes
 * from step to step is an argument, so a captured launch pair replays correctly.
 * VINE_ERR_INVALID_ARG: what vine_env_redraw_scheduled refuses; a spec vine_env_adr_spec did not fill; no reward matrix
 * bound to the handle (vine_bind_reward_matrix). */
int vine_env_adr_scheduled(VineHandle* h, const VineEnvAdrSpec* spec, const int64_t* reset, float* params_table,
                           float* inertia_table, int32_t* episode_index, int32_t* widen, int32_t* counts, int32_t* reached,
                           int32_t* probe, int32_t* history, int64_t* cursor, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_ENV_ADR_H */
