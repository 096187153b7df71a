/*
 * vine_mpc_track.h — the predictive controller's samples see the target move over the horizon (MPC_TRACK; product library
 * only): one short table of target positions per plant, written in front of the fork, and a launch behind every model step
 * that stores the next entry into every live sample.
 *
 * The plant of include/vine_mpc.h may carry a moving target (include/vine_env_target.h); the model handle never does.
 * vine_mpc_fork copies VF_TARGET_Y/Z and VF_OBJ_DEPTH as they stand behind the plant's last step -- the target of time t + 1 --
 * into every sample, and without this header all H model steps score the tip against that one point.  The target's path does
 * not depend on the actions, so it is a table per plant and not per sample, and the step kernels read the target from the
 * state block on every step, so a store between two model steps is all a sample needs.  The step kernels, vine_mpc.hip and
 * vine_env_target_scheduled are not touched.
 *
 * BUFFERS.  All the caller's, on the handles' device; M = num_plants, K = samples, H = horizon of the VineMpcConfig:
 *   path[M][H][3]   float32   (TY, TZ, DEPTH) of plant p at horizon entry k: what model step k + 1 reads
 *   live[M]         uint8     1: the plant's samples follow path[p]; 0: they keep what the fork gave them
 * and, read only: the plant observer's motion[VTM_COUNT][M], fresh[M] and target_table[VTG_NAMES][M]
 * (include/vine_env_target.h), the plant handle's reset buffer, the controller's window[1] and alive[M * K] (include/vine_mpc.h).
 *
 * PATH KINDS.  VINE_TRACK_EXACT: the planner knows the path as the plant's observer walks it -- anchor, offset, velocity,
 * span, reflections: the upper bound.  VINE_TRACK_LINEAR: the planner knows the current signed velocity only and extrapolates
 * without reflections: what the policy is told through its target-velocity columns.  VINE_TRACK_HELD: both launches run and
 * change nothing: the launches alone, for tests and measurements.
 *
 * THE PLAN.  vine_mpc_track_plan, one lane per plant p, enqueued once per control step in front of vine_mpc_fork.  It reads
 * the plant handle's state block, motion, fresh, target_table and plant_reset and writes none of them; it writes path and live.
 *   1. path[p][0] = (VF_TARGET_Y, VF_TARGET_Z, VF_OBJ_DEPTH) of plant p's column, the words themselves.  They hold the target
 *      of time t + 1, which model step 1 reads after the fork has copied it.
 *   2. live[p] = path kind != HELD && plant_reset[p] == 0 && fresh[p] == 0 && (motion's VEL_ALONG and VEL_ACROSS of p are not both
 *      exactly zero).  live[p] = 0 covers a plant whose next step only consumes a reset, a plant reset from outside the step
 *      (its motion rows are stale until the next launch of the observer anchors them) and a resting plant.  A plant that is not
 *      live gets path[p][k] = path[p][0] for every k: the table is defined everywhere.
 *   3. a live plant starts from (off, vel) = motion's OFF_ALONG/ACROSS and VEL_ALONG/ACROSS.  For k = 1 .. H - 1 it takes one
 *      control step along the path, then forms the words of step 5 of include/vine_env_target.h for the spec's mode from
 *      motion's ANCHOR_Y/Z, DEPTH0 and AXIS_C/S and the offsets:
 *          free space:  TY = ay + off_along,      TZ = az + off_across
 *          shelf:       TY = ay - off_along,                               DEPTH = depth0 + off_along
 *          pipe:        TY = ay - off_along * c,  TZ = az - off_along * s,  DEPTH = depth0 + off_along
 *      A word the mode does not write repeats path[p][0]'s.  The path step, per axis (along; across in free space only):
 *          EXACT:   step 4 of include/vine_env_target.h with S the table's SPAN of that axis: n = off + vel * cdt; if n > S:
 *                   n = S - (n - S), vel = -vel; else if n < -S: n = -S - (n + S), vel = -vel; off = n
 *          LINEAR:  off = off + vel * cdt, one multiply and one add, never reflected
 *      Everything is float32, without contraction, in that order of operations; cdt is the plant spec's.  So for a plant that
 *      neither resets nor is redrawn meanwhile, the EXACT entry k holds, in every bit, the three words the plant's observer
 *      leaves in the state block behind k more steps.
 *
 * THE NODE.  vine_mpc_track_scheduled, one lane per model env e = p * K + j, enqueued behind every vine_mpc_scheduled of the
 * horizon on the same stream.  With c the MODEL handle's step count read on the device (steps completed, as every observer
 * reads it) and k = c - window[0], it touches nothing unless 1 <= k <= H - 1, live[p] != 0 and alive[e] != 0 (as the node of
 * include/vine_mpc.h has just left it: a sample whose episode ended keeps what its reset will replace).  When they hold it stores
 * path[p][k] into the sample's column: VF_TARGET_Y in every mode, VF_TARGET_Z in free space and the pipe, VF_OBJ_DEPTH at the
 * shelf and in the pipe.  No other field, no observation, no reward and no flag is written: model step k + 1 reads the moved
 * target, and its distance, reward, success test and observation follow.  Nothing that changes from step to step is an
 * argument, so a captured launch replays.
 *
 * The kernels: 256 lanes per workgroup, no LDS, no atomics; a lane is the only writer of its entries.  The translation unit
 * is compiled without floating-point contraction; csrc/vine_target_path.h states the path step and the words once, for this
 * unit and for vine_env_target.hip.
 */
#ifndef VINE_MPC_TRACK_H
#define VINE_MPC_TRACK_H

#include "vine_env_target.h"
#include "vine_mpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_MPC_TRACK_ABI_VERSION 1
#define VINE_MPC_TRACK_THREADS 256
#define VINE_MPC_TRACK_WORDS 3      /* TY, TZ, DEPTH of a path entry */

typedef enum VineMpcTrackPath { VINE_TRACK_EXACT = 0, VINE_TRACK_LINEAR = 1, VINE_TRACK_HELD = 2 } VineMpcTrackPath;

typedef struct VineMpcTrackSpec {
    int32_t abi_version;            /* VINE_MPC_TRACK_ABI_VERSION */
    int32_t num_plants;             /* M */
    int32_t samples;                /* K */
    int32_t horizon;                /* H */
    int32_t mode;                   /* VineEnvTargetMode, the plant spec's */
    int32_t path;                   /* VineMpcTrackPath */
    float cdt;                      /* the plant spec's control period */
    uint32_t checked;               /* set by vine_mpc_track_spec; the two launches refuse a spec without it */
    uint32_t reserved[8];           /* zero; pads the struct to 64 bytes */
} VineMpcTrackSpec;

int vine_mpc_track_spec_size(void);

/* Host only.  Fills *out from the plant's CHECKED target spec (cdt and mode), the controller's configuration (M, K, H) and the
 * path kind, and sets checked.  VINE_ERR_INVALID_ARG, vine_last_error() naming the reason: a null pointer; a plant spec that
 * vine_env_target_spec did not fill; an abi_version mismatch of the plant spec or of the configuration; num_plants < 1 or
 * samples < 2; a path that is not a VineMpcTrackPath; a horizon outside 1 .. VINE_MPC_MAX_HORIZON. */
int vine_mpc_track_spec(const VineEnvTargetSpec* plant_spec, const VineMpcConfig* cfg, int path, VineMpcTrackSpec* out);

/* Enqueue the plan (see THE PLAN) in front of vine_mpc_fork.  plant_reset: the plant handle's reset buffer, int64 [M]; fresh,
 * target_table, motion: the plant observer's (include/vine_env_target.h); path: float [M, H, 3]; live: uint8 [M].
 * VINE_ERR_INVALID_ARG: a null pointer; a spec vine_mpc_track_spec did not fill; a plant handle without num_plants envs; a
 * spec whose mode is not that of the handle's obstacle flags. */
int vine_mpc_track_plan(VineHandle* plant, const VineMpcTrackSpec* spec, const int64_t* plant_reset, const uint8_t* fresh,
                        const float* target_table, const float* motion, float* path, uint8_t* live, void* stream);

/* Enqueue the node (see THE NODE) behind a vine_mpc_scheduled of the horizon.  window, alive: the controller's
 * (include/vine_mpc.h); path, live: what the plan wrote.  VINE_ERR_INVALID_ARG: a null pointer; a spec vine_mpc_track_spec did
 * not fill; a model handle without num_plants * samples envs; a spec whose mode is not that of the handle's obstacle flags. */
int vine_mpc_track_scheduled(VineHandle* model, const VineMpcTrackSpec* spec, const int64_t* window, const uint8_t* alive,
                             const float* path, const uint8_t* live, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_MPC_TRACK_H */
