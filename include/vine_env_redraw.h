/*
 * vine_env_redraw.h — a new plant for every episode (ENV_PARAMS_PER_EPISODE; extension of include/vine_env_params.h and
 * include/vine_env_inertia.h; product library only).
 *
 * The tables of those two headers give every env its own plant, drawn once.  vine_env_redraw_scheduled is a launch behind
 * every step (a step observer, like vine_episodes_scheduled) that rewrites the columns of the envs whose reset flag the step
 * has just raised, so that the next step -- the one that consumes the reset -- already reads the new plant.  The step
 * kernels are not touched: they read the bound tables as before, and vine_reset_env reads no overridable field.
 *
 * The draw is a pure function of (seed, name, global env id, episode): with mix = splitmix64's finaliser,
 *     pre = mix(seed ^ key(name)) + g * 0x9E3779B97F4A7C15
 *     h_k = mix(pre ^ mix(k))                 (mix(0) == 0: episode 0 is the draw the tables were built from)
 *     u   = (h_k >> 11) * 2^-53
 * and the value of a name follows from u by its form: a number is itself; [lo, hi] gives lo + (hi - lo) * u, for ACTION_DELAY
 * min(lo + floor(u * (hi - lo + 1)), hi); a value list gives values[min(floor(u * count), count - 1)] from episode 1 on and
 * values[(g / radix) % count] at episode 0.  Everything is formed in float64 and rounded once to the table's float32, and
 * the derived rows of the inertia table by the very statement vine_env_inertia_derive uses: the kernel's translation unit is
 * built without floating-point contraction, so a column holds the bits the host (utils/env_params.py draw_columns) gives.
 *
 * The kernel: one lane per env, 256 lanes per workgroup, no LDS, no atomics.  Nothing that changes from step to step is an
 * argument, so a launch captured in a hipGraph replays correctly.  A lane whose reset[e] == 0 loads that one word and
 * leaves.  A lane whose flag is set
 *   - increments episode_index[e] and draws episode k = episode_index[e] of global env env_id_offset + e;
 *   - writes the rows of every name of the spec into the parameter table (rows of absent names are never written);
 *   - with an inertia table, writes its 11 primary rows and re-derives its 20 derived rows;
 *   - if the env's ACTION_DELAY changed, zeroes the env's ring of delayed actions in the state block (VF_FIFO0 ..
 *     VF_FIFO0 + 2 * VINE_MAX_DELAY - 1), which is what a fresh handle holds: the step indexes the ring by
 *     `global step % delay`, so slots ordered under one modulus mean nothing under another, and slots beyond the old delay
 *     can be arbitrarily old.  An unchanged delay leaves the ring alone, as a reset does.  Nothing else of the state block is
 *     written.
 * Envs reset from outside the step (vine_reset_idx) raise no flag and keep their plant; this matches the episode log, which
 * writes no row for them.
 */
#ifndef VINE_ENV_REDRAW_H
#define VINE_ENV_REDRAW_H

#include "vine_env_inertia.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_ENV_REDRAW_ABI_VERSION 1
#define VINE_ENV_REDRAW_THREADS 256

/* The names of a spec, in this order: the twelve of the parameter table, then the three of the inertia table. */
typedef enum VineEnvRedrawSlot {
    VR_DAMPING = 0, VR_SMOOTHING_ALPHA_INFLATE, VR_SMOOTHING_ALPHA_DEFLATE, VR_RAIL_VELOCITY_SCALE, VR_RAIL_P_GAIN, VR_RAIL_D_GAIN,
    VR_RAIL_ACCELERATION, VR_ACTION_DELAY, VR_FPAM_K, VR_FPAM_C, VR_FPAM_b, VR_FPAM_B,      /* FPAM: a factor on the base's five */
    VR_CART_MASS,                   /* kg */
    VR_LINK_MASS,                   /* factor on the base's five link masses and inertias */
    VR_TIP_LINK_MASS,               /* further factor on link 4's */
    VR_NAMES = 15
} VineEnvRedrawSlot;

typedef enum VineEnvRedrawForm {
    VINE_REDRAW_ABSENT = 0,         /* the name is not in the spec: its rows are not written */
    VINE_REDRAW_NUMBER = 1,         /* lo */
    VINE_REDRAW_RANGE = 2,          /* [lo, hi] */
    VINE_REDRAW_VALUES = 3          /* values[values_first .. values_first + values_count - 1] */
} VineEnvRedrawForm;

typedef struct VineEnvRedrawName {
    int32_t form;                   /* VineEnvRedrawForm */
    int32_t values_first;           /* extent of the name's list in the values array */
    int32_t values_count;
    int32_t reserved;               /* must be 0 */
    uint64_t key;                   /* 64-bit key of the name (the first 8 bytes of its SHA-256, little endian) */
    uint64_t radix;                 /* value lists at episode 0: the product of the counts of the lists before this one */
    double lo, hi;
} VineEnvRedrawName;

typedef struct VineEnvRedrawSpec {
    int32_t abi_version;            /* VINE_ENV_REDRAW_ABI_VERSION */
    int32_t num_values;             /* doubles in the values array */
    uint64_t seed;
    const double* values;           /* DEVICE array of the value lists, the caller's; may be NULL when num_values == 0 */
    VineEnvRedrawName name[VR_NAMES];
    float base_params[VP_COUNT];                /* vine_env_params_row of the configuration */
    float base_inertia[VI_PRIMARY_COUNT];       /* the primary rows of vine_env_inertia_row */
    float link_length, link_com, gravity;
    uint32_t checked;               /* set by vine_env_redraw_spec; vine_env_redraw_scheduled refuses a spec without it */
    uint32_t reserved;
} VineEnvRedrawSpec;

int vine_env_redraw_spec_size(void);

/* Host only.  Fills *out from the configuration (base rows, link_length, link_com, gravity, seed), the caller's per-name
 * entries and the value lists: host_values (num_values doubles, read for the check) and device_values (the same numbers in
 * device memory, borrowed while the spec is used; only stored).  Everything the spec CAN give an env -- both ends of a
 * range, every listed value, the number -- is formed into columns exactly as the kernel forms them and put through
 * vine_env_params_check and vine_env_inertia_check, so the kernel never writes a column those would refuse; a refusal is
 * theirs (VINE_ERR_INVALID_ARG, vine_last_error() names the parameter).  Also refused: an unknown form, lo > hi or a
 * non-integer end for ACTION_DELAY's range, an extent outside the values array. */
int vine_env_redraw_spec(const VineConfig* cfg, const VineEnvRedrawName names[VR_NAMES], const double* host_values,
                         const double* device_values, int num_values, VineEnvRedrawSpec* out);

/* Enqueue the redraw behind the step just enqueued on `stream`.  reset: the step's reset buffer (int64 [N]); params_table
 * and inertia_table: the caller's WRITABLE buffers, the very memory bound to the handle with vine_bind_env_params /
 * vine_bind_env_inertia (the handle keeps its const view); inertia_table may be NULL when the spec names none of the three
 * mass names; episode_index: device int32 [N], zeroed by the caller before the first step.
 * VINE_ERR_INVALID_ARG: a null pointer; a spec vine_env_redraw_spec did not fill; no parameter table bound to the handle, or
 * another one than params_table; mass names in the spec with no inertia table bound (or another one than inertia_table). */
int vine_env_redraw_scheduled(VineHandle* h, const VineEnvRedrawSpec* spec, const int64_t* reset, float* params_table,
                              float* inertia_table, int32_t* episode_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_ENV_REDRAW_H */
