/*
 * vine_mpc_adapt_inertia.h — C ABI of the mass dimensions of online model adaptation (extension of vine_mpc_adapt.h), for
 * MI355X (gfx950): the belief of the adaptive controller carries up to three more dimensions -- the cart's mass, a factor on
 * the five link masses and inertias, a further factor on the tip link's -- whose candidates and planning value live in the
 * model's per-env inertia table (vine_env_inertia.h), derived rows included, formed on the device.
 *
 * Only libvine_hip.so exports this header.  Errors, streams and ownership as in vine_mpc_adapt.h: 0 = ok, negative =
 * VineStatus, message via vine_last_error(); both entry points enqueue on the caller's stream and do not synchronise,
 * allocate nothing and use no atomics; the caller owns every buffer.  The five launches of vine_mpc_adapt.h are not touched:
 * the two launches here stand beside them, and nothing that changes from step to step is a kernel argument, so both replay
 * from a captured hipGraph.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * HANDLES.  The MODEL handle of vine_mpc_adapt.h (N = M * K envs) with, beside its parameter table, an inertia table bound
 * (vine_bind_env_inertia).  Both launches take that very memory as `inertia_table` and WRITE it, as
 * vine_env_redraw_scheduled does; a handle without a bound inertia table, or one bound to other memory than the one passed,
 * is refused (VINE_ERR_UNSUPPORTED).  The VineMpcAdaptConfig passed beside the VineMpcAdaptInertiaConfig is the base
 * controller's own: what vine_mpc_adapt.h refuses of it is refused here in the same words.
 *
 * DIMENSIONS.  The mass belief has Dm = num_mass_dims dimensions (1 .. 3), each {name, lo, hi, std_floor} with 0 < lo <= hi:
 *   VINE_MPC_ADAPT_INERTIA_CART  the cart's mass, kg;
 *   VINE_MPC_ADAPT_INERTIA_LINK  a factor on the model configuration's five link masses and inertias (base_inertia);
 *   VINE_MPC_ADAPT_INERTIA_TIP   a further factor on link 4's.
 * These are the semantics of the ENV_PARAMS names CART_MASS, LINK_MASS and TIP_LINK_MASS.  A repeated or unknown name is
 * refused.
 *
 * STATE.  The caller's, on the handle's device:
 *   mass_mean[M][Dm], mass_std[M][Dm]               float64   the mass belief
 *   mass_prior_mean[M][Dm], mass_prior_std[M][Dm]   float64   what it returns to when it forgets
 * passes[M], err[N], trace_len[M] and episode_ended[M] are those of vine_mpc_adapt.h.
 *
 * CANDIDATES.  The value of sample e = p * K + j in mass dimension i during pass passes[p] is
 *   theta = min(max(mass_mean[p][i] + (double)z * mass_std[p][i], lo_i), hi_i)
 * in float64, one multiply, one add, no contraction; z is the deviate of vine_mpc_adapt.h under the same purpose word
 * VINE_MPC_ADAPT_RNG and the same key, with the counter
 *   (p * K + j, (unsigned)passes[p], VINE_MPC_ADAPT_RNG | (passes[p] >> 32) << 8, VINE_MPC_ADAPT_MAX_DIMS + i)
 * so that the mass dimensions' streams are apart from the table dimensions' (whose last word is d < VINE_MPC_ADAPT_MAX_DIMS).
 * Candidate 0 of every plant has z = 0.  An absent name has theta = 1, or base_inertia[VI_CART_MASS] for the cart.
 *
 * THE COLUMN of a set of thetas.  Primary rows: VI_CART_MASS = float32(theta_cart) (the base's own float where the cart is
 * absent); with f = theta_link for links 0 .. 3 and f = theta_link * theta_tip (one float64 multiply) for link 4,
 *   VI_LINK_MASS0 + i    = float32((double)base_inertia[VI_LINK_MASS0 + i] * f)
 *   VI_LINK_INERTIA0 + i = float32((double)base_inertia[VI_LINK_INERTIA0 + i] * f)
 * the rounding of env_params.set_inertia_rows: a candidate whose theta is a plant's drawn value holds that plant's bits.
 * The 20 derived rows are the composites of those float32 primaries with link_length, link_com and gravity, accumulated in
 * double without contraction and rounded once: the statement vine_env_inertia_derive makes, so every written column passes
 * vine_env_inertia_check.
 *
 * 1. THE PIN.  vine_mpc_adapt_inertia_pin, one lane per model env, 256 per workgroup, enqueued directly behind
 * vine_mpc_adapt_pin (which does not read the inertia table; the W model steps that follow do).  The lane writes the 11
 * primary and 20 derived rows of its candidate's column.  No LDS, no atomics; a lane is the only writer of its column.
 *
 * 2. THE ESTIMATE.  vine_mpc_adapt_inertia_estimate, one workgroup of VINE_MPC_THREADS lanes per plant, enqueued IN FRONT OF
 * vine_mpc_adapt_estimate, so that passes[p] is still the pin's.  It makes the estimate of vine_mpc_adapt.h (5) for the mass
 * dimensions: the same three cases in the same order (forget; belief unchanged; update), the same beta, ebar, tau and w_j
 * from the same err, the same reduction order (lane t goes through j = t, t + 256, .. in ascending j; a butterfly over each
 * wave; the four wave values through LDS, combined in wave order), the same update of mean and std with the floor.  No
 * atomics: two runs give the same bits.  In every case the planning value -- the column of the new mean clamped to the
 * ranges, the candidates' statement at z = 0 -- is then written into the inertia columns of all K samples of p.  passes is
 * only read: the base estimate behind this launch increments it.  Where `weights` is given, w_j of every sample is stored
 * (0 where the belief was not estimated).
 * ---------------------------------------------------------------------------------------------------------------------
 */
#ifndef VINE_MPC_ADAPT_INERTIA_H
#define VINE_MPC_ADAPT_INERTIA_H

#include <stdint.h>

#include "vine.h"
#include "vine_env_inertia.h"
#include "vine_mpc_adapt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VINE_MPC_ADAPT_INERTIA_ABI_VERSION 1
#define VINE_MPC_ADAPT_INERTIA_MAX_DIMS 3
#define VINE_MPC_ADAPT_INERTIA_CART 0
#define VINE_MPC_ADAPT_INERTIA_LINK 1
#define VINE_MPC_ADAPT_INERTIA_TIP 2

typedef struct VineMpcAdaptInertiaDim {
    int32_t name;          /* VINE_MPC_ADAPT_INERTIA_CART, _LINK or _TIP */
    int32_t reserved;      /* 0 */
    double lo;             /* 0 < lo <= hi, both finite */
    double hi;
    double std_floor;      /* >= 0, finite */
} VineMpcAdaptInertiaDim;

typedef struct VineMpcAdaptInertiaConfig {
    int32_t abi_version;       /* must be VINE_MPC_ADAPT_INERTIA_ABI_VERSION */
    int32_t num_mass_dims;     /* Dm; 1 .. VINE_MPC_ADAPT_INERTIA_MAX_DIMS; the caller sets it (default 0) */
    VineMpcAdaptInertiaDim dims[VINE_MPC_ADAPT_INERTIA_MAX_DIMS];
    float base_inertia[VI_PRIMARY_COUNT];   /* the MODEL configuration's vine_env_inertia_row() primaries; masses > 0 */
    float link_length;         /* the model configuration's; > 0 (the handle does not expose them to an observer) */
    float link_com;            /* > 0 */
    float gravity;             /* finite */
} VineMpcAdaptInertiaConfig;

int vine_mpc_adapt_inertia_config_default(VineMpcAdaptInertiaConfig* cfg);
int vine_mpc_adapt_inertia_config_size(void);    /* sizeof(VineMpcAdaptInertiaConfig): checked by the ctypes mirror */

/* See 1. THE PIN.  inertia_table: float[VI_COUNT][N], the table bound to `model`. */
int vine_mpc_adapt_inertia_pin(VineHandle* model, const VineMpcAdaptConfig* cfg, const VineMpcAdaptInertiaConfig* icfg,
                               float* inertia_table, const double* mass_mean, const double* mass_std, const int64_t* passes,
                               void* stream);

/* See 2. THE ESTIMATE.  weights: double[N] or NULL. */
int vine_mpc_adapt_inertia_estimate(VineHandle* model, const VineMpcAdaptConfig* cfg, const VineMpcAdaptInertiaConfig* icfg,
                                    float* inertia_table, const double* err, const int32_t* trace_len,
                                    const uint8_t* episode_ended, double* mass_mean, double* mass_std,
                                    const double* mass_prior_mean, const double* mass_prior_std, const int64_t* passes,
                                    double* weights, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VINE_MPC_ADAPT_INERTIA_H */
