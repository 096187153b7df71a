/*
 * vine_env_inertia.h — per-env cart and link masses of the env step (extension of include/vine_env_params.h; product library
 * only).
 *
 * The parameter table of vine_env_params.h gives every env its own damping, FPAM constants, smoothing, rail controller and
 * delay.  This second table gives every env its own cart mass, link masses and link inertias about the COM: the first
 * parameters that differ between a URDF and a built robot (a carriage on the cart, tubing, a camera or a gripper on a link).
 * It is a table of its own, [VI_COUNT][num_envs] floats in device memory, struct-of-arrays like the first (row r of env e at
 * table[r * num_envs + e]), so that the first table keeps its 28 rows.
 *
 * The step does not read masses.  It reads the constant coefficients of the absolute-angle Lagrangian that the host forms
 * from them in double: mtot, b_i, g b_i, a_ii and a_i0 = L b_i (every a_ij with j < i equals L b_i).  So the table holds
 * both: 11 PRIMARY rows, what a user states, and 20 DERIVED rows, what the kernel reads.  vine_env_inertia_derive fills the
 * derived rows from the primary ones with the very statement vine_create uses for the handle's own constants, so a uniform
 * handle and a table column of the same float32 masses hold identical bits.  vine_env_inertia_check refuses a table whose
 * derived rows are not what derive gives: the kernel never sees coefficients that no set of masses produces.
 *
 * The link inertias are read by the step directly only where joint stiffness or link angular damping is switched on (the
 * term cad * I_i * w_i); everywhere else they enter through a_ii.
 *
 * A table is read by the one-lane-per-env kernel only and needs a bound parameter table (vine_bind_env_params): the step
 * kernel then has three variants -- no table, the parameter table, both -- instead of four.
 *
 * What still cannot be overridden per env, and why:
 *   - link length, COM offset, joint1_z, phi0: they reach the kinematics, the contact geometry, the renderer and the
 *     recorder, which take them from the handle;
 *   - gravity and dt: they are per-launch constants of the substep (and dt of the observation's finite differences);
 *   - STIFFNESS, the link angular damping and the physics-mode flags: they select code paths of the whole launch.
 */
#ifndef VINE_ENV_INERTIA_H
#define VINE_ENV_INERTIA_H

#include "vine_env_params.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows of the table.  Primary: the VineConfig's cart_mass, link_mass[5], link_inertia[5].  Derived (i = link 0..4):
 * MTOT = cart + sum m_i;  B_i = m_i l + L sum_{k>i} m_k;  GB_i = g B_i;  ADIAG_i = m_i l^2 + L^2 sum_{k>i} m_k + I_i;
 * AOFF_i = L B_i for i = 1..4 (row VI_AOFF1 + i - 1), with L = link_length, l = link_com, g = gravity of the handle. */
typedef enum VineEnvInertia {
    VI_CART_MASS = 0,
    VI_LINK_MASS0 = 1,              /* links 0..4 at VI_LINK_MASS0 + i, kg, > 0 */
    VI_LINK_INERTIA0 = 6,           /* about the link's COM, kg m^2, >= 0 */
    VI_PRIMARY_COUNT = 11,
    VI_MTOT = 11,
    VI_B0 = 12,
    VI_GB0 = 17,
    VI_ADIAG0 = 22,
    VI_AOFF1 = 27,                  /* links 1..4 at VI_AOFF1 + i - 1 */
    VI_COUNT = 31
} VineEnvInertia;

/* Host only.  row[r] = the configuration's own value of row r, primary and derived: a table filled with this row in every
 * column reproduces the handle without a table, bit for bit. */
int vine_env_inertia_row(const VineConfig* cfg, float row[VI_COUNT]);

/* Host only.  host_table: [VI_COUNT][num_envs] floats in host memory.  Fills the derived rows of every column from its
 * primary rows and cfg's link_length, link_com and gravity, in double, rounded once to float. */
int vine_env_inertia_derive(const VineConfig* cfg, float* host_table, int num_envs);

/* Host only.  Every value finite, every mass > 0, every inertia >= 0, and the derived rows equal to what
 * vine_env_inertia_derive gives for the primary rows (bit for bit); otherwise VINE_ERR_INVALID_ARG, and vine_last_error()
 * names the row and the env. */
int vine_env_inertia_check(const VineConfig* cfg, const float* host_table, int num_envs);

/* Bind a table on the handle's device: [VI_COUNT][cfg.num_envs] floats, borrowed; NULL unbinds.  Ownership, rewriting
 * between steps and replay of a captured graph follow vine_bind_env_params: the contents are the caller's to check and may
 * be rewritten between steps, and a captured step reads whatever the table holds at replay.  A parameter table must be bound
 * already (VINE_ERR_UNSUPPORTED otherwise), and while an inertia table is bound vine_bind_env_params(h, NULL) is refused
 * with VINE_ERR_UNSUPPORTED: unbind the inertia table first.  Binding changes neither the kernel nor its grid. */
int vine_bind_env_inertia(VineHandle* h, const float* device_table);

/* 1 while a table is bound, else 0 (0 for a NULL handle). */
int vine_env_inertia_bound(VineHandle* h);

#ifdef __cplusplus
}
#endif
#endif /* VINE_ENV_INERTIA_H */
