"""Nine plants for the ENV_INERTIA tests: mass set ``g`` (0..8) differs from every other set in the cart's mass and in every
link's mass and inertia.  Each of the eleven values is the configuration's times a factor in 0.7 .. 1.4 that walks the range
in the row's own order (``g * k mod 9`` with k coprime to 9, offset by the row), so no two rows rise together and the
inertias do not follow the masses: the derived rows (include/vine_env_inertia.h) are exercised off the line ``LINK_MASS``
scales along.  The cart's factor stays within 0.8 .. 1.4: with the task YAML's rail controller a cart of 0.7 times the
configuration's 0.4 kg diverges in the oracle's float64 build itself within 30 steps (0.75 times does not), which is the
plant's doing and nothing a parity test can hold a kernel to.  tests/test_env_inertia_cpu.py checks that the oracle's
float32 and float64 builds stay within the parity tolerances of tests/test_hip_parity.py on every one of them."""
import ctypes as C

import numpy as np

from vine_robot_isaacgymenvs_amd import abi

NUM_SETS = 9
_STRIDES = (1, 2, 4, 5, 7, 8)
LO, HI = 0.7, 1.4
CART_LO = 0.8


def factor(g, row):
    """The factor of mass set ``g`` on primary row ``row`` (0 = cart, 1..5 link masses, 6..10 link inertias)."""
    k = (g * _STRIDES[row % len(_STRIDES)] + row) % NUM_SETS
    lo = CART_LO if row == abi.VI_CART_MASS else LO
    return lo + (HI - lo) * k / (NUM_SETS - 1.0)


def apply_set(cfg, g):
    """Write mass set ``g`` into a VineConfig (the uniform handles and the oracles are created from it)."""
    base = type(cfg).from_buffer_copy(cfg)
    cfg.cart_mass = base.cart_mass * factor(g, abi.VI_CART_MASS)
    for i in range(abi.NUM_LINKS):
        cfg.link_mass[i] = base.link_mass[i] * factor(g, abi.VI_LINK_MASS0 + i)
        cfg.link_inertia[i] = base.link_inertia[i] * factor(g, abi.VI_LINK_INERTIA0 + i)
    return cfg


def set_cfg(cfg, g):
    """A copy of ``cfg`` holding mass set ``g``."""
    return apply_set(type(cfg).from_buffer_copy(cfg), g)


def set_rows(lib, cfg):
    """float32 [NUM_SETS, VI_COUNT]: ``vine_env_inertia_row`` of every set's configuration."""
    rows = np.zeros((NUM_SETS, abi.VI_COUNT), dtype=np.float32)
    for g in range(NUM_SETS):
        row = (C.c_float * abi.VI_COUNT)()
        assert lib.vine_env_inertia_row(C.byref(set_cfg(cfg, g)), row) == 0
        rows[g] = np.array(row, dtype=np.float32)
    return rows


def table_of(lib, cfg, n):
    """The heterogeneous table [VI_COUNT, n]: env ``e`` carries set ``e % 9``."""
    return np.ascontiguousarray(set_rows(lib, cfg)[np.arange(n) % NUM_SETS].T)
