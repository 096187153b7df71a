"""Nine plants for the ENV_PARAMS tests: parameter set ``g`` (0..8) differs from every other set in all 28 table rows, its
action delay is ``g`` itself.  Ranges: joint damping 0.01 .. 0.05, FPAM factors 0.8 .. 1.2 (one factor per row), smoothing
constants 0.6 .. 0.95, rail velocity scale / P gain / acceleration +-30 % of the task YAML's, rail D gain 0 .. 0.4 (the YAML's
is 0).  Each row walks its range in its own order (``g * k mod 9`` with k coprime to 9), so no two rows rise together.
tests/test_env_params_cpu.py checks that the oracle's float32 and float64 builds stay within the parity tolerances of
tests/test_hip_parity.py on every one of them."""
import ctypes as C

import numpy as np

from vine_robot_isaacgymenvs_amd import abi

NUM_SETS = 9
_STRIDES = (1, 2, 4, 5, 7, 8)


def _lin(lo, hi, g, row):
    return lo + (hi - lo) * ((g * _STRIDES[row % len(_STRIDES)]) % NUM_SETS) / (NUM_SETS - 1.0)


def apply_set(cfg, g):
    """Write parameter set ``g`` into a VineConfig (the uniform handles and the oracles are created from it)."""
    base = type(cfg).from_buffer_copy(cfg)
    cfg.action_delay = int(g)
    cfg.damping = _lin(0.01, 0.05, g, 0)
    cfg.smoothing_alpha_inflate = _lin(0.6, 0.95, g, 1)
    cfg.smoothing_alpha_deflate = _lin(0.6, 0.95, g, 2)
    cfg.rail_velocity_scale = base.rail_velocity_scale * _lin(0.7, 1.3, g, 3)
    cfg.rail_p_gain = base.rail_p_gain * _lin(0.7, 1.3, g, 4)
    cfg.rail_d_gain = _lin(0.0, 0.4, g, 5)
    cfg.rail_acceleration = base.rail_acceleration * _lin(0.7, 1.3, g, 6)
    for k, field in enumerate(("fpam_K", "fpam_C", "fpam_b", "fpam_B")):
        for j in range(abi.NUM_LINKS):
            getattr(cfg, field)[j] = getattr(base, field)[j] * _lin(0.8, 1.2, g, 8 + 5 * k + j)
    return cfg


def set_cfg(cfg, g):
    """A copy of ``cfg`` holding parameter set ``g``."""
    return apply_set(type(cfg).from_buffer_copy(cfg), g)


def set_rows(lib, cfg):
    """float32 [NUM_SETS, VP_COUNT]: ``vine_env_params_row`` of every set's configuration."""
    rows = np.zeros((NUM_SETS, abi.VP_COUNT), dtype=np.float32)
    for g in range(NUM_SETS):
        row = (C.c_float * abi.VP_COUNT)()
        assert lib.vine_env_params_row(C.byref(set_cfg(cfg, g)), row) == 0
        rows[g] = np.array(row, dtype=np.float32)
    return rows


def table_of(lib, cfg, n):
    """The heterogeneous table [VP_COUNT, n]: env ``e`` carries set ``e % 9``."""
    return np.ascontiguousarray(set_rows(lib, cfg)[np.arange(n) % NUM_SETS].T)
