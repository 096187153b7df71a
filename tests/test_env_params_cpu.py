"""ENV_PARAMS without a GPU: the header against its ctypes mirror, the host-only entry points of include/vine_env_params.h,
the table builder of utils/env_params.py and the per-parameter columns of utils/episodes.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params, episodes
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.load()


@pytest.fixture()
def vcfg(lib):
    c = abi.VineConfig()
    assert lib.vine_config_default(C.byref(c)) == 0
    return c


def _header():
    text = open(os.path.join(REPO, "include", "vine_env_params.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_enum_and_prototypes_equal_the_mirror(lib):
    text = _header()
    body = re.search(r"typedef enum VineEnvParam \{(.*?)\} VineEnvParam;", text, flags=re.S).group(1)
    value, enum = -1, {}
    for item in [i.strip() for i in body.split(",") if i.strip()]:
        name, _, v = [x.strip() for x in item.partition("=")]
        value = int(v) if v else value + 1
        enum[name] = value
    mirror = {k: getattr(abi, k) for k in dir(abi) if k.startswith("VP_")}
    assert enum == mirror and enum["VP_COUNT"] == 28
    # the names are the task YAML's keys, in row order, and cover every row exactly once
    rows = []
    for name in abi.ENV_PARAM_NAMES:
        first, count = abi.ENV_PARAM_ROWS[name]
        assert enum["VP_" + name + ("0" if count > 1 else "")] == first and count in (1, abi.NUM_LINKS)
        rows += list(range(first, first + count))
    assert rows == list(range(abi.VP_COUNT)) and len(abi.ENV_PARAM_ROW_NAMES) == abi.VP_COUNT
    assert abi.ENV_PARAM_ROW_NAMES[abi.VP_FPAM_b0 + 3] == "FPAM_b[3]" and abi.ENV_PARAM_ROW_NAMES[abi.VP_ACTION_DELAY] == "ACTION_DELAY"
    from vine_robot_isaacgymenvs_amd.cfg.defaults import TASK
    env = TASK["Vine5LinkMovingBase"]["env"]
    assert all(name in env for name in abi.ENV_PARAM_NAMES if not name.startswith("FPAM_")) and env["ENV_PARAMS"] == {}
    functions = sorted(set(re.findall(r"\b(vine_[a-z_0-9]+)\s*\(", text)))
    assert functions == sorted(abi.ENV_PARAMS_PROTOTYPES)
    for name in functions:
        assert hasattr(lib, name), name


def test_row_equals_the_configuration_field_by_field(lib, vcfg):
    vcfg.damping, vcfg.rail_d_gain, vcfg.action_delay = 0.031, 0.7, 5
    for j in range(5):
        vcfg.fpam_b[j] = 0.01 * (j + 1)
    row = env_params.config_row(lib, vcfg)
    f32 = lambda v: np.float32(v)      # noqa: E731
    expected = {abi.VP_DAMPING: vcfg.damping, abi.VP_SMOOTHING_ALPHA_INFLATE: vcfg.smoothing_alpha_inflate,
                abi.VP_SMOOTHING_ALPHA_DEFLATE: vcfg.smoothing_alpha_deflate,
                abi.VP_RAIL_VELOCITY_SCALE: vcfg.rail_velocity_scale, abi.VP_RAIL_P_GAIN: vcfg.rail_p_gain,
                abi.VP_RAIL_D_GAIN: vcfg.rail_d_gain, abi.VP_RAIL_ACCELERATION: vcfg.rail_acceleration,
                abi.VP_ACTION_DELAY: 5.0}
    for j in range(5):
        expected[abi.VP_FPAM_K0 + j] = vcfg.fpam_K[j]
        expected[abi.VP_FPAM_C0 + j] = vcfg.fpam_C[j]
        expected[abi.VP_FPAM_b0 + j] = vcfg.fpam_b[j]
        expected[abi.VP_FPAM_B0 + j] = vcfg.fpam_B[j]
    assert sorted(expected) == list(range(abi.VP_COUNT))
    for p, v in expected.items():
        assert row[p] == f32(v), abi.ENV_PARAM_ROW_NAMES[p]
    assert lib.vine_env_params_row(None, (C.c_float * abi.VP_COUNT)()) == abi.ERR_INVALID_ARG


def test_check_accepts_the_row_and_names_each_bad_value(lib, vcfg):
    n = 7
    good = np.repeat(env_params.config_row(lib, vcfg)[:, None], n, axis=1)
    env_params.check_table(lib, vcfg, good)
    edge = good.copy()
    edge[abi.VP_SMOOTHING_ALPHA_INFLATE], edge[abi.VP_SMOOTHING_ALPHA_DEFLATE] = 0.0, 1.0
    edge[abi.VP_ACTION_DELAY, 0], edge[abi.VP_ACTION_DELAY, 1], edge[abi.VP_RAIL_ACCELERATION] = 0, abi.MAX_DELAY, 0.0
    edge[abi.VP_DAMPING, 2], edge[abi.VP_RAIL_P_GAIN, 3] = -0.5, -3.0       # unconstrained rows take any finite value
    env_params.check_table(lib, vcfg, edge)
    bad = [(abi.VP_DAMPING, 3, np.nan), (abi.VP_FPAM_C0 + 4, 6, np.inf), (abi.VP_RAIL_P_GAIN, 0, -np.inf),
           (abi.VP_SMOOTHING_ALPHA_INFLATE, 1, 1.0001), (abi.VP_SMOOTHING_ALPHA_DEFLATE, 2, -0.01),
           (abi.VP_ACTION_DELAY, 5, 2.5), (abi.VP_ACTION_DELAY, 4, abi.MAX_DELAY + 1), (abi.VP_ACTION_DELAY, 0, -1.0),
           (abi.VP_RAIL_ACCELERATION, 6, -1e-3)]
    for p, e, v in bad:
        t = good.copy()
        t[p, e] = v
        rc = lib.vine_env_params_check(C.byref(vcfg), t.ctypes.data, n)
        assert rc == abi.ERR_INVALID_ARG, (p, e, v)
        msg = lib.vine_last_error().decode()
        assert abi.ENV_PARAM_ROW_NAMES[p] + " of env %d " % e in msg, msg
        with pytest.raises(ValueError, match=re.escape(abi.ENV_PARAM_ROW_NAMES[p])):
            env_params.check_table(lib, vcfg, t)
    assert lib.vine_env_params_check(C.byref(vcfg), None, n) == abi.ERR_INVALID_ARG
    assert lib.vine_env_params_check(C.byref(vcfg), good.ctypes.data, 0) == abi.ERR_INVALID_ARG


def test_null_handle(lib):
    assert lib.vine_bind_env_params(None, None) == abi.ERR_INVALID_ARG
    assert lib.vine_env_params_bound(None) == 0


# ----------------------------------------------------------------------------------------------------- build_table
def test_build_table_scalar_range_values_and_product(lib, vcfg):
    n = 70
    base = env_params.config_row(lib, vcfg)
    assert np.array_equal(env_params.build_table({}, vcfg, 3, n, lib=lib), np.repeat(base[:, None], n, axis=1))
    spec = {"DAMPING": [0.01, 0.05],
            "ACTION_DELAY": {"values": [0, 2, 5]},
            "RAIL_P_GAIN": 7.5,
            "FPAM_K": {"values": [0.8, 1.2]},
            "FPAM_B": [0.9, 1.1],
            "FPAM_C": 0.5}
    t = env_params.build_table(spec, vcfg, 3, n, lib=lib)
    assert t.dtype == np.float32 and t.shape == (abi.VP_COUNT, n)
    g = np.arange(n)
    assert t[abi.VP_DAMPING].min() >= np.float32(0.01) and t[abi.VP_DAMPING].max() <= np.float32(0.05)
    assert len(np.unique(t[abi.VP_DAMPING])) > n // 2
    assert np.array_equal(t[abi.VP_ACTION_DELAY], np.float32([0, 2, 5])[g % 3])           # the first `values` key: fastest digit
    assert np.all(t[abi.VP_RAIL_P_GAIN] == np.float32(7.5))
    k = np.float64([0.8, 1.2])[(g // 3) % 2]                                              # the second: the next digit
    for j in range(5):
        assert np.array_equal(t[abi.VP_FPAM_K0 + j], (np.float64(base[abi.VP_FPAM_K0 + j]) * k).astype(np.float32))
        assert np.array_equal(t[abi.VP_FPAM_C0 + j], np.full(n, np.float32(np.float64(base[abi.VP_FPAM_C0 + j]) * 0.5)))
    fac = t[abi.VP_FPAM_B0:abi.VP_FPAM_B0 + 5].astype(np.float64) / base[abi.VP_FPAM_B0:abi.VP_FPAM_B0 + 5, None]
    assert np.allclose(fac, fac[0], rtol=2e-7) and fac.min() >= 0.9 - 1e-6 and fac.max() <= 1.1 + 1e-6 and np.ptp(fac[0]) > 0.05
    # every combination of the two `values` entries recurs every 3 * 2 envs
    combos = {(t[abi.VP_ACTION_DELAY, e], t[abi.VP_FPAM_K0, e]) for e in range(6)}
    assert len(combos) == 6
    assert np.array_equal(t[[abi.VP_ACTION_DELAY, abi.VP_FPAM_K0], :64], t[[abi.VP_ACTION_DELAY, abi.VP_FPAM_K0], 6:70])
    # untouched rows keep the configuration's value
    for p in (abi.VP_SMOOTHING_ALPHA_INFLATE, abi.VP_RAIL_D_GAIN, abi.VP_FPAM_b0 + 2):
        assert np.all(t[p] == base[p])
    assert env_params.varying_rows(t) == sorted([abi.VP_DAMPING, abi.VP_ACTION_DELAY] + list(range(abi.VP_FPAM_K0, abi.VP_FPAM_K0 + 5))
                                                + list(range(abi.VP_FPAM_B0, abi.VP_FPAM_B0 + 5)))


def test_build_table_depends_on_seed_name_and_global_id_only(lib, vcfg):
    spec = {"DAMPING": [0.01, 0.05], "SMOOTHING_ALPHA_INFLATE": [0.6, 0.95], "ACTION_DELAY": {"values": [0, 1, 2]},
            "FPAM_b": {"values": [0.8, 1.0, 1.2, 1.1]}, "RAIL_D_GAIN": [0.0, 0.3]}
    whole = env_params.build_table(spec, vcfg, 11, 70, 0, lib=lib)
    assert np.array_equal(whole, env_params.build_table(spec, vcfg, 11, 70, 0, lib=lib))
    shard = env_params.build_table(spec, vcfg, 11, 35, 35, lib=lib)
    assert np.array_equal(shard, whole[:, 35:70])
    other = env_params.build_table(spec, vcfg, 12, 70, 0, lib=lib)
    assert not np.array_equal(other[abi.VP_DAMPING], whole[abi.VP_DAMPING])
    assert np.array_equal(other[abi.VP_ACTION_DELAY], whole[abi.VP_ACTION_DELAY])          # `values` do not draw
    # two ranged names draw from different streams
    u = (whole[abi.VP_DAMPING] - 0.01) / 0.04
    v = (whole[abi.VP_SMOOTHING_ALPHA_INFLATE] - 0.6) / 0.35
    assert np.abs(u - v).max() > 0.3


def test_action_delay_ranges_are_integers_and_hit_both_ends(lib, vcfg):
    t = env_params.build_table({"ACTION_DELAY": [2, 6]}, vcfg, 5, 4096, lib=lib)
    d = t[abi.VP_ACTION_DELAY]
    assert np.array_equal(d, np.floor(d)) and d.min() == 2 and d.max() == 6
    counts = np.bincount(d.astype(int), minlength=7)[2:]
    assert counts.min() > 4096 / 5 * 0.8          # uniform over the five integers: 819 +- 26 each
    full = env_params.build_table({"ACTION_DELAY": [0, abi.MAX_DELAY]}, vcfg, 5, 4096, lib=lib)[abi.VP_ACTION_DELAY]
    assert full.min() == 0 and full.max() == abi.MAX_DELAY


@pytest.mark.parametrize("spec,exc,word", [
    ({"DAMPNG": 0.02}, ConfigError, "DAMPNG"),
    ({"DAMPING": [0.05, 0.01]}, ConfigError, "DAMPING"),
    ({"DAMPING": [0.01, 0.02, 0.03]}, ConfigError, "DAMPING"),
    ({"RAIL_P_GAIN": "high"}, ConfigError, "RAIL_P_GAIN"),
    ({"RAIL_P_GAIN": {"value": [1.0]}}, ConfigError, "RAIL_P_GAIN"),
    ({"RAIL_P_GAIN": {"values": []}}, ConfigError, "RAIL_P_GAIN"),
    ({"ACTION_DELAY": [0.5, 3]}, ConfigError, "ACTION_DELAY"),
    ({"ACTION_DELAY": [0, 9]}, ValueError, "ACTION_DELAY"),
    ({"ACTION_DELAY": 1.5}, ValueError, "ACTION_DELAY"),
    ({"ACTION_DELAY": {"values": [0, -1]}}, ValueError, "ACTION_DELAY"),
    ({"SMOOTHING_ALPHA_INFLATE": [0.5, 1.5]}, ValueError, "SMOOTHING_ALPHA_INFLATE"),
    ({"SMOOTHING_ALPHA_DEFLATE": -0.1}, ValueError, "SMOOTHING_ALPHA_DEFLATE"),
    ({"RAIL_ACCELERATION": {"values": [8.0, -8.0]}}, ValueError, "RAIL_ACCELERATION"),
    ({"DAMPING": float("nan")}, ValueError, "DAMPING"),
    ({"FPAM_K": float("inf")}, ValueError, "FPAM_K[0]"),
])
def test_build_table_refusals_name_the_parameter(lib, vcfg, spec, exc, word):
    with pytest.raises(exc, match=re.escape(word)):
        env_params.build_table(spec, vcfg, 1, 16, lib=lib)
    assert issubclass(ConfigError, ValueError)


# ------------------------------------------------------------------------------------------- episodes: param columns
def test_with_env_params_and_rates_by_hand(lib, vcfg):
    n = 6
    table = np.repeat(env_params.config_row(lib, vcfg)[:, None], n, axis=1)
    table[abi.VP_ACTION_DELAY] = [0, 2, 0, 2, 0, 2]
    table[abi.VP_DAMPING] = [0.01, 0.02, 0.03, 0.04, 0.05, 0.06]
    table[abi.VP_FPAM_K0:abi.VP_FPAM_K0 + 5, 3] *= 1.5
    env = np.array([0, 1, 2, 3, 4, 5, 1, 1, 3, 0], dtype=np.int64)
    reached = np.array([1, 0, 1, 1, 0, 0, 1, 0, 0, 1], dtype=np.float32)
    rows = {name: np.zeros(len(env), dtype=np.int64 if name in episodes.INT_COLUMNS else np.float32) for name in episodes.COLUMNS}
    rows["env"], rows["reached_ever"] = env, reached
    out = episodes.with_env_params(rows, table, abi.ENV_PARAM_ROW_NAMES)
    assert sorted(k for k in out if k.startswith("param_")) == ["param_ACTION_DELAY", "param_DAMPING", "param_FPAM_K"]
    assert all(np.array_equal(out[k], rows[k]) for k in rows)
    assert np.array_equal(out["param_ACTION_DELAY"], np.float32([0, 2, 0, 2, 0, 2, 2, 2, 2, 0]))
    assert np.array_equal(out["param_FPAM_K"], table[abi.VP_FPAM_K0][env])                  # joint 0 stands for the vector
    # delay 0: envs 0, 2, 4, 0 -> reached 1, 1, 0, 1; delay 2: envs 1, 3, 5, 1, 1, 3 -> 0, 1, 0, 1, 0, 0
    values, rate, count = episodes.value_rate(out, "param_ACTION_DELAY")
    assert values.tolist() == [0.0, 2.0] and count.tolist() == [4, 6] and rate.tolist() == [0.75, 2.0 / 6.0]
    # damping in two bins [0.01, 0.035), [0.035, 0.06]: envs {0, 1, 2} -> episodes 0, 1, 2, 6, 7, 9; envs {3, 4, 5} -> 3, 4, 5, 8
    rate, count, edges = episodes.binned_rate(out, "param_DAMPING", 2)
    assert count.tolist() == [6, 4] and rate.tolist() == [4.0 / 6.0, 0.25]
    assert edges[0] == pytest.approx(0.01) and edges[-1] == pytest.approx(0.06)


def test_npz_and_mat_hold_the_table_only_when_given(lib, vcfg, tmp_path):
    import scipy.io
    from vine_robot_isaacgymenvs_amd.utils import trajectory
    n = 4
    table = np.repeat(env_params.config_row(lib, vcfg)[:, None], n, axis=1)
    table[abi.VP_DAMPING] = [0.01, 0.02, 0.03, 0.04]
    rows = episodes.concat_rows([])
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    episodes.save(a, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {"SUCCESS_DIST": 0.08})
    episodes.save(b, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {"SUCCESS_DIST": 0.08}, table, abi.ENV_PARAM_ROW_NAMES)
    assert episodes.load_env_params(a) == (None, None)
    got, names = episodes.load_env_params(b)
    assert np.array_equal(got, table) and tuple(names) == abi.ENV_PARAM_ROW_NAMES
    assert episodes.load(b)[3] == {"SUCCESS_DIST": 0.08}
    rec = np.zeros((3, abi.RECORD_FIELDS), dtype=np.float32)
    plain = trajectory.trajectory_arrays(rec, [0, 1, 2], 0.0333, env=2)
    assert "env_params" not in plain and "env_param_names" not in plain
    path = trajectory.write_trajectory_mat(str(tmp_path / "t.mat"), rec, [0, 1, 2], 0.0333, 2, table[:, 2].astype(np.float64),
                                           abi.ENV_PARAM_ROW_NAMES)
    mat = scipy.io.loadmat(path)
    assert mat["env_params"].shape == (abi.VP_COUNT, 1) and np.array_equal(mat["env_params"][:, 0], table[:, 2].astype(np.float64))
    assert [str(s[0]) if isinstance(s, np.ndarray) else str(s).strip() for s in mat["env_param_names"].ravel()] == \
        list(abi.ENV_PARAM_ROW_NAMES)
    assert set(plain) <= set(mat)


# ------------------------------------------------------------------------- the nine plants of the GPU tests, on the oracle
def test_oracle_is_finite_and_within_tolerance_on_every_parameter_set(lib):
    """tests/env_params_sets.py: on each of the nine sets the oracle's float32 build stays finite and within the tolerances
    the GPU tests hold the kernel to against its float64 build -- one step from a random mid-episode state at
    single_step_case's float64 tolerances, then 40 steps at test_trajectory_tracks_oracle's -- so a miss on the GPU is the
    kernel's, not the ranges'.  All 28 rows differ between any two sets."""
    from oracle import vine_oracle as vo
    from tests.env_params_sets import NUM_SETS, set_cfg, set_rows
    from tests.helpers import base_cfg, random_state
    from tests.test_hip_parity import QPOS, compare_step
    n, T = 70, 40
    cfg0 = base_cfg(n, randomize=True, max_episode_length=12, seed=77)
    rows = set_rows(lib, cfg0)
    for a in range(NUM_SETS):
        for b in range(a + 1, NUM_SETS):
            assert np.all(rows[a] != rows[b]), (a, b)
    assert rows[:, abi.VP_ACTION_DELAY].tolist() == list(range(NUM_SETS))
    env_params.check_table(lib, cfg0, np.ascontiguousarray(rows.T))
    for g in range(NUM_SETS):
        cfg = set_cfg(cfg0, g)
        cfg.obs_noise_std, cfg.action_noise_std, cfg.dyn_scale_min, cfg.dyn_scale_max = 0.01, 0.02, 0.9, 1.1
        rng = np.random.default_rng(100 + g)
        lo, hi = vo.OracleEnv(cfg, "f32"), vo.OracleEnv(cfg, "f64")
        st = random_state(rng, n, cfg)
        reset = (rng.uniform(size=n) < 0.15).astype(np.int64)
        progress = rng.integers(0, cfg.max_episode_length - 1, n)
        progress[: n // 16] = cfg.max_episode_length - 2
        for o in (lo, hi):
            o.state[:] = st.astype(o.real)
            o.reset_buf[:], o.progress[:], o.step_count = reset, progress, 7
        actions = rng.uniform(-1.3, 1.3, (n, 2))
        lo.step(actions); hi.step(actions)
        assert np.isfinite(lo.state).all() and np.isfinite(lo.obs).all()
        compare_step((lo.obs, lo.rew, lo.reset_buf, lo.timeouts), hi, lo, 1e-4, 1e-2, 1e-2)
        lo.close(); hi.close()
        cfg = set_cfg(cfg0, g)
        lo, hi = vo.OracleEnv(cfg, "f32"), vo.OracleEnv(cfg, "f64")
        mismatched, worst_q = np.zeros(n, bool), 0.0
        for t in range(T):
            a = rng.uniform(-1, 1, (n, 2))
            lo.step(a); hi.step(a)
            mismatched |= lo.reset_buf != hi.reset_buf
            ok = ~mismatched
            assert np.isfinite(lo.state).all()
            worst_q = max(worst_q, np.abs(lo.state[QPOS][:, ok].astype(np.float64) - hi.state[QPOS][:, ok]).max())
            np.testing.assert_allclose(lo.obs[ok], hi.obs[ok], rtol=0, atol=2e-2)
            np.testing.assert_allclose(lo.rew[ok], hi.rew[ok], rtol=1e-4, atol=5e-3)
            np.testing.assert_array_equal(lo.progress[ok], hi.progress[ok])
        print("set %d: mismatched %d of %d, worst |dq| %.3g" % (g, mismatched.sum(), n, worst_q))
        assert mismatched.mean() < 0.02 and worst_q < 5e-3
        lo.close(); hi.close()
