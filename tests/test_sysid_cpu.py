"""SYSID without a GPU: the C ABI of include/vine_sysid.h against its ctypes mirror, the refusal of bad configurations, the
MAT reader against the recorder's writer, the window arithmetic on a hand-made log, and the search against a fake
evaluator."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params, sysid
from vine_robot_isaacgymenvs_amd.utils.trajectory import trajectory_arrays, write_trajectory_mat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(REPO, "include", "vine_sysid.h")).read()


@pytest.fixture(scope="module")
def hip_lib():
    native.build()
    return native.load()


def _scfg(lib, **over):
    c = abi.VineSysidConfig()
    assert lib.vine_sysid_config_default(c) == abi.OK
    c.num_rows = 40
    c.horizon = 12
    for k, v in over.items():
        if k == "weights":
            for i, x in enumerate(v):
                c.weights[i] = x
        else:
            setattr(c, k, v)
    return c


# --------------------------------------------------------------------------------------------------------------- ABI
def test_sysid_header_and_ctypes_mirror_agree(hip_lib):
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(vine_sysid_[a-z_0-9]+)\s*\(", code)))
    assert names == sorted(abi.SYSID_PROTOTYPES) and len(names) == 4
    for name in names:
        assert hasattr(hip_lib, name), name
    assert hip_lib.vine_sysid_config_size() == C.sizeof(abi.VineSysidConfig) == 16 + 4 * 16
    body = re.search(r"typedef struct VineSysidConfig \{(.*?)\}", code, re.S).group(1)
    fields = re.findall(r"^\s+(?:int32_t|float)\s+([a-z_]+)(?:\[[A-Z_]+\])?;", body, re.M)
    assert fields == [n for n, _ in abi.VineSysidConfig._fields_]
    for macro, value in (("ABI_VERSION", abi.SYSID_ABI_VERSION), ("FIELDS", abi.SYSID_FIELDS)):
        assert int(re.search(r"#define VINE_SYSID_%s (\d+)" % macro, text).group(1)) == value
    assert abi.SYSID_FIELDS == abi.VRF_TIP_VZ + 1
    # the number of arguments of the two device entry points, from the declarations themselves
    for name in ("vine_sysid_pin", "vine_sysid_scheduled"):
        decl = re.search(r"int %s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(abi.SYSID_PROTOTYPES[name][1]), name
    # out of vine.h: the CPU oracle exports every symbol of that header
    assert "vine_sysid" not in open(os.path.join(REPO, "include", "vine.h")).read()
    assert not set(abi.SYSID_PROTOTYPES) & set(abi.PROTOTYPES)
    # the fingerprint of the library covers the new source and headers
    deps = [os.path.basename(d) for d in native.DEPS]
    assert "vine_sysid.hip" in deps and "vine_sysid.h" in deps and "vine_task_shared.h" in deps


def test_sysid_defaults(hip_lib):
    c = abi.VineSysidConfig()
    assert hip_lib.vine_sysid_config_default(c) == abi.OK
    assert (c.abi_version, c.num_rows, c.horizon, c.reserved) == (1, 0, 50, 0)
    assert list(c.weights) == [1.0] * 6 + [0.0] * 10 == list(sysid.DEFAULT_WEIGHTS)
    assert hip_lib.vine_sysid_config_default(None) == abi.ERR_INVALID_ARG


@pytest.mark.parametrize("over, word", [(dict(abi_version=7), b"abi_version"), (dict(reserved=1), b"reserved"),
                                        (dict(num_rows=1), b"num_rows"), (dict(horizon=0), b"horizon"),
                                        (dict(horizon=40), b"horizon"), (dict(weights=[-1.0]), b"weights"),
                                        (dict(weights=[float("nan")]), b"weights")])
def test_sysid_refuses_bad_configs(hip_lib, over, word):
    """Validation comes before the handle or any pointer is looked at, so no device is needed to see it."""
    bad = _scfg(hip_lib, **over)
    for fn, args in ((hip_lib.vine_sysid_pin, (None, bad, None, 0) + (None,) * 6),
                     (hip_lib.vine_sysid_scheduled, (None, bad) + (None,) * 7)):
        hip_lib.vine_set_step_count(None, -1)             # leaves another message behind
        assert fn(*args) == abi.ERR_INVALID_ARG
        assert word in hip_lib.vine_last_error()


def test_sysid_refuses_null_pointers(hip_lib):
    good = _scfg(hip_lib)
    assert hip_lib.vine_sysid_pin(None, good, None, 0, *([None] * 6)) == abi.ERR_INVALID_ARG
    assert b"null argument to vine_sysid_pin" in hip_lib.vine_last_error()
    assert hip_lib.vine_sysid_scheduled(None, good, *([None] * 7)) == abi.ERR_INVALID_ARG
    assert b"null argument to vine_sysid_scheduled" in hip_lib.vine_last_error()


# ---------------------------------------------------------------------------------------------------------- the log
def _made_up_rows(T=9, seed=0):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((T, abi.RECORD_FIELDS)).astype(np.float32)
    rows[:, abi.VRF_RESET] = 0
    rows[:, abi.VRF_TIMEOUT] = 0
    rows[:, abi.VRF_PROGRESS] = np.arange(T)
    rows[:, abi.VRF_RESERVED0:] = 0
    return rows


def test_load_log_inverts_trajectory_arrays(tmp_path):
    """Every column of a made-up table survives the MAT file bit for bit (float32 -> float64 -> float32 is exact)."""
    rows = _made_up_rows()
    rows[4, abi.VRF_RESET] = 1
    rows[4, abi.VRF_TIMEOUT] = 1
    path = write_trajectory_mat(str(tmp_path / "t.mat"), rows, np.arange(len(rows)), 0.03332, env=3)
    back = sysid.load_log(path, [1.0] * abi.SYSID_FIELDS)
    assert back.dtype == np.float32 and back.shape == rows.shape
    assert np.array_equal(back.view(np.int32), rows.view(np.int32))


def test_load_log_required_and_optional_keys(tmp_path):
    import scipy.io
    rows = _made_up_rows()
    arrays = trajectory_arrays(rows, np.arange(len(rows)), 0.03332)
    no_action = {k: v for k, v in arrays.items() if k != "action"}
    scipy.io.savemat(str(tmp_path / "a.mat"), no_action)
    with pytest.raises(ValueError, match="'action'"):
        sysid.load_log(str(tmp_path / "a.mat"))
    for key in sysid.REQUIRED_KEYS:
        scipy.io.savemat(str(tmp_path / "k.mat"), {k: v for k, v in arrays.items() if k != key})
        with pytest.raises(ValueError, match="'%s'" % key):
            sysid.load_log(str(tmp_path / "k.mat"))
    # a log of the real robot without tip keys: allowed while their weights are 0
    no_tip = {k: v for k, v in arrays.items() if k not in ("tip_pos", "tip_vel")}
    scipy.io.savemat(str(tmp_path / "n.mat"), no_tip)
    back = sysid.load_log(str(tmp_path / "n.mat"))
    want = rows.copy()
    want[:, abi.VRF_TIP_Y:abi.VRF_TIP_VZ + 1] = 0
    assert np.array_equal(back, want)
    with pytest.raises(ValueError, match="'tip_pos'"):
        sysid.load_log(str(tmp_path / "n.mat"), [1.0] * abi.SYSID_FIELDS)
    with pytest.raises(ValueError, match="'tip_vel'"):
        sysid.load_log(str(tmp_path / "n.mat"), [0.0] * 14 + [1.0, 0.0])


def test_windows_on_a_hand_made_log():
    """30 rows: an episode that ends at row 13 (reset = 1 there; row 14 is the next episode's initial state, progress 0),
    and a progress jump between rows 22 and 23 (rows dropped from the log)."""
    T = 30
    log = np.zeros((T, abi.RECORD_FIELDS), dtype=np.float32)
    progress = list(range(1, 14)) + [14] + list(range(0, 9)) + list(range(20, 27))
    assert len(progress) == T
    log[:, abi.VRF_PROGRESS] = progress
    log[13, abi.VRF_RESET] = 1
    # horizon 4, every row: r = 0; r = 1..7 are below VINE_MAX_DELAY; 8, 9 fit before the reset row (rows r..r+3 without
    # reset: r + 3 <= 12); 10..13 cross it; 14..18 lie in the second episode (r + 4 <= 22); 19..22 cross the jump; 23..25
    assert sysid.windows(log, 4, 1) == [0, 8, 9, 14, 15, 16, 17, 18, 23, 24, 25]
    assert sysid.windows(log, 4, 3) == [0, 9, 15, 18, 24]
    assert sysid.windows(log, 4, 8) == [0, 8, 16, 24]
    assert sysid.windows(log, 8, 1) == [0, 14]                 # rows 0..8; rows 14..22
    assert sysid.windows(log, 9, 1) == [0]
    assert sysid.windows(log, 13, 1) == [0]                    # rows 0..13: the row with reset = 1 may END a window
    assert sysid.windows(log, 14, 1) == []                     # ... but not lie inside one: row 14 is another episode
    assert sysid.windows(log, 29, 1) == [] and sysid.windows(log, 40, 1) == []
    with pytest.raises(ValueError):
        sysid.windows(log, 0, 1)


# ---------------------------------------------------------------------------------------------------------- the search
def test_cem_against_a_fake_evaluator(hip_lib):
    """error = (DAMPING - 0.035)^2 + [delay != 2] on 512 candidates."""
    vcfg = abi.VineConfig()
    assert hip_lib.vine_config_default(C.byref(vcfg)) == abi.OK
    base = env_params.config_row(hip_lib, vcfg)
    spec = {"DAMPING": [0.005, 0.1], "ACTION_DELAY": {"values": [0, 1, 2, 3]}, "FPAM_K": [0.7, 1.3]}
    N, seed = 512, 11
    seen, checked = [], []

    def evaluate(table):
        assert table.dtype == np.float32 and table.shape == (abi.VP_COUNT, N)
        assert checked and checked[-1] is table                     # this very table passed the check before it got here
        seen.append(table.copy())
        return (table[abi.VP_DAMPING].astype(np.float64) - 0.035) ** 2 + (table[abi.VP_ACTION_DELAY] != 2)

    def check(table):
        t = env_params.check_table(hip_lib, vcfg, table)
        checked.append(table)
        return t

    best, best_err, history = sysid.cem(evaluate, spec, base, N, 6, seed, check=check)
    assert len(seen) == len(history) == 6
    # iteration 0 is build_table's draw
    assert np.array_equal(seen[0], env_params.build_table(spec, vcfg, seed, N, lib=hip_lib))
    errs = [h["best_error"] for h in history]
    assert all(b <= a for a, b in zip(errs, errs[1:])) and errs[-1] == best_err
    assert [h["iteration_best"] for h in history] == errs           # column 0 keeps the best alive in every population
    for it in range(1, 6):                                          # column 0 = the best of everything before
        prev = np.concatenate(seen[:it], axis=1)
        e = (prev[abi.VP_DAMPING].astype(np.float64) - 0.035) ** 2 + (prev[abi.VP_ACTION_DELAY] != 2)
        assert np.array_equal(seen[it][:, 0], prev[:, int(np.argmin(e))]), it
    assert best[abi.VP_ACTION_DELAY] == 2.0
    e0 = (seen[0][abi.VP_DAMPING].astype(np.float64) - 0.035) ** 2 + (seen[0][abi.VP_ACTION_DELAY] != 2)
    first_best = seen[0][:, int(np.argmin(e0))]
    assert abs(float(best[abi.VP_DAMPING]) - 0.035) <= abs(float(first_best[abi.VP_DAMPING]) - 0.035)
    assert np.array_equal(best, seen[-1][:, int(np.argmin(history[-1]["errors"]))])
    assert history[-1]["table"].shape == (abi.VP_COUNT, N) and history[-1]["errors"].shape == (N,)
    # every table that was evaluated had passed the check; ranges never leave the initial ones and they narrow
    assert len(checked) >= 6
    for h in history:
        for name, (lo, hi) in h["ranges"].items():
            lo0, hi0 = spec[name]
            assert lo0 <= lo <= hi <= hi0, (name, lo, hi)
        assert set(h["counts"]) == {"ACTION_DELAY"} and set(h["ranges"]) == {"DAMPING", "FPAM_K"}
    assert history[0]["ranges"]["DAMPING"] == [0.005, 0.1]
    lo, hi = history[-1]["ranges"]["DAMPING"]
    assert hi - lo < 0.1 - 0.005                                    # (the elites' spread, not the initial range)
    assert history[-1]["counts"]["ACTION_DELAY"] == {2.0: 52}       # the elites: ceil(0.1 * 512), all of delay 2
    for t in seen:
        assert np.float32(0.005) <= t[abi.VP_DAMPING].min() and t[abi.VP_DAMPING].max() <= np.float32(0.1)
        assert set(np.unique(t[abi.VP_ACTION_DELAY])) <= {0.0, 1.0, 2.0, 3.0}
        k = t[abi.VP_FPAM_K0:abi.VP_FPAM_K0 + 5] / base[abi.VP_FPAM_K0:abi.VP_FPAM_K0 + 5, None]
        assert 0.7 - 1e-6 <= k.min() and k.max() <= 1.3 + 1e-6
    # a bad table is stopped by the check, not evaluated
    with pytest.raises(ValueError, match="SMOOTHING_ALPHA_INFLATE"):
        sysid.cem(evaluate, {"SMOOTHING_ALPHA_INFLATE": [0.5, 1.5]}, base, N, 2, seed, check=check)


def test_candidate_config_forces_what_a_candidate_needs(caplog):
    import logging
    from vine_robot_isaacgymenvs_amd import load_task_config
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=64"])
    assert cfg["env"]["CREATE_PIPE"] and cfg["task"]["vine_randomize"] and cfg["env"]["USE_TARGET_REACHED_RESET"]
    cfg["env"]["maxEpisodeLength"] = 10
    with caplog.at_level(logging.INFO):
        out = sysid.candidate_config(cfg, {"DAMPING": [0.01, 0.05]}, 70, 12)
    assert cfg["env"]["CREATE_PIPE"] and cfg["env"]["numEnvs"] == 64            # the caller's config is not touched
    assert out["task"]["vine_randomize"] is False
    rp = out["task"]["randomization_parameters"]
    assert rp["OBSERVATION_NOISE_STD"] == 0.0 and rp["ACTION_NOISE_STD"] == 0.0
    env = out["env"]
    assert not env["CREATE_PIPE"] and not env["CREATE_SHELF"]
    assert not (env["USE_TARGET_REACHED_RESET"] or env["USE_TIP_LIMIT_HIT_RESET"] or env["USE_NONZERO_CONTACT_FORCE_RESET"])
    assert env["maxEpisodeLength"] > 12 and env["numEnvs"] == 70 and env["ENV_PARAMS"] == {"DAMPING": [0.01, 0.05]}
    for word in ("vine_randomize", "CREATE_PIPE", "USE_TARGET_REACHED_RESET", "maxEpisodeLength", "numEnvs"):
        assert word in caplog.text, word
