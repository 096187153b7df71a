"""MPC without a GPU: the C ABI of include/vine_mpc.h against its ctypes mirror, the refusal of bad configurations by name,
the model's forced configuration, the build plumbing of the eleventh unit, and the numpy statement of the update
(``mpc.mpc_replay``) on hand-made costs."""
import ctypes as C
import logging
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_sensor, mpc
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(REPO, "include", "vine_mpc.h")).read()


@pytest.fixture(scope="module")
def hip_lib():
    native.build()
    return native.load()


def _mcfg(lib, **over):
    c = abi.VineMpcConfig()
    assert lib.vine_mpc_config_default(c) == abi.OK
    c.num_plants = 3
    for k, v in over.items():
        if k == "sigma":
            for i, x in enumerate(v):
                c.sigma[i] = x
        else:
            setattr(c, k, v)
    return c


# --------------------------------------------------------------------------------------------------------------- ABI
def test_mpc_header_and_ctypes_mirror_agree(hip_lib):
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(vine_mpc_[a-z_0-9]+)\s*\(", code)))
    assert names == sorted(abi.MPC_PROTOTYPES) and len(names) == 5
    for name in names:
        assert hasattr(hip_lib, name), name
    assert hip_lib.vine_mpc_config_size() == C.sizeof(abi.VineMpcConfig) == 16 + 8 + 8 + 8
    body = re.search(r"typedef struct VineMpcConfig \{(.*?)\}", code, re.S).group(1)
    fields = re.findall(r"^\s+(?:int32_t|float|double|uint64_t)\s+([a-z_]+)(?:\[\d+\])?;", body, re.M)
    assert fields == [n.rstrip("_") for n, _ in abi.VineMpcConfig._fields_]
    for macro, value in (("ABI_VERSION", abi.MPC_ABI_VERSION), ("THREADS", abi.MPC_THREADS),
                         ("MAX_HORIZON", abi.MPC_MAX_HORIZON), ("RNG_NOISE", abi.MPC_RNG_NOISE)):
        assert int(re.search(r"#define VINE_MPC_%s (\d+)" % macro, text).group(1)) == value
    # the purpose word is nobody else's
    assert abi.MPC_RNG_NOISE not in (abi.SENSOR_RNG_NOISE, abi.SENSOR_RNG_HOLD) and abi.MPC_RNG_NOISE > 7
    for name in ("vine_mpc_fork", "vine_mpc_scheduled", "vine_mpc_update"):
        decl = re.search(r"int %s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(abi.MPC_PROTOTYPES[name][1]), name
    # out of vine.h: the CPU oracle exports every symbol of that header
    assert "vine_mpc" not in open(os.path.join(REPO, "include", "vine.h")).read()
    assert not set(abi.MPC_PROTOTYPES) & set(abi.PROTOTYPES)


def test_mpc_build_plumbing():
    assert native.ALL_UNITS == native.BUILD_UNITS + (native.SRC_MPC,) and len(native.ALL_UNITS) == 11
    assert len(native.BUILD_UNITS) == 10 and native.SRC_MPC not in native.BUILD_UNITS
    assert os.path.basename(native.SRC_MPC) == "vine_mpc.hip" and os.path.exists(native.SRC_MPC)
    deps = [os.path.basename(d) for d in native.DEPS]
    for name in ("vine_mpc.hip", "vine_mpc.h", "vine_task_shared.h", "vine_observer.h", "vine_policy_head.h"):
        assert name in deps, name
    assert any(d.endswith("vine_mpc.h") for d in native._SOURCE_HEADERS[native.SRC_MPC])
    # u must hold numpy's bits: the pragma in front of everything the unit includes, and the flag that makes it count
    assert native._SOURCE_FLAGS[native.SRC_MPC] == ["-ffp-contract=fast-honor-pragmas"]
    flags = native._flags(native.SRC_MPC)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast")      # (a later one wins)
    src = open(native.SRC_MPC).read()
    assert src.index("#pragma clang fp contract(off)") < src.index("#include")
    assert '#include "vine_observer.h"' in src and '#include "vine_task_shared.h"' in src
    assert "atomic" not in re.sub(r"//.*", "", src)


def test_mpc_defaults(hip_lib):
    c = abi.VineMpcConfig()
    assert hip_lib.vine_mpc_config_default(c) == abi.OK
    assert (c.abi_version, c.num_plants, c.samples, c.horizon, c.lambda_, list(c.sigma), c.seed) == (1, 0, 256, 20, 0.05, [0.5, 0.5], 0)
    assert (c.samples, c.horizon, c.lambda_, c.sigma[0]) == tuple(mpc.DEFAULTS[k] for k in ("samples", "horizon", "lambda", "sigma"))
    assert hip_lib.vine_mpc_config_default(None) == abi.ERR_INVALID_ARG


def _entry_points(lib, cfg):
    return ((lib.vine_mpc_fork, (None, None, cfg) + (None,) * 12), (lib.vine_mpc_scheduled, (None, cfg) + (None,) * 9),
            (lib.vine_mpc_update, (None, cfg) + (None,) * 8))


@pytest.mark.parametrize("over, word", [
    (dict(abi_version=7), b"abi_version"), (dict(num_plants=0), b"num_plants"), (dict(samples=1), b"samples"),
    (dict(num_plants=1 << 20, samples=1 << 20), b"num_plants * samples"), (dict(horizon=0), b"horizon"),
    (dict(horizon=65), b"horizon"), (dict(lambda_=0.0), b"lambda"), (dict(lambda_=float("inf")), b"lambda"),
    (dict(lambda_=float("nan")), b"lambda"), (dict(sigma=[-1.0, 0.5]), b"sigma"), (dict(sigma=[0.5, float("nan")]), b"sigma"),
    (dict(sigma=[float("inf"), 0.0]), b"sigma")])
def test_mpc_refuses_bad_configs(hip_lib, over, word):
    """Validation comes before the handles or any pointer is looked at, so no device is needed to see it."""
    bad = _mcfg(hip_lib, **over)
    for fn, args in _entry_points(hip_lib, bad):
        hip_lib.vine_set_step_count(None, -1)             # leaves another message behind
        assert fn(*args) == abi.ERR_INVALID_ARG
        assert word in hip_lib.vine_last_error(), hip_lib.vine_last_error()


def test_mpc_refuses_null_pointers(hip_lib):
    good = _mcfg(hip_lib)
    for (fn, args), name in zip(_entry_points(hip_lib, good), (b"vine_mpc_fork", b"vine_mpc_scheduled", b"vine_mpc_update")):
        assert fn(*args) == abi.ERR_INVALID_ARG
        assert b"null argument to " + name in hip_lib.vine_last_error()
    for fn, args in _entry_points(hip_lib, None):
        assert fn(*args) == abi.ERR_INVALID_ARG
        assert b"config is NULL" in hip_lib.vine_last_error()


@pytest.mark.parametrize("kwargs, word", [
    (dict(num_plants=0), "plants"), (dict(num_plants=2.5), "plants"), (dict(samples=1), "samples"), (dict(samples=True), "samples"),
    (dict(horizon=0), "horizon"), (dict(horizon=65), "horizon"), (dict(lam=0.0), "lambda"), (dict(lam=-1.0), "lambda"),
    (dict(lam=float("nan")), "lambda"), (dict(lam="x"), "lambda"), (dict(sigma=-0.1), "sigma"), (dict(sigma=[0.1, 0.2, 0.3]), "sigma"),
    (dict(sigma=[0.1, float("inf")]), "sigma"), (dict(sigma=1e60), "sigma"), (dict(seed=-1), "seed"), (dict(seed=1.5), "seed"),
    (dict(num_plants=1 << 20, samples=1 << 20), "plants * samples")])
def test_mpc_config_errors_name_the_key(kwargs, word):
    args = dict(num_plants=4, samples=8, horizon=3)
    args.update(kwargs)
    with pytest.raises(ConfigError, match=re.escape(word)):
        mpc.mpc_config(**args)


def test_mpc_config_fills_the_mirror():
    c = mpc.mpc_config(5, 14, 12, lam=0.2, sigma=[0.25, 0.5], seed=(1 << 63) + 5)
    assert (c.abi_version, c.num_plants, c.samples, c.horizon, c.lambda_, list(c.sigma), c.seed) == (
        abi.MPC_ABI_VERSION, 5, 14, 12, 0.2, [0.25, 0.5], (1 << 63) + 5)
    assert list(mpc.mpc_config(1, 2, 1, sigma=0.125).sigma) == [0.125, 0.125]


# ------------------------------------------------------------------------------------------------------ model_config
def test_model_config_forces_and_keeps(caplog):
    from vine_robot_isaacgymenvs_amd import load_task_config
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=4"])
    env = cfg["env"]
    assert env["CREATE_PIPE"] and cfg["task"]["vine_randomize"] and env["USE_TARGET_REACHED_RESET"]
    env.update({"EPISODE_LOG": True, "RECORD_TRAJECTORIES": True, "CAPTURE_VIDEO": True, "MAT_FILE": "x.mat",
                "ENV_PARAMS": {"DAMPING": [0.01, 0.05]}, "ENV_PARAMS_PER_EPISODE": True,
                "ENV_PARAMS_ADR": {"DAMPING": {"START": [0.02, 0.03], "STEP": 0.005}}, "ENV_SENSOR": {"DELAY": 2},
                "ENV_PUSH": {"IMPULSE": 0.1}, "maxEpisodeLength": 123})
    cfg["task"].setdefault("randomization_parameters", {}).update({"OBSERVATION_NOISE_STD": 0.1, "ACTION_NOISE_STD": 0.2})
    before = repr(cfg)
    with caplog.at_level(logging.INFO):
        out = mpc.model_config(cfg, 4, 16, {"POSITION_REWARD_WEIGHT": 2.0, "RAIL_LIMIT_REWARD_WEIGHT": 1.5})
    assert repr(cfg) == before                                               # the caller's config is not touched
    assert out["task"]["vine_randomize"] is False
    rp = out["task"]["randomization_parameters"]
    assert rp["OBSERVATION_NOISE_STD"] == 0.0 and rp["ACTION_NOISE_STD"] == 0.0
    o = out["env"]
    assert not (o["EPISODE_LOG"] or o["RECORD_TRAJECTORIES"] or o["CAPTURE_VIDEO"] or o["ENV_PARAMS_PER_EPISODE"])
    assert o["MAT_FILE"] == "" and o["ENV_PARAMS_ADR"] == {} and o["ENV_SENSOR"] == {} and o["ENV_PUSH"] == {}
    assert o["numEnvs"] == 64
    assert o["POSITION_REWARD_WEIGHT"] == 2.0 and o["RAIL_LIMIT_REWARD_WEIGHT"] == 1.5
    # kept: the obstacles, the resets, the episode length, every other weight
    for key in ("CREATE_PIPE", "CREATE_SHELF", "USE_TARGET_REACHED_RESET", "USE_TIP_LIMIT_HIT_RESET",
                "USE_NONZERO_CONTACT_FORCE_RESET", "maxEpisodeLength", "ACTION_DELAY", "POSITION_SUCCESS_REWARD_WEIGHT"):
        assert o[key] == env[key], key
    for word in ("vine_randomize", "OBSERVATION_NOISE_STD", "ACTION_NOISE_STD", "EPISODE_LOG", "RECORD_TRAJECTORIES",
                 "CAPTURE_VIDEO", "MAT_FILE", "ENV_PARAMS_PER_EPISODE", "ENV_PARAMS_ADR", "ENV_SENSOR", "ENV_PUSH", "numEnvs",
                 "POSITION_REWARD_WEIGHT", "RAIL_LIMIT_REWARD_WEIGHT"):
        assert word in caplog.text, word
    # the default cost: a slope on the position term, on top of the task's own weights
    plain = mpc.model_config(cfg, 4, 16)["env"]
    assert plain["POSITION_REWARD_WEIGHT"] == 1.0 and plain["POSITION_SUCCESS_REWARD_WEIGHT"] == env["POSITION_SUCCESS_REWARD_WEIGHT"]
    with pytest.raises(ConfigError, match="NO_SUCH_REWARD_WEIGHT"):
        mpc.model_config(cfg, 4, 16, {"NO_SUCH_REWARD_WEIGHT": 1.0})
    with pytest.raises(ConfigError, match="DAMPING"):
        mpc.model_config(cfg, 4, 16, {"DAMPING": 1.0})
    with pytest.raises(ConfigError, match="POSITION_REWARD_WEIGHT"):
        mpc.model_config(cfg, 4, 16, {"POSITION_REWARD_WEIGHT": float("nan")})


# -------------------------------------------------------------------------------------------------------- mpc_replay
M, K, H, CLIP = 3, 10, 4, 1.0


def _nominal(seed=0):
    return (np.random.default_rng(seed).uniform(-0.6, 0.6, (M, H, 2))).astype(np.float32)


def _replay(cost, nominal=None, **kw):
    args = dict(sigma=[0.5, 0.25], lam=0.05, seed=1234, tick=[0, 7, (1 << 32) + 3], clip=CLIP)
    args.update(kw)
    return mpc.mpc_replay(_nominal() if nominal is None else nominal, cost, **args)


def test_replay_equal_costs_give_the_plain_mean():
    r = _replay(np.full(M * K, 3.5))
    assert np.array_equal(r["weights"], np.ones((M, K)))
    assert np.array_equal(r["new"], r["u"].astype(np.float64).mean(axis=1).astype(np.float32))


def test_replay_one_cost_far_below_gives_that_sample():
    cost = np.full((M, K), 100.0)
    best = [4, 0, 9]
    cost[np.arange(M), best] = 1.0
    r = _replay(cost.reshape(-1))
    assert np.array_equal(r["new"], r["u"][np.arange(M), best])           # exp(-99 / 0.05) is 0 in float64
    assert np.array_equal(r["plant_actions"], r["u"][np.arange(M), best, 0])


def test_replay_infinite_costs_are_ignored_and_all_infinite_keeps_the_nominal():
    cost = np.full((M, K), 2.0)
    cost[0, 3:] = np.inf
    cost[1, :] = np.inf
    nominal = _nominal(1)
    r = _replay(cost.reshape(-1), nominal)
    assert np.array_equal(r["weights"][0], [1.0] * 3 + [0.0] * (K - 3)) and not r["weights"][1].any()
    assert np.array_equal(r["new"][0], r["u"][0, :3].astype(np.float64).mean(axis=0).astype(np.float32))
    assert np.array_equal(r["new"][1], nominal[1])
    assert np.array_equal(r["plant_actions"][1], nominal[1, 0]) and np.array_equal(r["nominal"][1, :-1], nominal[1, 1:])
    assert np.isfinite(r["new"]).all()


def test_replay_reset_branch_shift_history_and_tick():
    history = np.random.default_rng(2).uniform(-1, 1, (M, abi.MAX_DELAY, 2)).astype(np.float32)
    r = _replay(np.arange(M * K, dtype=np.float64) * 0.01, plant_reset=[0, 1, 0], history=history)
    assert np.array_equal(r["plant_actions"][1], [0.0, 0.0]) and not r["nominal"][1].any()
    for p in (0, 2):
        assert np.array_equal(r["plant_actions"][p], r["new"][p, 0])
        assert np.array_equal(r["nominal"][p, :-1], r["new"][p, 1:])
        assert np.array_equal(r["nominal"][p, -1], r["new"][p, -1]) and np.array_equal(r["nominal"][p, -1], r["nominal"][p, -2])
    assert np.array_equal(r["history"][:, 0], r["plant_actions"]) and np.array_equal(r["history"][:, 1:], history[:, :-1])
    assert np.array_equal(r["tick"], [1, 8, (1 << 32) + 4])


def test_replay_sample_zero_carries_the_nominal_and_u_stays_inside_the_clip():
    nominal = _nominal(3)
    u = mpc.sample_actions(nominal, [0.5, 0.5], 99, K, 5, CLIP)
    assert np.array_equal(u[:, 0], nominal)
    wide = mpc.sample_actions(nominal, [3.0, 3.0], 99, 64, 5, 0.75)
    assert np.abs(wide).max() == np.float32(0.75) and (np.abs(wide) < 0.75).any()
    assert np.array_equal(wide[:, 0], nominal)
    # a pure function of (seed, p, j, tick, k, a, nominal): another tick or seed, other draws; the same, the same
    assert np.array_equal(u, mpc.sample_actions(nominal, [0.5, 0.5], 99, K, 5, CLIP))
    assert not np.array_equal(u[:, 1:], mpc.sample_actions(nominal, [0.5, 0.5], 99, K, 6, CLIP)[:, 1:])
    assert not np.array_equal(u[:, 1:], mpc.sample_actions(nominal, [0.5, 0.5], 98, K, 5, CLIP)[:, 1:])
    # ... and the sensor's statement of the deviate under the controller's purpose word: one float32 multiply, one add
    z = mpc.noise_deviate(99, M, K, 5, H)
    c = (np.float64(np.float32(0.5)) * env_sensor.NOISE_SCALE).astype(np.float32)
    assert np.array_equal(u, np.clip(nominal[:, None] + z * c, -np.float32(CLIP), np.float32(CLIP)))


def test_deviate_has_mean_zero_and_variance_one():
    z = mpc.noise_deviate(7, 16, 65, 3, 32)[:, 1:].astype(np.float64) * env_sensor.NOISE_SCALE     # 16 * 64 * 32 * 2 draws
    n = z.size
    assert n == 65536
    # the sum of eight uniforms has excess kurtosis -1.2 / 8: var(z^2) = 2 - 0.15
    assert abs(z.mean()) < 5.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 5.0 * np.sqrt(1.85 / n)


def test_cost_sums_stop_behind_a_reset_and_turn_infinite_on_a_nan():
    rew = np.array([[-1.0, -1.0, -1.0, -1.0], [-2.0, -2.0, np.nan, -2.0], [-4.0, -4.0, -4.0, -4.0]], dtype=np.float32)
    reset = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    cost, alive = mpc.cost_sums(rew, reset)
    assert np.array_equal(cost, [7.0, 3.0, np.inf, 7.0]) and np.array_equal(alive, [1, 0, 0, 0])
