"""MPC_ENSEMBLE without a GPU: include/vine_mpc_ensemble.h against its ctypes mirror and the build plumbing of the twenty-first
unit, every ``ConfigError`` of ``ensemble_config`` and ``Play``'s refusal of every other variant and of ``model_params=``, every
refusal of the entry points by name through the library, the members' draw, and the numpy statements of utils/mpc_ensemble.py:
``group_costs`` on hand-made costs and ``ensemble_replay`` against ``mpc.mpc_replay``."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params, mpc, mpc_ensemble
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError, parse_scalar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"DAMPING": [0.005, 0.1], "LINK_MASS": [0.7, 1.4], "ACTION_DELAY": {"values": [0, 2]}}


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.load()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_equals_the_mirror_the_struct_size_and_the_build_wiring(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vine_mpc_ensemble.h")).read(), flags=re.S)
    for macro, value in (("VINE_MPC_ENSEMBLE_ABI_VERSION", abi.MPC_ENSEMBLE_ABI_VERSION),
                         ("VINE_MPC_ENSEMBLE_MAX_MEMBERS", abi.MPC_ENSEMBLE_MAX_MEMBERS), ("VINE_MPC_RISK_MEAN", abi.MPC_RISK_MEAN),
                         ("VINE_MPC_RISK_MAX", abi.MPC_RISK_MAX), ("VINE_MPC_RISK_ENTROPIC", abi.MPC_RISK_ENTROPIC)):
        assert int(re.search(r"#define %s (\d+)\s" % macro, text).group(1)) == value, macro
    assert abi.MPC_ENSEMBLE_MAX_MEMBERS == 16 and abi.MPC_RISK_NAMES == ("mean", "max", "entropic")
    body = re.search(r"typedef struct VineMpcEnsembleConfig \{(.*?)\} VineMpcEnsembleConfig;", text, flags=re.S).group(1)
    decls = [decl.strip() for decl in body.split(";") if decl.strip()]
    assert [d.split()[-1] for d in decls] == [f[0] for f in abi.VineMpcEnsembleConfig._fields_] == ["abi_version", "members", "risk", "theta"]
    kinds = {"int32_t": C.c_int32, "double": C.c_double}
    assert [kinds[d.split()[0]] for d in decls] == [f[1] for f in abi.VineMpcEnsembleConfig._fields_]
    assert lib.vine_mpc_ensemble_config_size() == C.sizeof(abi.VineMpcEnsembleConfig) == 24
    functions = sorted(set(re.findall(r"\b(vine_mpc_ensemble[a-z_0-9]*)\s*\(", text)))
    assert functions == sorted(abi.MPC_ENSEMBLE_PROTOTYPES) and len(functions) == 4
    for name, count in (("vine_mpc_ensemble_scheduled", 8), ("vine_mpc_ensemble_update", 12)):
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert hasattr(lib, name) and len(decl.split(",")) == len(abi.MPC_ENSEMBLE_PROTOTYPES[name][1]) == count, name
    assert "declare_mpc_ensemble" in inspect.getsource(abi.declare_all)
    c = abi.VineMpcEnsembleConfig()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    assert lib.vine_mpc_ensemble_config_default(C.byref(c)) == abi.OK
    assert (c.abi_version, c.members, c.risk, c.theta) == (1, 4, abi.MPC_RISK_MEAN, 1.0)
    assert lib.vine_mpc_ensemble_config_default(None) == abi.ERR_INVALID_ARG
    # nothing of it went into the base header or the base unit
    assert "ensemble" not in open(os.path.join(REPO, "include", "vine_mpc.h")).read()
    assert "ensemble" not in open(native.SRC_MPC).read().lower()


def test_the_pinned_unit_tuples_stand_and_the_new_unit_is_built():
    n = native
    assert n.NOISE_UNITS == (n.SRC_MPC_NOISE,) and n.INERTIA_UNITS == (n.SRC_MPC_ADAPT_INERTIA,)
    assert n.ENSEMBLE_UNITS == (n.SRC_MPC_ENSEMBLE,)
    for pinned in (n.SOURCES, n.UNITS, n.BUILD_UNITS, n.ALL_UNITS, n.LIB_UNITS, n.POLICY_UNITS, n.LATER_UNITS, n.NOISE_UNITS,
                   n.INERTIA_UNITS):
        assert n.SRC_MPC_ENSEMBLE not in pinned
    build = inspect.getsource(n.build)
    at = [build.index(line) for line in ("map(compile_unit, INERTIA_UNITS)", "map(compile_unit, ENSEMBLE_UNITS)", "proc.wait()")]
    assert at == sorted(at) and build.count("compile_unit(") == 3
    src = n.SRC_MPC_ENSEMBLE
    assert os.path.basename(src) == "vine_mpc_ensemble.hip" and os.path.exists(src)
    assert src in n.DEPS and any(d.endswith("vine_mpc_ensemble.h") for d in n.DEPS)          # it enters the library's fingerprint
    assert {"vine_mpc.h", "vine_mpc_ensemble.h", "vine_mpc_shared.h"} <= {os.path.basename(h) for h in n._SOURCE_HEADERS[src]}
    assert n._SOURCE_FLAGS[src] == ["-ffp-contract=fast-honor-pragmas"]
    flags = n._flags(src)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast") and "-ffp-contract=off" not in flags
    source = open(src).read()
    assert source.index("#pragma clang fp contract(off)") < source.index("#include")
    assert "atomic" not in source.replace("No atomics", "") and "hipMalloc" not in source and "Synchronize" not in source
    assert '#include "vine_mpc_shared.h"' in source and "mpc_deviate_int" in source


# ------------------------------------------------------------------------------------------------------ the configuration
def test_every_config_error_of_ensemble_config_by_name():
    got = mpc_ensemble.ensemble_config({"params": {"DAMPING": [0.005, 0.1]}})
    assert got == {"params": {"DAMPING": [0.005, 0.1]}, "MEMBERS": 4, "RISK": "mean", "THETA": None, "SEED": None}
    text = "{params: {DAMPING: [0.005, 0.1], LINK_MASS: [0.7, 1.4], ACTION_DELAY: {values: [0, 2]}}, MEMBERS: 8, RISK: entropic, THETA: 0.5, SEED: 3}"
    got = mpc_ensemble.ensemble_config(parse_scalar(text))
    assert (got["MEMBERS"], got["RISK"], got["THETA"], got["SEED"]) == (8, "entropic", 0.5, 3)
    assert got["params"] == env_params.spec_forms(PARAMS) and mpc_ensemble.ensemble_config(got) == got
    good = {"DAMPING": 0.02}
    with pytest.raises(ConfigError, match="ensemble=.*must be a mapping, not 4"):
        mpc_ensemble.ensemble_config(4)
    with pytest.raises(ConfigError, match=r"ensemble: unknown key\(s\) Members, theta"):
        mpc_ensemble.ensemble_config({"params": good, "Members": 2, "theta": 1.0})
    with pytest.raises(ConfigError, match="ensemble.params is missing"):
        mpc_ensemble.ensemble_config({"MEMBERS": 2})
    for bad in ({}, [0.1, 0.2], 0.5):
        with pytest.raises(ConfigError, match="ensemble.params must be a mapping of parameter names that is not empty"):
            mpc_ensemble.ensemble_config({"params": bad})
    with pytest.raises(ConfigError, match="ensemble.params: ENV_PARAMS: unknown parameter 'DAMPNG'"):
        mpc_ensemble.ensemble_config({"params": {"DAMPNG": 0.1}})
    with pytest.raises(ConfigError, match="ensemble.params: ENV_PARAMS.ACTION_DELAY: an integer parameter takes an integer range"):
        mpc_ensemble.ensemble_config({"params": {"ACTION_DELAY": [0.5, 2]}})
    for bad in (0, 17, -1, 2.0, True, "4", None):
        with pytest.raises(ConfigError, match=r"ensemble.MEMBERS must be an integer in 1 \.\. 16"):
            mpc_ensemble.ensemble_config({"params": good, "MEMBERS": bad})
    for bad in ("cvar", "MEAN", 1, None):
        with pytest.raises(ConfigError, match="ensemble.RISK must be one of mean, max, entropic"):
            mpc_ensemble.ensemble_config({"params": good, "RISK": bad})
    with pytest.raises(ConfigError, match="ensemble.THETA is missing"):
        mpc_ensemble.ensemble_config({"params": good, "RISK": "entropic"})
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ConfigError, match="ensemble.THETA must be a finite number > 0"):
            mpc_ensemble.ensemble_config({"params": good, "RISK": "entropic", "THETA": bad})
    for risk in ("mean", "max"):
        with pytest.raises(ConfigError, match="ensemble.THETA is refused with RISK %s" % risk):
            mpc_ensemble.ensemble_config({"params": good, "RISK": risk, "THETA": 0.5})
    for bad in (-1, 1.5, "7", True):
        with pytest.raises(ConfigError, match="ensemble.SEED must be an integer >= 0"):
            mpc_ensemble.ensemble_config({"params": good, "SEED": bad})
    # the struct beside a controller's configuration
    c = mpc_ensemble.ensemble_struct({"params": good, "MEMBERS": 8, "RISK": "entropic", "THETA": 0.25}, mpc.mpc_config(3, 16, 5))
    assert (c.abi_version, c.members, c.risk, c.theta) == (abi.MPC_ENSEMBLE_ABI_VERSION, 8, abi.MPC_RISK_ENTROPIC, 0.25)
    c = mpc_ensemble.ensemble_struct({"params": good, "MEMBERS": 1, "RISK": "max"}, mpc.mpc_config(3, 15, 5))
    assert (c.members, c.risk) == (1, abi.MPC_RISK_MAX)
    with pytest.raises(ConfigError, match="mpc: samples = 18 is not a multiple of ensemble.MEMBERS = 4"):
        mpc_ensemble.ensemble_struct({"params": good}, mpc.mpc_config(3, 18, 5))


OTHER_ARGUMENT = {"noise": {"BETA": 0.8}, "track": {"PATH": "exact"}, "observe": {"DELAY": 1}, "filter": {},
                  "adapt": {"params": {"DAMPING": [0.005, 0.1]}}, "policy": "x.pth", "model_params": {"DAMPING": [0.01, 0.05]}}
SPEC = {"params": {"DAMPING": [0.005, 0.1]}, "MEMBERS": 4}


@pytest.mark.parametrize("other", mpc.VARIANTS + ("model_params",))
def test_play_refuses_ensemble_together_with_each_variant_and_model_params_by_name(other, monkeypatch):
    message = "mpc: ensemble= together with %s= is refused" % other
    args = dict.fromkeys(mpc.VARIANTS + ("model_params",))
    args.update({"ensemble": SPEC, other: OTHER_ARGUMENT[other]})
    run = types.SimpleNamespace(args=args, M=2, samples=16, planner=(5, 0.05, 0.5, 0))
    with pytest.raises(ConfigError, match=message):
        mpc_ensemble.Play(SPEC).check(run)
    # ... and through play, before any task is made (filter needs observe beside it: the table of rules comes first)

    def no_task(*a, **k):
        raise AssertionError("a task was made before the combination was refused")

    monkeypatch.setattr(mpc, "make_task", no_task)
    env = {"numEnvs": 2, "ENV_TARGET": {"VEL_ALONG": 0.1, "SPAN_ALONG": 0.05}}
    given = {other: OTHER_ARGUMENT[other]}
    if other == "filter":
        given["observe"], message = OTHER_ARGUMENT["observe"], "mpc: ensemble= together with observe= is refused"
    with pytest.raises(ConfigError, match=message):
        mpc.play({"env": env, "seed": 0}, samples=256, ensemble=SPEC, **given)


def test_play_takes_ensemble_and_the_rule_table_is_unchanged(monkeypatch):
    assert mpc.VARIANTS == ("noise", "track", "observe", "filter", "policy", "adapt") and mpc.FIRST == ("ensemble",)
    assert inspect.signature(mpc.play).parameters["ensemble"].default is None
    assert len(mpc.RULES) == 12 and not any("ensemble" in k for keys, _ in mpc.RULES for k in keys)
    assert not any("ensemble" in message for _, message in mpc.RULES)
    import mpc as tool
    assert tool.OWN["ensemble"] is None and "ensemble=own[\"ensemble\"]" in inspect.getsource(tool.main)
    with pytest.raises(ConfigError, match="mpc: ensemble=.*must be a mapping, not 4"):
        tool.main(["ensemble=4"])

    def no_task(*a, **k):
        raise AssertionError("a task was made before the argument was refused")

    monkeypatch.setattr(mpc, "make_task", no_task)
    plain = {"env": {"numEnvs": 2}, "seed": 0}
    with pytest.raises(ConfigError, match="ensemble.params is missing"):
        mpc.play(plain, samples=16, ensemble={"MEMBERS": 4})
    with pytest.raises(ConfigError, match="mpc: samples = 18 is not a multiple of ensemble.MEMBERS = 4"):
        mpc.play(plain, samples=18, ensemble=SPEC)
    run = types.SimpleNamespace(args={}, M=2, samples=16, planner=(5, 0.05, 0.5, 7))
    for spec, seed in ((SPEC, 8), (dict(SPEC, SEED=7), 7)):                   # the default: the planner's seed + 1
        play = mpc_ensemble.Play(spec)
        play.check(run)
        assert play.seed == seed


# ------------------------------------------------------------------------------------------- refusals of the entry points
REFUSALS = (
    ("VineMpcEnsembleConfig.abi_version mismatch", dict(abi_version=2)),
    ("mpc ensemble members must be in 1 .. VINE_MPC_ENSEMBLE_MAX_MEMBERS (16)", dict(members=0)),
    ("mpc ensemble members must be in 1 .. VINE_MPC_ENSEMBLE_MAX_MEMBERS (16)", dict(members=17)),
    ("mpc ensemble members must divide samples of the VineMpcConfig", dict(members=5)),
    ("mpc ensemble risk must be VINE_MPC_RISK_MEAN, VINE_MPC_RISK_MAX or VINE_MPC_RISK_ENTROPIC", dict(risk=3)),
    ("mpc ensemble risk must be VINE_MPC_RISK_MEAN, VINE_MPC_RISK_MAX or VINE_MPC_RISK_ENTROPIC", dict(risk=-1)),
    ("mpc ensemble theta must be finite and positive with VINE_MPC_RISK_ENTROPIC", dict(risk=2, theta=0.0)),
    ("mpc ensemble theta must be finite and positive with VINE_MPC_RISK_ENTROPIC", dict(risk=2, theta=float("nan"))),
    ("mpc ensemble theta must be finite and positive with VINE_MPC_RISK_ENTROPIC", dict(risk=2, theta=float("inf"))),
    ("null argument to vine_mpc_ensemble_", dict(risk=1, theta=-3.0)),          # without ENTROPIC theta is not looked at
    ("null argument to vine_mpc_ensemble_", dict(members=16)),
    ("null argument to vine_mpc_ensemble_", dict(members=1)),
)


@pytest.mark.parametrize("message,change", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_every_refusal_of_the_entry_points_by_name(lib, message, change):
    mcfg = mpc.mpc_config(3, 16, 5)
    e = abi.VineMpcEnsembleConfig()
    assert lib.vine_mpc_ensemble_config_default(C.byref(e)) == abi.OK
    for k, v in change.items():
        setattr(e, k, v)
    calls = (lambda: lib.vine_mpc_ensemble_scheduled(None, mcfg, e, None, None, None, None, None),
             lambda: lib.vine_mpc_ensemble_update(None, mcfg, e, None, None, None, None, None, None, None, None, None))
    for call in calls:
        assert call() == abi.ERR_INVALID_ARG
        assert message in lib.vine_last_error().decode()
    # the base configuration is refused first, in vine_mpc.hip's words
    mcfg.horizon = abi.MPC_MAX_HORIZON + 1
    for call in calls:
        assert call() == abi.ERR_INVALID_ARG
        assert lib.vine_last_error() == b"mpc needs 1 <= horizon <= VINE_MPC_MAX_HORIZON (64)"
    assert lib.vine_mpc_ensemble_scheduled(None, None, e, None, None, None, None, None) == abi.ERR_INVALID_ARG
    assert lib.vine_last_error() == b"mpc config is NULL"
    assert lib.vine_mpc_ensemble_scheduled(None, mpc.mpc_config(3, 16, 5), None, None, None, None, None, None) == abi.ERR_INVALID_ARG
    assert lib.vine_last_error() == b"mpc ensemble config is NULL"


# --------------------------------------------------------------------------------------------------------- the members
def test_draw_members_is_pure_and_is_not_the_plants_own_draw(lib):
    vcfg = abi.VineConfig()
    assert lib.vine_config_default(C.byref(vcfg)) == 0
    M, E, seed = 6, 4, 11
    a = mpc_ensemble.draw_members(PARAMS, vcfg, lib, seed + 1, M, E)
    b = mpc_ensemble.draw_members(PARAMS, vcfg, lib, seed + 1, M, E)
    assert set(a) == set(PARAMS) and all(v.shape == (M, E) and v.dtype == np.float64 for v in a.values())
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)
    assert np.all((a["DAMPING"] >= 0.005) & (a["DAMPING"] <= 0.1)) and np.all((a["LINK_MASS"] >= 0.7) & (a["LINK_MASS"] <= 1.4))
    assert set(np.unique(a["ACTION_DELAY"])) <= {0.0, 2.0} and len(np.unique(a["DAMPING"])) == M * E
    # the global id of member m of plant p is p * E + m: env_params' own draw over M * E envs
    flat = {}
    env_params.draw_table(PARAMS, env_params.config_row(lib, vcfg), seed + 1, M * E, draws=flat)
    assert all(np.array_equal(a[k].reshape(-1), flat[k]) for k in a)
    # under the plants' own seed the first M members WOULD be the plants (which is why SEED defaults to seed + 1) ...
    plants = mpc.draw_model_params(PARAMS, vcfg, lib, seed, M)
    own = mpc_ensemble.draw_members(PARAMS, vcfg, lib, seed, M, E)
    assert np.array_equal(own["DAMPING"].reshape(-1)[:M], plants["DAMPING"])
    # ... and under the default they are not
    assert not np.any(a["DAMPING"].reshape(-1)[:M] == plants["DAMPING"])
    assert not np.any(a["DAMPING"][:, 0] == plants["DAMPING"])
    # each plant's E values tiled over its groups: sample j takes member j mod E
    G = 3
    tiled = mpc_ensemble.tile_members(a, G)
    assert tiled["DAMPING"].shape == (M * G * E,)
    t = tiled["DAMPING"].reshape(M, G, E)
    assert all(np.array_equal(t[:, g], a["DAMPING"]) for g in range(G))
    with pytest.raises(ValueError, match="DAMPING takes an array"):
        mpc_ensemble.tile_members({"DAMPING": np.zeros(M)}, G)


# ------------------------------------------------------------------------------------------------- the numpy statements
def test_group_costs_on_hand_made_costs():
    cost = np.array([[1.0, 3.0, 2.0, 2.0, 0.5, np.inf, 4.0, 0.0],
                     [0.1, 0.2, 0.3, 0.4, 5.0, 5.0, np.inf, np.inf]])
    mean = mpc_ensemble.group_costs(cost, 2, "mean")
    assert np.array_equal(mean, [[2.0, 2.0, np.inf, 2.0], [(0.1 + 0.2) / 2.0, (0.3 + 0.4) / 2.0, 5.0, np.inf]])
    worst = mpc_ensemble.group_costs(cost, 2, "max")
    assert np.array_equal(worst, [[3.0, 2.0, np.inf, 4.0], [0.2, 0.4, 5.0, np.inf]])
    # the mean's order is the written-out one, not np.sum's pairwise one
    rng = np.random.default_rng(0)
    c16 = rng.uniform(0.0, 1.0, (3, 5 * 16))
    want = c16.reshape(3, 5, 16)[..., 0].copy()
    for m in range(1, 16):
        want = want + c16.reshape(3, 5, 16)[..., m]
    assert np.array_equal(bits(mpc_ensemble.group_costs(c16, 16, "mean")), bits(want / 16.0))
    # entropic lies between the mean and the maximum, and rises with theta; identical members: all three the member's cost
    finite = np.isfinite(mean)
    last = mean
    for theta in (0.01, 0.5, 4.0, 50.0):
        ent = mpc_ensemble.group_costs(cost, 2, "entropic", theta)
        assert np.array_equal(np.isfinite(ent), finite) and np.all(np.isposinf(ent[~finite]))
        assert np.all(ent[finite] >= mean[finite] - 1e-15) and np.all(ent[finite] <= worst[finite])
        spread = worst[finite] > mean[finite]
        assert np.all(ent[finite][spread] > last[finite][spread]) and np.all(ent[finite][~spread] == mean[finite][~spread])
        last = ent
    assert np.allclose(mpc_ensemble.group_costs(cost, 2, "entropic", 1e-6)[finite], mean[finite], atol=1e-5)
    assert np.allclose(mpc_ensemble.group_costs(cost, 2, "entropic", 1e4)[finite], worst[finite], atol=1e-3)
    assert mpc_ensemble.group_costs(cost, 2, "entropic", 0.5)[0, 0] == 3.0 + np.log((np.exp(0.5 * (1.0 - 3.0)) + 1.0) / 2.0) / 0.5
    # one +inf (or NaN) member discards its group, whatever the risk
    for risk, theta in (("mean", None), ("max", None), ("entropic", 0.5)):
        g = mpc_ensemble.group_costs([0.0, np.inf, 1.0, 1.0, np.nan, 0.0], 2, risk, theta)
        assert g.shape == (1, 3) and np.isposinf(g[0, 0]) and g[0, 1] == 1.0 and np.isposinf(g[0, 2])
        # E = 1 is the identity in every bit
        c1 = rng.uniform(0.0, 30.0, (4, 9))
        c1[2, 3] = np.inf
        assert np.array_equal(bits(mpc_ensemble.group_costs(c1, 1, risk, theta)), bits(c1))
    with pytest.raises(ValueError, match="not a multiple of members"):
        mpc_ensemble.group_costs(np.zeros((2, 7)), 2, "mean")
    with pytest.raises(ValueError, match="entropic needs a finite theta"):
        mpc_ensemble.group_costs(np.zeros((2, 8)), 2, "entropic")
    with pytest.raises(ValueError, match="risk must be one of"):
        mpc_ensemble.group_costs(np.zeros((2, 8)), 2, "cvar")


def test_group_actions_are_a_controller_of_g_samples():
    M, K, E, H, clip = 3, 12, 4, 5, 1.0
    rng = np.random.default_rng(1)
    nominal = rng.uniform(-0.95, 0.95, (M, H, 2)).astype(np.float32)
    tick = np.array([(1 << 33) + 9, 0, 4], dtype=np.int64)
    u = mpc_ensemble.group_actions(nominal, [0.5, 0.25], 77, K, E, tick, clip)
    assert u.shape == (M, K // E, H, 2) and u.dtype == np.float32
    assert np.array_equal(bits(u), bits(mpc.sample_actions(nominal, [0.5, 0.25], 77, K // E, tick, clip)))
    assert np.array_equal(bits(u[:, 0]), bits(nominal))                        # group 0 is the (clamped) nominal
    full = mpc_ensemble.member_actions(u, E)
    assert full.shape == (M, K, H, 2) and all(np.array_equal(bits(full[:, g * E + m]), bits(u[:, g])) for g in range(3) for m in range(E))
    # not the leader's model env: a controller of K samples draws other words for sample g * E
    assert not np.array_equal(bits(mpc.sample_actions(nominal, [0.5, 0.25], 77, K, tick, clip)[:, E]), bits(u[:, 1]))
    with pytest.raises(ValueError, match="not a multiple of members"):
        mpc_ensemble.group_actions(nominal, 0.5, 77, 13, E, tick, clip)


def test_ensemble_replay_with_one_member_is_the_base_replay_and_groups_weigh_as_one():
    M, K, H, clip = 3, 10, 4, 1.0
    rng = np.random.default_rng(3)
    nominal = rng.uniform(-0.5, 0.5, (M, H, 2)).astype(np.float32)
    history = rng.uniform(-1, 1, (M, abi.MAX_DELAY, 2)).astype(np.float32)
    cost = rng.uniform(0, 0.5, (M, K))
    cost[0, 3] = np.inf
    cost[1] = np.inf
    reset = np.array([0, 0, 1])
    tick = np.array([3, (1 << 33) + 4, 5])
    base = mpc.mpc_replay(nominal, cost.reshape(-1), [0.5, 0.25], 0.05, 9, tick, clip, reset, history)
    for risk, theta in (("mean", None), ("max", None), ("entropic", 0.7)):
        r = mpc_ensemble.ensemble_replay(nominal, cost.reshape(-1), [0.5, 0.25], 0.05, 9, tick, clip, 1, risk, theta, reset, history)
        for key in ("u", "weights", "new", "nominal", "plant_actions", "history", "tick"):
            a, b = np.ascontiguousarray(base[key]), np.ascontiguousarray(r[key])
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (risk, key)
        assert np.array_equal(bits(r["group_cost"]), bits(cost)) and np.array_equal(r["member_weights"], r["weights"])
    # E = 2: one +inf member gives its group the weight 0, on both members; a plant without a finite group keeps its nominal
    r = mpc_ensemble.ensemble_replay(nominal, cost.reshape(-1), [0.5, 0.25], 0.05, 9, tick, clip, 2, "mean", None, reset, history)
    assert r["weights"].shape == (M, 5) and r["member_weights"].shape == (M, K) and r["u"].shape == (M, 5, H, 2)
    assert r["weights"][0, 1] == 0.0 and np.count_nonzero(r["weights"][0]) == 4 and r["weights"][0].max() == 1.0
    assert r["member_weights"][0, 2] == r["member_weights"][0, 3] == 0.0
    assert not r["weights"][1].any() and np.array_equal(r["nominal"][1, :-1], nominal[1, 1:])
    assert not r["nominal"][2].any() and not r["plant_actions"][2].any() and np.array_equal(r["tick"], tick + 1)
    # the device's own group costs in the place of group_costs'
    given = mpc_ensemble.ensemble_replay(nominal, cost.reshape(-1), [0.5, 0.25], 0.05, 9, tick, clip, 2, "max", None, reset, history,
                                         group_cost=r["group_cost"])
    assert np.array_equal(given["weights"], r["weights"]) and np.array_equal(given["nominal"], r["nominal"])
