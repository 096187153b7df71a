"""ENV_PUSH without a GPU: include/vine_env_push.h against its ctypes mirror, every refusal of its host entry point and of
the configuration, the draw, utils/env_push.py push_replay on hand-made states (the properties the header states, against
the oracle's forward dynamics, energy and tip kinematics), the statistics of the draws, and the episode log's join and file
round trip."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from oracle import vine_oracle as vo
from vine_robot_isaacgymenvs_amd import abi, load_config, native
from vine_robot_isaacgymenvs_amd.utils import env_params, env_push, episodes
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 42
ND = 6


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.load()


@pytest.fixture()
def vcfg(lib):
    c = abi.VineConfig()
    assert lib.vine_config_default(C.byref(c)) == 0
    c.seed = SEED
    return c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def config(**keys):
    return env_push.push_config({"ENV_PUSH": keys})


def hand_states(steps, n, seed=1):
    """State blocks [T, VF_COUNT, N]: joints within +-10 degrees, the cart within +-0.3, velocities within +-3; every other
    field a recognisable pattern."""
    rng = np.random.default_rng(seed)
    f, t, e = np.meshgrid(np.arange(abi.VF_COUNT), np.arange(steps), np.arange(n), indexing="ij")
    st = ((f + 1) / 8.0 + t / 1024.0 + e / 65536.0).astype(np.float32).transpose(1, 0, 2).copy()
    st[:, abi.VF_Q0] = rng.uniform(-0.3, 0.3, (steps, n))
    st[:, abi.VF_Q0 + 1:abi.VF_Q0 + ND] = rng.uniform(-np.radians(10), np.radians(10), (steps, ND - 1, n))
    st[:, abi.VF_QD0:abi.VF_QD0 + ND] = rng.uniform(-3, 3, (steps, ND, n))
    return st


def exact_geometry(lib, vcfg):
    """The geometry in double, as the oracle holds it: composites not rounded, sin / cos of phi0 in double."""
    phi0 = np.float64(np.float32(vcfg.phi0))
    return {"L": np.float64(np.float32(vcfg.link_length)), "s0": np.sin(phi0), "c0": np.cos(phi0), "composites": env_push.composites64(vcfg)}


def relative_effort(Q):
    """J^T P in the relative coordinates from the absolute ones: eff_0 = Q_0, eff_{j+1} = sum_{k >= j} Q_{k+1}."""
    out = np.array(Q, dtype=np.float64)
    out[1:] = np.cumsum(Q[1:][::-1])[::-1]
    return out


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_equals_the_mirror_the_struct_size_and_the_build_wiring(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vine_env_push.h")).read(), flags=re.S)
    for macro, value in (("VINE_ENV_PUSH_ABI_VERSION", abi.ENV_PUSH_ABI_VERSION), ("VINE_ENV_PUSH_THREADS", abi.ENV_PUSH_THREADS),
                         ("VINE_PUSH_MAX_POINTS", abi.PUSH_MAX_POINTS), ("VINE_PUSH_COMPOSITES", abi.PUSH_COMPOSITES),
                         ("VINE_PUSH_RNG", abi.PUSH_RNG)):
        assert int(re.search(r"#define %s (\d+)u?\s" % macro, text).group(1)) == value, macro
    assert abi.PUSH_RNG == 7 and abi.PUSH_COMPOSITES == abi.VI_COUNT - abi.VI_MTOT == 20 and abi.PUSH_MAX_POINTS == abi.NUM_LINKS + 1
    # purpose word 7 is nobody else's: the step kernels stop at 4, the sensor uses 5 and 6
    hip = open(native.SRC).read()
    used = [int(v) for v in re.findall(r"RNG_\w+ = (\d+)", re.search(r"enum \{ (RNG_RESET.*?)\};", hip).group(1))]
    assert max(used) == 4 and sorted({abi.SENSOR_RNG_NOISE, abi.SENSOR_RNG_HOLD, abi.PUSH_RNG}) == [5, 6, 7]
    csrc = os.path.dirname(native.SRC)
    for name in sorted(os.listdir(csrc)):
        if name != "vine_env_push.hip":
            source = open(os.path.join(csrc, name)).read()
            assert "VINE_PUSH_RNG" not in source and not re.search(r"RNG\w*\s*=?\s*7u?\b", source), name
    slots = re.search(r"typedef enum VineEnvPushSlot \{(.*?)\}", text, flags=re.S).group(1)
    assert [w.split("=")[0].strip() for w in slots.split(",")] == ["VPU_RATE", "VPU_IMPULSE", "VPU_NAMES"]
    assert ["VPU_" + n for n in abi.ENV_PUSH_NAMES] == ["VPU_RATE", "VPU_IMPULSE"] and abi.VPU_NAMES == 2
    body = re.search(r"typedef struct VineEnvPushSpec \{(.*?)\} VineEnvPushSpec;", text, flags=re.S).group(1)
    fields = [re.sub(r"\[.*?\]", "", decl.strip()).replace("*", " ").split()[-1] for decl in body.split(";") if decl.strip()]
    assert fields == [f[0] for f in abi.VineEnvPushSpec._fields_]
    assert lib.vine_env_push_spec_size() == C.sizeof(abi.VineEnvPushSpec) == 24 + 2 * 48 + 8 + 6 * 4 + 20 * 4 + 8 == 240
    functions = sorted(set(re.findall(r"\b(vine_env_push[a-z_0-9]*)\s*\(", text)))
    assert functions == sorted(abi.ENV_PUSH_PROTOTYPES)
    for name in functions:
        assert hasattr(lib, name), name
    # the tenth translation unit, behind the nine; its pragma, the flag that makes the compiler honour it, its headers
    assert native.BUILD_UNITS == native.UNITS + (native.SRC_PUSH,) and len(native.BUILD_UNITS) == 10 and len(native.UNITS) == 9
    assert native.SRC_PUSH in native.DEPS and any(d.endswith("vine_env_push.h") for d in native.DEPS)
    headers = native._SOURCE_HEADERS[native.SRC_PUSH]
    assert any(d.endswith("vine_env_push.h") for d in headers) and any(d.endswith("vine_named_draw.h") for d in headers)
    flags = native._flags(native.SRC_PUSH)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast") and "-ffp-contract=off" not in flags
    source = open(native.SRC_PUSH).read()
    assert source.index("#pragma clang fp contract(off)") < source.index("#include")
    assert "__shared__" not in source and "atomic" not in source.replace("no atomics", "")
    for word, slot in (("PUSH_RATE", 0), ("PUSH_IMPULSE", 1)):
        assert env_push.DRAW_NAMES[slot] == word
        assert env_params.name_key(word) == int.from_bytes(hashlib.sha256(word.encode()).digest()[:8], "little")


# ------------------------------------------------------------------------------------------- refusals of the entry point
def spec_call(lib, vcfg, spec, points=None, per_episode=None, mutate=None, device_values=0x1000):
    names, values = env_push.push_names(spec)
    if mutate:
        mutate(names)
    points = list(spec["POINTS"]) if points is None else points
    out = abi.VineEnvPushSpec()
    rc = lib.vine_env_push_spec(C.byref(vcfg), names, values.ctypes.data if len(values) else None,
                                device_values if len(values) else None, len(values), (C.c_int32 * max(len(points), 1))(*points),
                                len(points), int(spec["PER_EPISODE"]) if per_episode is None else per_episode, C.byref(out))
    return rc, lib.vine_last_error().decode(), out


def test_spec_entry_point_fills_and_refuses_by_name(lib, vcfg):
    good = config(RATE={"values": [0.0, 0.3, 1.0]}, IMPULSE=[0.0, 0.01], POINTS=[0, 2, 5])
    rc, _, out = spec_call(lib, vcfg, good)
    assert rc == abi.OK and out.checked == 1 and out.num_points == 3 and list(out.points) == [0, 2, 5, 0, 0, 0]
    assert out.seed == SEED and out.per_episode == 0 and out.num_values == 3
    assert [out.name[s].form for s in range(2)] == [abi.REDRAW_VALUES, abi.REDRAW_RANGE]
    assert [out.name[s].key for s in range(2)] == [env_params.name_key(n) for n in env_push.DRAW_NAMES]
    row = env_params.inertia_config_row(lib, vcfg)
    assert np.array_equal(bits(np.array(out.composites)), bits(row[abi.VI_MTOT:]))
    assert np.array_equal(bits(env_push.composites64(vcfg).astype(np.float32)), bits(row[abi.VI_MTOT:]))      # double, rounded once

    def setter(slot, **fields):
        def mutate(names):
            for k, v in fields.items():
                setattr(names[slot], k, v)
        return mutate
    refusals = [
        (dict(mutate=setter(0, form=abi.REDRAW_ABSENT)), "PUSH_RATE: absent"),
        (dict(mutate=setter(1, form=7)), "PUSH_IMPULSE: unknown form"),
        (dict(mutate=setter(1, reserved=1)), "PUSH_IMPULSE: reserved must be 0"),
        (dict(mutate=setter(1, lo=2.0, hi=1.0)), "PUSH_IMPULSE: a range needs finite lo <= hi"),
        (dict(mutate=setter(1, hi=float("inf"))), "PUSH_IMPULSE: a range needs finite lo <= hi"),
        (dict(mutate=setter(1, lo=-0.001)), "PUSH_IMPULSE: must not be negative"),
        (dict(mutate=setter(0, values_count=4)), "PUSH_RATE: the extent of the value list lies outside the values array"),
        (dict(mutate=setter(0, values_first=-1)), "PUSH_RATE: the extent of the value list lies outside the values array"),
        (dict(mutate=setter(0, radix=0)), "PUSH_RATE: radix must be at least 1"),
        (dict(points=[]), "POINTS: the list is empty"),
        (dict(points=[0, 1, 2, 3, 4, 5, 5]), "POINTS: more than VINE_PUSH_MAX_POINTS"),
        (dict(points=[0, 6]), "POINTS: a point index lies outside 0 .. 5"),
        (dict(points=[-1]), "POINTS: a point index lies outside 0 .. 5"),
        (dict(points=[2, 5, 2]), "POINTS: a point is listed twice"),
        (dict(device_values=None), "the value lists need a host and a device array"),
    ]
    for kw, match in refusals:
        rc, msg, out = spec_call(lib, vcfg, good, **kw)
        assert rc == abi.ERR_INVALID_ARG and match in msg and out.checked == 0, (kw, msg)
    for keys, match in ((dict(RATE={"values": [0.0, 1.5]}), "PUSH_RATE: must lie in [0, 1]"), (dict(RATE=[-0.1, 0.5]), "PUSH_RATE: must lie in [0, 1]"),
                        (dict(IMPULSE={"values": [0.01, float("nan")]}), "PUSH_IMPULSE: a listed value is not finite"),
                        (dict(RATE=float("nan")), "PUSH_RATE: the number is not finite")):
        rc, msg, _ = spec_call(lib, vcfg, dict(good, **keys))
        assert rc == abi.ERR_INVALID_ARG and match in msg, msg
    for keys, match in ((dict(RATE=0.0), "PUSH_RATE: constant zero: nothing to do"), (dict(IMPULSE=[0.0, 0.0]), "PUSH_IMPULSE: constant zero: nothing to do"),
                        (dict(RATE={"values": [0.0]}), "PUSH_RATE: constant zero: nothing to do")):
        zero = dict(good, **keys)
        rc, msg, _ = spec_call(lib, vcfg, zero)
        assert rc == abi.ERR_INVALID_ARG and match in msg, msg
        assert spec_call(lib, vcfg, zero, per_episode=1)[0] == abi.OK
    assert spec_call(lib, vcfg, dict(good, RATE=1.0))[0] == abi.OK                                  # both ends of [0, 1]
    assert lib.vine_env_push_spec(None, None, None, None, 0, None, 0, 0, None) == abi.ERR_INVALID_ARG
    assert "null argument to vine_env_push_spec" in lib.vine_last_error().decode()
    # the launch entry point: null pointers and an unchecked spec, refused before anything touches a device
    unchecked = abi.VineEnvPushSpec()
    unchecked.abi_version = abi.ENV_PUSH_ABI_VERSION
    out = spec_call(lib, vcfg, good)[2]
    assert lib.vine_env_push_scheduled(None, C.byref(out), 16, 16, 16, 16, None) == abi.ERR_INVALID_ARG
    assert "null argument to vine_env_push_scheduled" in lib.vine_last_error().decode()
    for k in range(4):                               # each of the four buffers in turn
        args = [16] * 4
        args[k] = None
        assert lib.vine_env_push_scheduled(0x10, C.byref(out), *args, None) == abi.ERR_INVALID_ARG
        assert "null argument to vine_env_push_scheduled" in lib.vine_last_error().decode()
    assert lib.vine_env_push_scheduled(0x10, None, *([16] * 4), None) == abi.ERR_INVALID_ARG
    assert lib.vine_env_push_scheduled(0x10, C.byref(unchecked), *([16] * 4), None) == abi.ERR_INVALID_ARG
    assert "was not filled by vine_env_push_spec" in lib.vine_last_error().decode()


# ---------------------------------------------------------------------------------------------------- the configuration
def test_default_is_off_and_every_config_error_names_the_key():
    cfg = load_config()["task"]
    assert cfg["env"]["ENV_PUSH"] == {} and env_push.push_config(cfg["env"]) is None and env_push.push_config({}) is None
    assert "task.env.ENV_PUSH" in __import__("vine_robot_isaacgymenvs_amd.cfg.defaults", fromlist=["x"]).__doc__
    good = config(RATE=[0.0, 0.1], IMPULSE={"values": [0.0, 0.01]}, POINTS=[5, 0, 2], PER_EPISODE=True)
    assert good == {"RATE": [0.0, 0.1], "IMPULSE": {"values": [0.0, 0.01]}, "POINTS": [5, 0, 2], "PER_EPISODE": True}
    assert config(RATE=1, IMPULSE=0.01) == {"RATE": 1.0, "IMPULSE": 0.01, "POINTS": [5], "PER_EPISODE": False}
    for keys, match in (
            (dict(RATE=0.1, IMPULSE=0.01, FORCE=2), "ENV_PUSH: unknown key.* FORCE"),
            (dict(RATE={"value": [1]}, IMPULSE=0.01), "ENV_PUSH.RATE: a mapping must hold the one key 'values'"),
            (dict(RATE={"values": []}, IMPULSE=0.01), "ENV_PUSH.RATE: 'values' must be a non-empty list"),
            (dict(RATE=0.1, IMPULSE=[0.1, 0.2, 0.3]), "ENV_PUSH.IMPULSE: a range is"),
            (dict(RATE=0.1, IMPULSE=[0.3, 0.1]), "ENV_PUSH.IMPULSE: lo > hi"),
            (dict(RATE="often", IMPULSE=0.01), "ENV_PUSH.RATE: 'often' is not a finite number"),
            (dict(RATE=True, IMPULSE=0.01), "ENV_PUSH.RATE: True is not a finite number"),
            (dict(RATE=1.5, IMPULSE=0.01), r"ENV_PUSH.RATE: 1.5 lies outside \[0, 1\]"),
            (dict(RATE=[-0.1, 0.5], IMPULSE=0.01), r"ENV_PUSH.RATE: -0.1 lies outside \[0, 1\]"),
            (dict(RATE=0.1, IMPULSE=-0.01), "ENV_PUSH.IMPULSE: -0.01 is negative"),
            (dict(RATE=0.1, IMPULSE=float("inf")), "ENV_PUSH.IMPULSE: inf is not a finite number"),
            (dict(RATE=0.1, IMPULSE={"values": [0.01, float("nan")]}), "ENV_PUSH.IMPULSE: nan is not a finite number"),
            (dict(RATE=0.1, IMPULSE=0.01, POINTS=[0, 6]), "ENV_PUSH.POINTS: point 6 lies outside 0 .. 5"),
            (dict(RATE=0.1, IMPULSE=0.01, POINTS=[-1]), "ENV_PUSH.POINTS: point -1 lies outside"),
            (dict(RATE=0.1, IMPULSE=0.01, POINTS=[2, 3, 2]), "ENV_PUSH.POINTS: point 2 is listed twice"),
            (dict(RATE=0.1, IMPULSE=0.01, POINTS=[]), "ENV_PUSH.POINTS is a non-empty list"),
            (dict(RATE=0.1, IMPULSE=0.01, POINTS="tip"), "ENV_PUSH.POINTS is a non-empty list"),
            (dict(RATE=0.1, IMPULSE=0.01, POINTS=[1.5]), "ENV_PUSH.POINTS: 1.5 is not a point index"),
            (dict(RATE=0.1, IMPULSE=0.01, PER_EPISODE="yes"), "ENV_PUSH.PER_EPISODE must be a bool"),
            (dict(IMPULSE=0.01), "ENV_PUSH.RATE is constant zero: nothing to do"),
            (dict(RATE=0.1), "ENV_PUSH.IMPULSE is constant zero: nothing to do"),
            (dict(RATE=0.1, IMPULSE=[0, 0]), "ENV_PUSH.IMPULSE is constant zero: nothing to do")):
        with pytest.raises(ConfigError, match=match):
            config(**keys)
    with pytest.raises(ConfigError, match="ENV_PUSH must be a mapping"):
        env_push.push_config({"ENV_PUSH": [1, 2]})
    assert config(RATE=0, PER_EPISODE=True)["PER_EPISODE"] is True       # per episode, constant zero is allowed to run


def test_sysid_forces_it_off_and_the_test_entry_keeps_it_on(caplog, monkeypatch, tmp_path):
    import logging
    from vine_robot_isaacgymenvs_amd import train
    from vine_robot_isaacgymenvs_amd.learning import a2c_continuous
    from vine_robot_isaacgymenvs_amd.utils import sysid
    assert ("env", "ENV_PUSH", {}) in sysid.FORCED
    cfg = load_config()["task"]
    cfg["env"]["ENV_PUSH"] = {"RATE": 0.05, "IMPULSE": 0.01}
    with caplog.at_level(logging.INFO):
        out = sysid.candidate_config(cfg, {"DAMPING": [0.01, 0.05]}, 70, 12)
    assert out["env"]["ENV_PUSH"] == {} and cfg["env"]["ENV_PUSH"] == {"RATE": 0.05, "IMPULSE": 0.01}
    assert any("ENV_PUSH forced from" in r.getMessage() for r in caplog.records)
    seen = {}
    monkeypatch.setattr(a2c_continuous.Runner, "run", lambda self, args: seen.update(args) or "ran")
    monkeypatch.chdir(tmp_path)
    cfg = load_config("config", overrides=["task.env.ENV_PUSH={RATE: 0.05, IMPULSE: {values: [0, 0.005, 0.01]}}", "test=True", "multi_gpu=False"])
    assert train.launch(cfg) == "ran" and seen["play"] is True
    assert cfg["task"]["env"]["ENV_PUSH"] == {"RATE": 0.05, "IMPULSE": {"values": [0, 0.005, 0.01]}}


# -------------------------------------------------------------------------------------------------------------- the draw
def test_draw_forms_episode_zero_and_a_shard(lib, vcfg):
    gids = np.arange(1000, 1070)
    spec = config(RATE=[0.0, 0.5], IMPULSE={"values": [0.0, 0.005, 0.01]})
    d0 = env_push.draw_push(spec, SEED, gids, 0)
    assert d0.dtype == np.float64 and d0.shape == (2, 70)
    u = env_params.uniform01(SEED, "PUSH_RATE", gids)                 # episode 0 is the set-up draw's hash
    assert np.array_equal(d0[0], 0.0 + (0.5 - 0.0) * u)
    assert np.array_equal(d0[1], np.asarray([0.0, 0.005, 0.01])[gids % 3])     # a value list counts the global id
    two = config(RATE={"values": [0.1, 1.0]}, IMPULSE={"values": [0.0, 0.005, 0.01]})
    d = env_push.draw_push(two, SEED, gids, 0)
    assert np.array_equal(d[0], np.asarray([0.1, 1.0])[gids % 2]) and np.array_equal(d[1], np.asarray([0.0, 0.005, 0.01])[(gids // 2) % 3])
    later = env_push.draw_push(spec, SEED, gids, np.arange(70) + 1)
    assert not np.array_equal(later[0], d0[0]) and set(later[1]) <= {0.0, 0.005, 0.01}
    u = env_params.uniform01_episode(SEED, "PUSH_IMPULSE", gids, np.arange(70) + 1)
    assert np.array_equal(later[1], np.asarray([0.0, 0.005, 0.01])[np.minimum(np.floor(u * 3.0).astype(int), 2)])
    assert np.array_equal(env_push.draw_push(config(RATE=0.25, IMPULSE=0.01), SEED, gids, 4), np.asarray([[0.25] * 70, [0.01] * 70]))
    # a shard draws what the whole batch would: the upper half of 70 envs is 35 envs at offset 35
    assert np.array_equal(env_push.draw_push(spec, SEED, np.arange(35, 70), 2), env_push.draw_push(spec, SEED, np.arange(70), 2)[:, 35:])
    # the replay's first table is episode 0's draw, rounded once
    geometry = env_push.geometry_of(lib, vcfg)
    rep = env_push.push_replay(hand_states(1, 70), np.zeros((1, 70)), spec, SEED, gids, [0], geometry)
    assert np.array_equal(bits(rep[0]["table"]), bits(d0.astype(np.float32)))
    whole = env_push.push_replay(hand_states(3, 70), np.zeros((3, 70)), spec, SEED, np.arange(70), [5, 6, 7], geometry)
    shard = env_push.push_replay(hand_states(3, 70)[:, :, 35:], np.zeros((3, 35)), spec, SEED, np.arange(35, 70), [5, 6, 7], geometry)
    for w, s in zip(whole, shard):
        assert np.array_equal(w["pushed"][35:], s["pushed"]) and np.array_equal(w["dqd"][35:], s["dqd"]) and np.array_equal(w["P"][35:], s["P"])


def test_the_draws_of_a_push():
    """65536 draws at p = 0.3: the standard error of the rate is sqrt(0.3 * 0.7 / 65536) = 0.00179, the bound five of them.
    The components lie in [-1, 1), are multiples of 2^-23, and every listed point occurs."""
    gids = np.arange(65536) + 77
    u, a, pick = env_push.push_draw(SEED, gids, 31, 3)
    assert u.dtype == np.float32 and a.dtype == np.float32 and a.shape == (65536, 2)
    for p in (0.05, 0.3, 0.9):
        rate = float((u < np.float32(p)).mean())
        print("rate at p = %g: %.5f" % (p, rate))
        assert abs(rate - p) < 5.0 * np.sqrt(p * (1.0 - p) / 65536.0)
    assert u.min() >= 0.0 and u.max() < 1.0 and not (u < np.float32(0.0)).any() and (u < np.float32(1.0)).all()
    assert a.min() >= -1.0 and a.max() < 1.0 and a.min() < -0.999 and a.max() > 0.999
    assert np.array_equal(a.astype(np.float64) * 2.0 ** 23, np.round(a.astype(np.float64) * 2.0 ** 23))      # exact in float32
    assert abs(float(a.mean())) < 5.0 * np.sqrt(1.0 / 3.0 / 131072.0)
    assert sorted(set(pick.tolist())) == [0, 1, 2] and np.bincount(pick).min() > 65536 / 3 - 5 * np.sqrt(65536 * 2 / 9)
    for count in (1, 6):
        assert sorted(set(env_push.push_draw(SEED, gids, 31, count)[2].tolist())) == list(range(count))
    other = env_push.push_draw(SEED, gids[:8], 2 ** 32 + 31, 3)
    assert not np.array_equal(other[0], u[:8])                       # the high word of the step is keyed


# ------------------------------------------------------------------------------------------------------------ the replay
def test_horizontal_momentum_and_the_cart_push(lib, vcfg):
    """Row 0 of M D is the horizontal momentum the impulse adds: P_y, for every point.  A push on the cart with P_z only is
    taken by the rail: nothing changes."""
    geometry = exact_geometry(lib, vcfg)
    st = hand_states(1, 40)[0]
    q = st[abi.VF_Q0:abi.VF_Q0 + ND].T.astype(np.float64)
    rng = np.random.default_rng(3)
    cm = np.repeat(geometry["composites"][None], 40, axis=0)
    M, _, _ = env_push.mass_matrix(q, cm, geometry["s0"], geometry["c0"])
    assert np.array_equal(M, M.transpose(0, 2, 1)) and (np.linalg.eigvalsh(M) > 0).all()
    for point in range(6):
        P = rng.uniform(-0.01, 0.01, (40, 2))
        dqd = env_push.impulse_response(q, P, np.full(40, point), cm, geometry)
        D = dqd.copy()
        D[:, 1:] = np.cumsum(dqd[:, 1:], axis=1)                     # back to the absolute coordinates
        momentum = np.einsum("bj,bj->b", M[:, 0], D)
        assert np.abs(momentum - P[:, 0]).max() <= 1e-10 * np.abs(P[:, 0]).max(), point
        assert np.abs(dqd).max() > 1e-3
    Pz = np.stack([np.zeros(40), rng.uniform(-0.01, 0.01, 40)], axis=1)
    assert not env_push.impulse_response(q, Pz, np.zeros(40, dtype=int), cm, geometry).any()
    for dtype in (np.float32, np.float64):
        out = env_push.impulse_response(q, Pz, np.zeros(40, dtype=int), cm, geometry, dtype)
        assert out.dtype == dtype and not out.any()


def test_the_solve_is_the_oracles_forward_dynamics(lib, vcfg):
    """dqd = forward_dynamics(eff = J^T P in relative coordinates, h = 0) - forward_dynamics(eff = 0), in float64, at the 1e-10
    relative that tests/test_oracle_physics.py uses between formulations.  The oracle's call is its absolute-angle formulation
    (fd_abs, the one the header names; that the other two agree with it is test_oracle_physics.py's subject).

    "Relative" is what it is there: |difference| / (1 + max |acceleration|).  The reference is a difference of two
    accelerations of 2e3 .. 1.5e4 (light links at +-3 rad/s), each rounded at its own size, for a dqd of 0.05 .. 30: relative
    to max |dqd| the same difference reads up to 1.7e-10, all of it the reference's cancellation (measured: 3e-16 on the
    scale above).  So the solve itself is also held against numpy's LU solve of the same matrix, at 1e-10 relative to
    max |dqd| (condition number 6e4: expected 1e-11 or better; measured 1.4e-14)."""
    geometry = exact_geometry(lib, vcfg)
    n = 60
    st = hand_states(1, n, seed=9)
    spec = config(RATE=1.0, IMPULSE=[0.002, 0.01], POINTS=[0, 1, 2, 3, 4, 5])
    rep = env_push.push_replay(st, np.zeros((1, n)), spec, SEED, np.arange(n), [4], geometry)[0]
    assert rep["pushed"].all() and sorted(set(rep["point"].tolist())) == [0, 1, 2, 3, 4, 5]
    cm = np.repeat(geometry["composites"][None], n, axis=0)
    q = st[0, abi.VF_Q0:abi.VF_Q0 + ND].T.astype(np.float64)
    qd = st[0, abi.VF_QD0:abi.VF_QD0 + ND].T.astype(np.float64)
    M, sp, cp = env_push.mass_matrix(q, cm, geometry["s0"], geometry["c0"])
    Q = env_push.generalised_impulse(rep["P"], rep["point"], sp, cp, geometry["L"])
    worst, worst_of_dqd, worst_lu = 0.0, 0.0, 0.0
    for e in range(n):
        pushed = vo.forward_dynamics(vcfg, q[e], qd[e], relative_effort(Q[e]), 0.0)
        want = pushed - vo.forward_dynamics(vcfg, q[e], qd[e], np.zeros(6), 0.0)
        worst = max(worst, np.abs(rep["dqd"][e] - want).max() / (1 + np.abs(pushed).max()))
        worst_of_dqd = max(worst_of_dqd, np.abs(rep["dqd"][e] - want).max() / np.abs(want).max())
        lu = env_push.to_relative(np.linalg.solve(M[e], Q[e])[None])[0]
        worst_lu = max(worst_lu, np.abs(rep["dqd"][e] - lu).max() / np.abs(lu).max())
    print("solve against the oracle: worst %.3g of 1 + max |acceleration|, %.3g of max |dqd|; against numpy's LU %.3g of max |dqd|"
          % (worst, worst_of_dqd, worst_lu))
    assert worst < 1e-10 and worst_lu < 1e-10


def test_kinetic_energy_of_a_tip_push(lib, vcfg):
    """For an impulse at the tip, the energy gained is P . (v_before + v_after) / 2 with the tip's velocities (positions do
    not move, so the potential part cancels)."""
    geometry = exact_geometry(lib, vcfg)
    n = 60
    st = hand_states(1, n, seed=11)
    spec = config(RATE=1.0, IMPULSE=0.01)
    rep = env_push.push_replay(st, np.zeros((1, n)), spec, SEED, np.arange(n), [8], geometry)[0]
    assert rep["pushed"].all() and (rep["point"] == 5).all()
    q = st[0, abi.VF_Q0:abi.VF_Q0 + ND].T.astype(np.float64)
    qd = st[0, abi.VF_QD0:abi.VF_QD0 + ND].T.astype(np.float64)
    for e in range(n):
        e0, e1 = vo.energy(vcfg, q[e], qd[e]), vo.energy(vcfg, q[e], rep["qd"][e])
        v0, v1 = vo.tip(vcfg, q[e], qd[e])[2:], vo.tip(vcfg, q[e], rep["qd"][e])[2:]
        work = float(np.dot(rep["P"][e].astype(np.float64), (v0 + v1) / 2.0))
        assert abs((e1 - e0) - work) <= 1e-10 * (abs(e0) + abs(e1)), (e, e1 - e0, work)
        assert abs(work) > 1e-6


def test_no_push_at_reset_the_zero_cases_and_per_episode(lib, vcfg):
    geometry = env_push.geometry_of(lib, vcfg)
    n, steps = 24, 20
    st = hand_states(steps, n, seed=5)
    st[3, abi.VF_QD0 + 2, 4] = np.float32(-0.0)
    reset = np.zeros((steps, n), dtype=np.int64)
    reset[:, 1::3] = 1
    reset[7, 0] = reset[12, 0] = reset[12, 3] = 1
    gids = np.arange(n) + 1000
    spec = config(RATE=1.0, IMPULSE=[0.002, 0.01], PER_EPISODE=True, POINTS=[0, 2, 5])
    for dtype in (np.float64, np.float32):
        rep = env_push.push_replay(st, reset, spec, SEED, gids, np.arange(steps), geometry, dtype=dtype)
        episode, count = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for t in range(steps):
            assert np.array_equal(rep[t]["pushed"], reset[t] == 0)                       # RATE 1: everybody but the flagged
            assert not rep[t]["dqd"][reset[t] != 0].any() and not rep[t]["P"][reset[t] != 0].any()
            assert rep[t]["dqd"][reset[t] == 0].any(axis=1).all() and rep[t]["dqd"].dtype == dtype
            assert np.array_equal(rep[t]["qd"][reset[t] != 0], st[t, abi.VF_QD0:abi.VF_QD0 + ND].T[reset[t] != 0].astype(dtype))
            assert set(rep[t]["point"].tolist()) <= {0, 2, 5}
            episode += reset[t]
            count += reset[t] == 0
            assert np.array_equal(rep[t]["episode_index"], episode) and np.array_equal(rep[t]["push_count"], count)
            assert np.array_equal(bits(rep[t]["table"]), bits(env_push.draw_push(spec, SEED, gids, episode).astype(np.float32)))
    held = env_push.push_replay(st, reset, dict(spec, PER_EPISODE=False), SEED, gids, np.arange(steps), geometry)
    table0 = env_push.draw_push(spec, SEED, gids, 0).astype(np.float32)
    assert all(np.array_equal(bits(r["table"]), bits(table0)) and not r["episode_index"].any() for r in held)
    # RATE 0 or IMPULSE 0 leaves every bit: nothing is stored, a -0 stays a -0
    quiet = np.zeros((steps, n), dtype=np.int64)
    for keys, pushed in ((dict(RATE=0.0, IMPULSE=0.01), False), (dict(RATE=1.0, IMPULSE=0.0), True)):
        rep = env_push.push_replay(st, quiet, dict(spec, **keys), SEED, gids, np.arange(steps), geometry, dtype=np.float32)
        for t in range(steps):
            assert rep[t]["pushed"].all() == pushed and rep[t]["pushed"].any() == pushed and not rep[t]["stored"].any()
            assert np.array_equal(bits(rep[t]["qd"]), bits(st[t, abi.VF_QD0:abi.VF_QD0 + ND].T))
        assert np.signbit(rep[3]["qd"][4, 2])
    # float32 restates float64: the same pushes, close velocities
    a = env_push.push_replay(st, reset, spec, SEED, gids, np.arange(steps), geometry)
    b = env_push.push_replay(st, reset, spec, SEED, gids, np.arange(steps), geometry, dtype=np.float32)
    for x, y in zip(a, b):
        assert np.array_equal(x["pushed"], y["pushed"]) and np.array_equal(bits(x["P"]), bits(y["P"])) and np.array_equal(x["point"], y["point"])
        f = x["stored"]
        assert y["qd"].dtype == np.float32 and (np.abs(y["dqd"][f] - x["dqd"][f]).max(axis=1) / np.abs(x["dqd"][f]).max(axis=1)).max() < 1e-3


# ------------------------------------------------------------------------------------------------- the episode log's join
def rows_of(env, end_step, **more):
    rows = {name: np.zeros(len(env)) for name in episodes.COLUMNS}
    rows.update(env=np.asarray(env, dtype=np.int64), end_step=np.asarray(end_step, dtype=np.int64), **more)
    return rows


def test_log_join_and_file_round_trip(tmp_path):
    offset = 1000
    held = config(RATE=0.05, IMPULSE={"values": [0.0, 0.005, 0.01]})
    rows = rows_of([0, 1, 2, 4, 1], [5, 6, 7, 8, 9])
    params = lambda spec: (lambda envs, eps: env_push.episode_params(spec, SEED, np.asarray(envs) + offset, eps))      # noqa: E731
    out = episodes.with_push_params(rows, params(held))
    assert [k for k in out if k.startswith("param_")] == ["param_PUSH_IMPULSE"]       # only the names that vary
    assert np.array_equal(out["param_PUSH_IMPULSE"], np.asarray([0, 0.005, 0.01], dtype=np.float32)[(np.asarray([0, 1, 2, 4, 1]) + offset) % 3])
    spec = config(RATE=[0.0, 0.1], IMPULSE=[0.0, 0.02], PER_EPISODE=True)
    env, end = np.asarray([3, 0, 3, 69]), np.asarray([4, 9, 11, 12])
    rows = rows_of(env, end, episode=np.asarray([0, 0, 1, 0]))
    out = episodes.with_push_params(rows, params(spec))
    expect = env_push.draw_push(spec, SEED, env + offset, [0, 0, 1, 0]).astype(np.float32)
    assert sorted(k for k in out if k.startswith("param_")) == ["param_PUSH_IMPULSE", "param_PUSH_RATE"]
    assert np.array_equal(bits(out["param_PUSH_RATE"]), bits(expect[0])) and np.array_equal(bits(out["param_PUSH_IMPULSE"]), bits(expect[1]))
    path = str(tmp_path / "episodes.npz")
    episodes.save(path, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {}, push={"spec": spec, "seed": SEED, "env_id_offset": offset})
    loaded_spec, episode, push_params = episodes.load_env_push(path)
    assert loaded_spec == spec and episode.tolist() == [0, 0, 1, 0]
    back = episodes.load_rows_with_params(path)
    for slot, name in enumerate(env_push.DRAW_NAMES):
        assert np.array_equal(bits(back["param_" + name]), bits(expect[slot])) and np.array_equal(bits(push_params(env, [0, 0, 1, 0])[name]), bits(expect[slot]))
    assert back["episode"].tolist() == [0, 0, 1, 0] and np.array_equal(back["env"], env)
    plain = str(tmp_path / "plain.npz")
    episodes.save(plain, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {})
    assert episodes.load_env_push(plain) == (None, None, None)
    assert not any(k.startswith("param_") for k in episodes.load_rows_with_params(plain))
