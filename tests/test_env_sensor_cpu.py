"""ENV_SENSOR without a GPU: include/vine_env_sensor.h against its ctypes mirror, every refusal of its host entry point and
of the configuration, the draw, utils/env_sensor.py sensor_replay on hand-made sequences (the properties the header states),
the deviate's moments, the episode log's join and file round trip, and the contraction check of the device code.  Every
comparison of values is bit for bit or on integers."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, load_config, native
from vine_robot_isaacgymenvs_amd.utils import env_params, env_sensor, episodes
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_OBS = 28
SEED = 42


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.load()


@pytest.fixture()
def vcfg(lib):
    c = abi.VineConfig()
    assert lib.vine_config_default(C.byref(c)) == 0
    assert lib.vine_config_set_obs_type(C.byref(c), abi.OBS_TYPE_BY_NAME["POS_AND_FD_VEL_AND_OBJ_INFO"], 0) == 0
    c.seed = SEED
    return c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def config(num_obs=NUM_OBS, **keys):
    return env_sensor.sensor_config({"ENV_SENSOR": keys}, num_obs)


def pattern(steps, n, num_obs=NUM_OBS):
    """A recognisable observation of (step, env, column), exact in float32 and inside +-5."""
    t, e, j = np.meshgrid(np.arange(steps), np.arange(n), np.arange(num_obs), indexing="ij")
    return ((t + 1) / 64.0 + e / 4096.0 + j / 262144.0).astype(np.float32)


def episodes_of(lengths, steps):
    """progress [T] of one env whose episodes have the given lengths: 0 at the first frame of each."""
    out = []
    for length in lengths:
        out += list(range(length))
    return np.asarray((out + list(range(steps)))[:steps], dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_equals_the_mirror_and_the_struct_size(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vine_env_sensor.h")).read(), flags=re.S)
    for macro, value in (("VINE_ENV_SENSOR_ABI_VERSION", abi.ENV_SENSOR_ABI_VERSION), ("VINE_ENV_SENSOR_THREADS", abi.ENV_SENSOR_THREADS),
                         ("VINE_SENSOR_MAX_DELAY", abi.SENSOR_MAX_DELAY), ("VINE_SENSOR_RNG_NOISE", abi.SENSOR_RNG_NOISE),
                         ("VINE_SENSOR_RNG_HOLD", abi.SENSOR_RNG_HOLD)):
        assert int(re.search(r"#define %s (\d+)u?\s" % macro, text).group(1)) == value, macro
    assert abi.SENSOR_MAX_DELAY == abi.MAX_DELAY == 8 and abi.SENSOR_SLOTS == 9
    assert re.search(r"#define VINE_SENSOR_SLOTS \(VINE_SENSOR_MAX_DELAY \+ 1\)", text)
    hip = open(os.path.join(REPO, "vine_robot_isaacgymenvs_amd", "csrc", "vine_hip.hip")).read()
    used = [int(v) for v in re.findall(r"RNG_\w+ = (\d+)", re.search(r"enum \{ (RNG_RESET.*?)\};", hip).group(1))]
    assert max(used) == 4 and abi.SENSOR_RNG_NOISE not in used and abi.SENSOR_RNG_HOLD not in used
    slots = re.search(r"typedef enum VineEnvSensorSlot \{(.*?)\}", text, flags=re.S).group(1)
    assert [w.split("=")[0].strip() for w in slots.split(",")] == ["VSN_DELAY", "VSN_HOLD", "VSN_NOISE_STD", "VSN_NAMES"]
    assert ["VSN_" + n for n in abi.ENV_SENSOR_NAMES] == ["VSN_DELAY", "VSN_HOLD", "VSN_NOISE_STD"] and abi.VSN_NAMES == 3
    body = re.search(r"typedef struct VineEnvSensorSpec \{(.*?)\} VineEnvSensorSpec;", text, flags=re.S).group(1)
    fields = [f for decl in body.split(";") if decl.strip()
              for f in re.sub(r"\[.*?\]", "", decl.strip().split(None, 1)[-1]).replace(" ", "").replace("double*", "").split(",")]
    assert [f.split()[-1] if " " in f else f for f in fields] == [f[0] for f in abi.VineEnvSensorSpec._fields_]
    assert lib.vine_env_sensor_spec_size() == C.sizeof(abi.VineEnvSensorSpec) == 24 + 3 * 48 + 24 == 192
    functions = sorted(set(re.findall(r"\b(vine_env_sensor[a-z_0-9]*)\s*\(", text)))
    assert functions == sorted(abi.ENV_SENSOR_PROTOTYPES)
    for name in functions:
        assert hasattr(lib, name), name
    # the ninth translation unit, behind the eight; its pragma, the flag that makes the compiler honour it, its headers
    assert native.UNITS == native.SOURCES + (native.SRC_SENSOR,) and len(native.UNITS) == 9
    assert native.SRC_SENSOR in native.DEPS and any(d.endswith("vine_env_sensor.h") for d in native.DEPS)
    assert any(d.endswith("vine_env_sensor.h") for d in native._SOURCE_HEADERS[native.SRC_SENSOR])
    flags = native._flags(native.SRC_SENSOR)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast") and "-ffp-contract=off" not in flags
    source = open(native.SRC_SENSOR).read()
    assert source.index("#pragma clang fp contract(off)") < source.index("#include")
    for word, slot in (("SENSOR_DELAY", 0), ("SENSOR_HOLD", 1), ("SENSOR_NOISE_STD", 2)):
        assert env_sensor.DRAW_NAMES[slot] == word
        assert env_params.name_key(word) == int.from_bytes(hashlib.sha256(word.encode()).digest()[:8], "little")


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10 through the numpy statement the replay uses."""
    for ctr, key, expect in (([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                             ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                             ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
                              [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        assert [int(w) for w in env_sensor.philox4x32_10(*ctr, *key)] == expect


# ------------------------------------------------------------------------------------------- refusals of the entry point
def spec_call(lib, vcfg, spec, mask=None, per_episode=None, mutate=None, device_values=0x1000):
    names, values = env_sensor.sensor_names(spec)
    if mutate:
        mutate(names)
    out = abi.VineEnvSensorSpec()
    rc = lib.vine_env_sensor_spec(C.byref(vcfg), names, values.ctypes.data if len(values) else None,
                                  device_values if len(values) else None, len(values),
                                  env_sensor.column_mask(spec) if mask is None else mask,
                                  int(spec["PER_EPISODE"]) if per_episode is None else per_episode, C.byref(out))
    return rc, lib.vine_last_error().decode(), out


def test_spec_entry_point_fills_and_refuses_by_name(lib, vcfg):
    good = config(DELAY=[0, 8], HOLD={"values": [0.0, 0.3, 0.9]}, NOISE_STD=0.01, COLUMNS=[1, 2, 26])
    rc, _, out = spec_call(lib, vcfg, good)
    assert rc == abi.OK and out.checked == 1 and out.num_obs == NUM_OBS and out.column_mask == (1 << 1 | 1 << 2 | 1 << 26)
    assert out.seed == SEED and out.per_episode == 0 and out.clip_observations == vcfg.clip_observations and out.num_values == 3
    assert [out.name[s].form for s in range(3)] == [abi.REDRAW_RANGE, abi.REDRAW_VALUES, abi.REDRAW_NUMBER]
    assert [out.name[s].key for s in range(3)] == [env_params.name_key(n) for n in env_sensor.DRAW_NAMES]

    def setter(slot, **fields):
        def mutate(names):
            for k, v in fields.items():
                setattr(names[slot], k, v)
        return mutate
    refusals = [
        (dict(mutate=setter(0, form=abi.REDRAW_ABSENT)), "SENSOR_DELAY: absent"),
        (dict(mutate=setter(1, form=7)), "SENSOR_HOLD: unknown form"),
        (dict(mutate=setter(2, reserved=1)), "SENSOR_NOISE_STD: reserved must be 0"),
        (dict(mutate=setter(0, lo=2.0, hi=1.0)), "SENSOR_DELAY: a range needs finite lo <= hi"),
        (dict(mutate=setter(0, hi=float("inf"))), "SENSOR_DELAY: a range needs finite lo <= hi"),
        (dict(mutate=setter(0, lo=0.5)), "SENSOR_DELAY: must be an integer in 0 .. VINE_SENSOR_MAX_DELAY"),
        (dict(mutate=setter(0, hi=9.0)), "SENSOR_DELAY: must be an integer in 0 .. VINE_SENSOR_MAX_DELAY"),
        (dict(mutate=setter(0, lo=-1.0)), "SENSOR_DELAY: must be an integer in 0 .. VINE_SENSOR_MAX_DELAY"),
        (dict(mutate=setter(1, values_count=4)), "SENSOR_HOLD: the extent of the value list lies outside the values array"),
        (dict(mutate=setter(1, values_first=-1)), "SENSOR_HOLD: the extent of the value list lies outside the values array"),
        (dict(mutate=setter(1, radix=0)), "SENSOR_HOLD: radix must be at least 1"),
        (dict(mutate=setter(2, lo=-0.01)), "SENSOR_NOISE_STD: must not be negative"),
        (dict(mutate=setter(2, lo=float("nan"))), "SENSOR_NOISE_STD: the number is not finite"),
        (dict(mask=0), "COLUMNS: the mask is empty"),
        (dict(mask=1 << 28), "COLUMNS: a column index lies outside"),
        (dict(device_values=None), "the value lists need a host and a device array"),
    ]
    for kw, match in refusals:
        rc, msg, out = spec_call(lib, vcfg, good, **kw)
        assert rc == abi.ERR_INVALID_ARG and match in msg and out.checked == 0, (kw, msg)
    for hold, match in (({"values": [0.0, 1.0]}, "SENSOR_HOLD: must lie in [0, 1)"), ([-0.1, 0.5], "SENSOR_HOLD: must lie in [0, 1)")):
        bad = dict(good, HOLD=hold)
        rc, msg, _ = spec_call(lib, vcfg, bad)
        assert rc == abi.ERR_INVALID_ARG and match in msg, msg
    zero = dict(good, DELAY=0.0, HOLD=[0.0, 0.0], NOISE_STD={"values": [0.0]})
    rc, msg, _ = spec_call(lib, vcfg, zero)
    assert rc == abi.ERR_INVALID_ARG and "all constant zero: nothing to do" in msg
    assert spec_call(lib, vcfg, zero, per_episode=1)[0] == abi.OK          # its next episode may draw ... the same, but it may run
    assert lib.vine_env_sensor_spec(None, None, None, None, 0, 1, 0, None) == abi.ERR_INVALID_ARG
    assert "null argument to vine_env_sensor_spec" in lib.vine_last_error().decode()
    # the launch entry point: null pointers and an unchecked spec, refused before anything touches a device
    unchecked = abi.VineEnvSensorSpec()
    unchecked.abi_version = abi.ENV_SENSOR_ABI_VERSION
    out = spec_call(lib, vcfg, good)[2]
    assert lib.vine_env_sensor_scheduled(None, C.byref(out), 16, 16, 16, 16, 16, 16, 16, None) == abi.ERR_INVALID_ARG
    assert "null argument to vine_env_sensor_scheduled" in lib.vine_last_error().decode()
    for k in range(7):                               # each of the seven buffers in turn
        args = [16] * 7
        args[k] = None
        assert lib.vine_env_sensor_scheduled(0x10, C.byref(out), *args, None) == abi.ERR_INVALID_ARG
        assert "null argument to vine_env_sensor_scheduled" in lib.vine_last_error().decode()
    assert lib.vine_env_sensor_scheduled(0x10, None, *([16] * 7), None) == abi.ERR_INVALID_ARG
    assert lib.vine_env_sensor_scheduled(0x10, C.byref(unchecked), *([16] * 7), None) == abi.ERR_INVALID_ARG
    assert "was not filled by vine_env_sensor_spec" in lib.vine_last_error().decode()


# ---------------------------------------------------------------------------------------------------- the configuration
def test_default_is_off_and_every_config_error_names_the_key():
    cfg = load_config()["task"]
    assert cfg["env"]["ENV_SENSOR"] == {} and env_sensor.sensor_config(cfg["env"], NUM_OBS) is None
    assert env_sensor.sensor_config({}, NUM_OBS) is None
    assert "task.env.ENV_SENSOR" in __import__("vine_robot_isaacgymenvs_amd.cfg.defaults", fromlist=["x"]).__doc__
    good = config(DELAY=[0, 3], HOLD=0.25, NOISE_STD={"values": [0.0, 0.01]}, COLUMNS=[3, 1, 2], PER_EPISODE=True)
    assert good == {"DELAY": [0.0, 3.0], "HOLD": 0.25, "NOISE_STD": {"values": [0.0, 0.01]}, "COLUMNS": [1, 2, 3], "PER_EPISODE": True}
    assert config(DELAY=2)["COLUMNS"] == list(range(NUM_OBS)) and config(18, DELAY=2, COLUMNS="all")["COLUMNS"] == list(range(18))
    for keys, match in (
            (dict(DELAY=1, LATENCY=2), "ENV_SENSOR: unknown key.* LATENCY"),
            (dict(DELAY={"value": [1]}), "ENV_SENSOR.DELAY: a mapping must hold the one key 'values'"),
            (dict(DELAY={"values": []}), "ENV_SENSOR.DELAY: 'values' must be a non-empty list"),
            (dict(HOLD=[0.1, 0.2, 0.3]), "ENV_SENSOR.HOLD: a range is"),
            (dict(HOLD=[0.3, 0.1]), "ENV_SENSOR.HOLD: lo > hi"),
            (dict(NOISE_STD="big"), "ENV_SENSOR.NOISE_STD: 'big' is not a finite number"),
            (dict(NOISE_STD=True), "ENV_SENSOR.NOISE_STD: True is not a finite number"),
            (dict(DELAY=1.5), "ENV_SENSOR.DELAY: 1.5 is not an integer in 0 .. 8"),
            (dict(DELAY=[0, 9]), "ENV_SENSOR.DELAY: 9 is not an integer in 0 .. 8"),
            (dict(DELAY={"values": [0, -1]}), "ENV_SENSOR.DELAY: -1 is not an integer in 0 .. 8"),
            (dict(HOLD=1.0), r"ENV_SENSOR.HOLD: 1 lies outside \[0, 1\)"),
            (dict(HOLD=[-0.1, 0.5]), r"ENV_SENSOR.HOLD: -0.1 lies outside \[0, 1\)"),
            (dict(NOISE_STD=-0.01), "ENV_SENSOR.NOISE_STD: -0.01 is negative"),
            (dict(DELAY=1, COLUMNS=[0, 28]), r"ENV_SENSOR.COLUMNS: column 28 lies outside \[0, 28\)"),
            (dict(DELAY=1, COLUMNS=[-1]), "ENV_SENSOR.COLUMNS: column -1 lies outside"),
            (dict(DELAY=1, COLUMNS=[2, 3, 2]), "ENV_SENSOR.COLUMNS: column 2 is listed twice"),
            (dict(DELAY=1, COLUMNS=[]), "ENV_SENSOR.COLUMNS is 'all' or a non-empty list"),
            (dict(DELAY=1, COLUMNS="some"), "ENV_SENSOR.COLUMNS is 'all' or a list"),
            (dict(DELAY=1, COLUMNS=[1.5]), "ENV_SENSOR.COLUMNS: 1.5 is not a column index"),
            (dict(DELAY=1, PER_EPISODE="yes"), "ENV_SENSOR.PER_EPISODE must be a bool"),
            (dict(DELAY=0, HOLD=[0, 0]), "ENV_SENSOR: DELAY, HOLD and NOISE_STD are all constant zero: nothing to do")):
        with pytest.raises(ConfigError, match=match):
            config(**keys)
    with pytest.raises(ConfigError, match=r"column 18 lies outside \[0, 18\)"):
        config(18, DELAY=1, COLUMNS=[18])
    with pytest.raises(ConfigError, match="ENV_SENSOR must be a mapping"):
        env_sensor.sensor_config({"ENV_SENSOR": [1, 2]}, NUM_OBS)
    assert config(DELAY=0, PER_EPISODE=True)["PER_EPISODE"] is True      # per episode, all zero is allowed to run


def test_sysid_forces_it_off_and_the_test_entry_keeps_it_on(caplog, monkeypatch, tmp_path):
    import logging
    from vine_robot_isaacgymenvs_amd import train
    from vine_robot_isaacgymenvs_amd.learning import a2c_continuous
    from vine_robot_isaacgymenvs_amd.utils import sysid
    assert ("env", "ENV_SENSOR", {}) in sysid.FORCED
    cfg = load_config()["task"]
    cfg["env"]["ENV_SENSOR"] = {"DELAY": [0, 3]}
    with caplog.at_level(logging.INFO):
        out = sysid.candidate_config(cfg, {"DAMPING": [0.01, 0.05]}, 70, 12)
    assert out["env"]["ENV_SENSOR"] == {} and cfg["env"]["ENV_SENSOR"] == {"DELAY": [0, 3]}
    assert any("ENV_SENSOR forced from" in r.getMessage() for r in caplog.records)
    seen = {}
    monkeypatch.setattr(a2c_continuous.Runner, "run", lambda self, args: seen.update(args) or "ran")
    monkeypatch.chdir(tmp_path)
    cfg = load_config("config", overrides=["task.env.ENV_SENSOR={DELAY: {values: [0, 2, 4]}, COLUMNS: [0, 1]}", "test=True", "multi_gpu=False"])
    assert train.launch(cfg) == "ran" and seen["play"] is True
    assert cfg["task"]["env"]["ENV_SENSOR"] == {"DELAY": {"values": [0, 2, 4]}, "COLUMNS": [0, 1]}


# -------------------------------------------------------------------------------------------------------------- the draw
def test_draw_forms_and_episode_zero():
    gids = np.arange(1000, 1070)
    spec = config(DELAY=[0, 8], HOLD={"values": [0.0, 0.3, 0.9]}, NOISE_STD=0.01)
    d0 = env_sensor.draw_sensor(spec, SEED, gids, 0)
    assert d0.dtype == np.float64 and d0.shape == (3, 70)
    assert np.array_equal(d0[2], np.full(70, 0.01)) and np.array_equal(env_sensor.draw_sensor(spec, SEED, gids, 5)[2], np.full(70, 0.01))
    u = env_params.uniform01(SEED, "SENSOR_DELAY", gids)              # episode 0 is the set-up draw's hash
    assert np.array_equal(d0[0], np.minimum(np.floor(u * 9.0), 8.0)) and set(d0[0]) <= set(range(9)) and len(set(d0[0])) > 4
    assert np.array_equal(d0[1], np.asarray([0.0, 0.3, 0.9])[gids % 3])     # a value list counts the global id
    two = config(DELAY={"values": [0, 2, 4]}, HOLD={"values": [0.0, 0.5]})
    d = env_sensor.draw_sensor(two, SEED, gids, 0)
    assert np.array_equal(d[0], np.asarray([0.0, 2.0, 4.0])[gids % 3]) and np.array_equal(d[1], np.asarray([0.0, 0.5])[(gids // 3) % 2])
    later = env_sensor.draw_sensor(spec, SEED, gids, np.arange(70) + 1)
    assert not np.array_equal(later[0], d0[0]) and set(later[1]) <= {0.0, 0.3, 0.9} and set(later[0]) <= set(range(9))
    u = env_params.uniform01_episode(SEED, "SENSOR_HOLD", gids, np.arange(70) + 1)
    assert np.array_equal(later[1], np.asarray([0.0, 0.3, 0.9])[np.minimum(np.floor(u * 3.0).astype(int), 2)])
    cont = env_sensor.draw_sensor(config(HOLD=[0.1, 0.6]), SEED, gids, 3)[1]
    assert np.array_equal(cont, 0.1 + (0.6 - 0.1) * env_params.uniform01_episode(SEED, "SENSOR_HOLD", gids, 3))
    # a shard draws what the whole batch would: the upper half of 70 envs is 35 envs at offset 35
    assert np.array_equal(env_sensor.draw_sensor(spec, SEED, np.arange(35, 70), 2), env_sensor.draw_sensor(spec, SEED, np.arange(70), 2)[:, 35:])
    # the replay's first table is episode 0's draw, rounded once
    rep = env_sensor.sensor_replay(spec, SEED, gids, [0], pattern(1, 70), np.zeros((1, 70)), np.zeros((1, 70)))
    assert np.array_equal(bits(rep[0]["table"]), bits(d0.astype(np.float32)))


# ------------------------------------------------------------------------------------------------------------ the replay
def fixed(delay=0, hold=0.0, std=0.0, n=1):
    return np.repeat(np.asarray([[delay], [hold], [std]], dtype=np.float32), n, axis=1)


def test_all_zero_settings_are_the_identity_in_bits():
    spec = config(DELAY=0, PER_EPISODE=True)
    raw = pattern(30, 5)
    raw[3, 2, 7] = np.float32(-0.0)
    progress = np.stack([episodes_of([7, 5, 9], 30)] * 5, axis=1)
    rep = env_sensor.sensor_replay(spec, SEED, np.arange(5), np.arange(30), raw, progress, progress == 0, clip=5.0)
    for t in range(30):
        assert np.array_equal(bits(rep[t]["obs"]), bits(raw[t]))
        assert np.array_equal(bits(rep[t]["ring"][t % 9]), bits(raw[t])) and not rep[t]["held"].any()


def test_delay_delivers_frame_t_minus_d_and_no_frame_crosses_an_episode():
    spec = config(DELAY=3, COLUMNS=list(range(1, 27)))
    raw = pattern(40, 1)
    progress = episodes_of([11, 4, 2, 12], 40)
    starts = np.flatnonzero(progress == 0)
    for step0 in (0, 5, 123456789012):           # the slots follow the device's count, wherever it starts
        rep = env_sensor.sensor_replay(spec, SEED, [7], step0 + np.arange(40), raw, progress[:, None], np.zeros((40, 1)), clip=5.0)
        for t in range(40):
            start = starts[starts <= t].max()
            source = max(t - 3, start)               # frame t - d, but never one of an earlier episode: the first frame instead
            obs = rep[t]["obs"][0]
            assert np.array_equal(bits(obs[1:27]), bits(raw[source, 0, 1:27])), (step0, t)
            assert np.array_equal(bits(obs[[0, 27]]), bits(raw[t, 0, [0, 27]]))      # unmasked columns: untouched
            assert rep[t]["first"][0] == (t in starts)
            if t in starts:
                assert all(np.array_equal(bits(rep[t]["ring"][k, 0]), bits(raw[t, 0])) for k in range(9))


def test_every_delay_and_an_external_reset_refills_the_ring():
    spec = config(DELAY=[0, 8])
    raw = pattern(30, 9)
    table = fixed(n=9)
    table[0] = np.arange(9)
    progress = np.tile(np.arange(30)[:, None], (1, 9))
    external = [[] for _ in range(30)]
    external[14] = [2, 8]
    rep = env_sensor.sensor_replay(spec, SEED, np.arange(9), np.arange(30), raw, progress, np.zeros((30, 9)), external, 5.0, table=table)
    for t in range(30):
        for e in range(9):
            start = 14 if (e in (2, 8) and t >= 14) else 0
            assert np.array_equal(bits(rep[t]["obs"][e]), bits(raw[max(t - e, start), e])), (t, e)
        assert not rep[t]["fresh"].any()
    assert rep[14]["first"].tolist() == [e in (2, 8) for e in range(9)] and rep[0]["first"].all() and not rep[15]["first"].any()


def test_hold_never_holds_a_first_frame_and_repeats_the_previous_frame_with_its_noise():
    spec = config(HOLD=0.6, NOISE_STD=0.02, DELAY=1)
    n, steps = 16, 60
    raw = pattern(steps, n)
    progress = np.stack([episodes_of([9, 1, 1, 14, 6], steps)] * n, axis=1)
    gids = np.arange(n) + 500
    rep = env_sensor.sensor_replay(spec, SEED, gids, np.arange(steps), raw, progress, np.zeros((steps, n)), clip=5.0)
    held = np.stack([r["held"] for r in rep])
    first = np.stack([r["first"] for r in rep])
    assert not (held & first).any() and 0.45 < held[~first].mean() < 0.75 and held.any(axis=0).all()
    u = np.stack([env_sensor.hold_uniform(SEED, gids, t) for t in range(steps)])
    assert np.array_equal(held, ~first & (u < np.float32(0.6))) and u.dtype == np.float32
    for t in range(1, steps):
        cur, prev = rep[t]["ring"][t % 9], rep[t - 1]["ring"][(t - 1) % 9]
        assert np.array_equal(bits(cur[held[t]]), bits(prev[held[t]]))                  # the previous frame, noise included
        fresh_rows = ~held[t]
        assert not np.array_equal(bits(cur[fresh_rows]), bits(raw[t][fresh_rows]))      # ... and a new one carries its own
        z = env_sensor.noise_deviate(SEED, gids[fresh_rows], t, np.arange(NUM_OBS))
        c = np.float32(np.float64(np.float32(0.02)) * env_sensor.NOISE_SCALE)
        assert np.array_equal(bits(cur[fresh_rows]), bits(raw[t][fresh_rows] + z * c))
        # DELAY 1: what is delivered is the slot pushed one step ago, unless this is a first frame
        expect = np.where(first[t][:, None], cur, prev)
        assert np.array_equal(bits(rep[t]["obs"]), bits(expect))


def test_noise_stays_off_unmasked_columns_and_the_reclamp_holds():
    spec = config(NOISE_STD=0.5, COLUMNS=[2, 3, 5, 20])
    raw = pattern(20, 8) * np.float32(12.0)
    raw = np.minimum(raw, np.float32(5.0))           # as the step leaves it: clamped; many entries sit at the clip
    progress = np.tile(np.arange(20)[:, None], (1, 8))
    rep = env_sensor.sensor_replay(spec, SEED, np.arange(8), np.arange(20), raw, progress, np.zeros((20, 8)), clip=5.0)
    obs = np.stack([r["obs"] for r in rep])
    rest = np.setdiff1d(np.arange(NUM_OBS), [2, 3, 5, 20])
    assert np.array_equal(bits(obs[:, :, rest]), bits(raw[:, :, rest]))
    masked = obs[:, :, [2, 3, 5, 20]]
    assert masked.max() == np.float32(5.0) and np.abs(masked).max() <= np.float32(5.0)
    assert np.count_nonzero(masked != raw[:, :, [2, 3, 5, 20]]) > 0.9 * masked.size - np.count_nonzero(masked == 5.0)
    loose = env_sensor.sensor_replay(spec, SEED, np.arange(8), np.arange(20), raw, progress, np.zeros((20, 8)))      # clip inf
    assert np.stack([r["obs"] for r in loose]).max() > 5.0


def test_per_episode_redraws_at_the_flag_and_leaves_unflagged_envs_alone():
    spec = config(DELAY=[0, 8], HOLD=[0.0, 0.5], NOISE_STD={"values": [0.0, 0.01]}, PER_EPISODE=True)
    n, steps = 6, 25
    gids = np.arange(n) + 1000
    raw = pattern(steps, n)
    resets = np.zeros((steps, n), dtype=np.int64)
    resets[4, 1] = resets[9, 1] = resets[9, 3] = resets[24, 5] = 1
    progress = np.tile(np.arange(steps)[:, None], (1, n)) + 1
    progress[5, 1] = progress[10, 1] = progress[10, 3] = 0               # the step that consumes a flag leaves progress 0
    rep = env_sensor.sensor_replay(spec, SEED, gids, np.arange(steps), raw, progress, resets, clip=5.0)
    table0 = env_sensor.draw_sensor(spec, SEED, gids, 0).astype(np.float32)
    episode = np.zeros(n, dtype=np.int64)
    for t in range(steps):
        episode += resets[t]
        assert np.array_equal(rep[t]["episode_index"], episode)
        expect = env_sensor.draw_sensor(spec, SEED, gids, episode).astype(np.float32)
        assert np.array_equal(bits(rep[t]["table"]), bits(expect))
    for e in (0, 2, 4):
        assert all(np.array_equal(bits(r["table"][:, e]), bits(table0[:, e])) for r in rep)
    held = env_sensor.sensor_replay(dict(spec, PER_EPISODE=False), SEED, gids, np.arange(steps), raw, progress, resets, clip=5.0)
    assert all(np.array_equal(bits(r["table"]), bits(table0)) and not r["episode_index"].any() for r in held)
    # the frame behind the flagged step is still handled with the old values: the new ones act from the next first frame
    assert np.array_equal(bits(rep[4]["obs"]), bits(held[4]["obs"]))


def test_the_deviate_has_zero_mean_unit_variance_and_bounded_support():
    """65536 draws: the standard error of the mean is 1 / 256 and of the variance sqrt(1.85 / 65536) ~ 0.0053 (an
    eight-uniform sum has kurtosis 2.85); the bounds are five standard errors.  The support ends just inside sqrt(8 * 3) = 4.899."""
    z = env_sensor.noise_deviate(SEED, np.arange(2048) + 77, 31, np.arange(32)).astype(np.float64) * env_sensor.NOISE_SCALE
    assert z.size == 65536
    print("deviate: mean %.5f variance %.5f max |z| %.4f" % (z.mean(), z.var(), np.abs(z).max()))
    assert abs(z.mean()) < 0.02 and abs(z.var() - 1.0) < 0.03 and np.abs(z).max() <= 4.9
    assert 4.898 < 524280 * env_sensor.NOISE_SCALE < 4.9             # the support's end: 8 * 65535 halves, just inside sqrt(24)
    raw = env_sensor.noise_deviate(SEED, [5], 2 ** 32 + 3, [0, 1])
    assert raw.dtype == np.float32 and np.all(raw == np.round(raw)) and np.all(np.abs(raw) <= 524280) and np.all(raw % 2 == 0)
    assert not np.array_equal(raw, env_sensor.noise_deviate(SEED, [5], 3, [0, 1]))      # the high word of the step is keyed


# ------------------------------------------------------------------------------------------------- the episode log's join
def rows_of(env, end_step, **more):
    rows = {name: np.zeros(len(env)) for name in episodes.COLUMNS}
    rows.update(env=np.asarray(env, dtype=np.int64), end_step=np.asarray(end_step, dtype=np.int64), **more)
    return rows


def test_log_join_for_held_and_per_episode_values_with_a_dropped_row():
    offset = 1000
    held = config(DELAY={"values": [0, 2, 4]}, HOLD=0.1)
    rows = rows_of([0, 1, 2, 4, 1], [5, 6, 7, 8, 9])
    params = lambda spec: (lambda envs, eps: env_sensor.episode_params(spec, SEED, np.asarray(envs) + offset, eps))      # noqa: E731
    out = episodes.with_sensor_params(rows, params(held))
    assert [k for k in out if k.startswith("param_")] == ["param_SENSOR_DELAY"]       # only the names that vary
    assert np.array_equal(out["param_SENSOR_DELAY"], np.asarray([0, 2, 4], dtype=np.float32)[(np.asarray([0, 1, 2, 4, 1]) + offset) % 3])
    # per episode: env 1 finished episodes 0, 1, 2 but the ring dropped its first row; ordinals count back from the counters
    spec = config(DELAY=[0, 8], NOISE_STD=[0.0, 0.02], PER_EPISODE=True)
    env, end = np.asarray([1, 0, 1, 2]), np.asarray([20, 21, 30, 31])
    counters = np.asarray([1, 3, 1, 0])
    rows = rows_of(env, end, episode=episodes.episode_ordinals(env, end, counters))
    assert rows["episode"].tolist() == [1, 0, 2, 0]
    out = episodes.with_sensor_params(rows, params(spec))
    expect = env_sensor.draw_sensor(spec, SEED, env + offset, [1, 0, 2, 0]).astype(np.float32)
    assert sorted(k for k in out if k.startswith("param_")) == ["param_SENSOR_DELAY", "param_SENSOR_NOISE_STD"]
    assert np.array_equal(bits(out["param_SENSOR_DELAY"]), bits(expect[0])) and np.array_equal(bits(out["param_SENSOR_NOISE_STD"]), bits(expect[2]))
    assert len(episodes.with_sensor_params(rows_of([], []), params(spec))) == len(rows_of([], []))
    values, rate, count = episodes.value_rate(dict(out, reached_ever=np.asarray([1, 0, 1, 1])), "param_SENSOR_DELAY")
    assert count.sum() == 4 and len(values) == len(np.unique(expect[0]))


def test_file_round_trip(tmp_path):
    spec = config(DELAY=[0, 8], HOLD={"values": [0.0, 0.3]}, PER_EPISODE=True, COLUMNS=[1, 2])
    env, end = np.asarray([3, 0, 3, 69]), np.asarray([4, 9, 11, 12])
    rows = rows_of(env, end, episode=np.asarray([0, 0, 1, 0]))
    path = str(tmp_path / "episodes.npz")
    episodes.save(path, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {}, sensor={"spec": spec, "seed": SEED, "env_id_offset": 35})
    loaded_spec, episode, sensor_params = episodes.load_env_sensor(path)
    assert loaded_spec == spec and episode.tolist() == [0, 0, 1, 0]
    back = episodes.load_rows_with_params(path)
    expect = env_sensor.episode_params(spec, SEED, env + 35, [0, 0, 1, 0])
    assert sorted(expect) == ["SENSOR_DELAY", "SENSOR_HOLD"]
    for name, v in expect.items():
        assert np.array_equal(bits(back["param_" + name]), bits(v)) and np.array_equal(bits(sensor_params(env, [0, 0, 1, 0])[name]), bits(v))
    assert back["episode"].tolist() == [0, 0, 1, 0] and np.array_equal(back["env"], env)
    plain = str(tmp_path / "plain.npz")
    episodes.save(plain, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {})
    assert episodes.load_env_sensor(plain) == (None, None, None)
    assert not any(k.startswith("param_") for k in episodes.load_rows_with_params(plain))


# ----------------------------------------------------------------------------------------------------------- contraction
def test_the_device_code_holds_no_contracted_multiply_add_of_the_noise_term(tmp_path):
    """`obs + z * c` must stay a multiply and an add.  Compiled for the device with native.py's flags, the only float32
    fused multiply-adds in the unit's assembly are those of the 64-bit integer divisions the compiler expands (they carry
    the literals +-2^32, 0x4f800000 / 0xcf800000); the same compile under plain `fast` ignores the pragma and shows the
    noise term fused, one per column of a row vector, so the check can fail."""
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def fused(name, extra):
        out = str(tmp_path / name)
        subprocess.check_call([hipcc] + native._flags(native.SRC_SENSOR) + extra + ["--cuda-device-only", "-S", "-o", out, native.SRC_SENSOR],
                              stderr=subprocess.DEVNULL)
        text = open(out).read()
        assert text.count("vine_env_sensor_kernel") >= 4
        lines = [ln.strip() for ln in text.splitlines() if re.search(r"\bv_(pk_)?(fma|fmac|fmaak|fmamk|mad|mac|madak|madmk)_(legacy_)?f32", ln)]
        return [ln for ln in lines if "0x4f800000" not in ln and "0xcf800000" not in ln], text
    contracted, text = fused("sensor.s", [])
    assert contracted == [], contracted[:3]
    assert len(re.findall(r"\bv_mul_f32", text)) >= 4 and len(re.findall(r"\bv_add_f32", text)) >= 4
    contracted, _ = fused("sensor_fast.s", ["-ffp-contract=fast"])      # (the later flag wins: the pragma is ignored again)
    assert len(contracted) >= 4, contracted
