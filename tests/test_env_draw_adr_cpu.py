"""ENV_DRAW_ADR without a GPU: include/vine_env_draw_adr.h against its ctypes mirror, the two keys against the host hash, the
build plumbing of the eighteenth unit, every refusal of its host entry point (through the library and through the stand-alone
sanitizer build of scripts/env_draw_adr_host_check.cpp) and of the configuration, utils/env_draw_adr.py draw_adr_replay (its
reduction to the three observers' draws, widening and narrowing on hand-made flags, the range formula), the episode log's
join of a row to the range in force, and the file and checkpoint round trips.  Every comparison is bit for bit or on integers."""
import ctypes as C
import hashlib
import inspect
import logging
import os
import re
import subprocess

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, load_config, native
from vine_robot_isaacgymenvs_amd.utils import env_draw_adr, env_params, env_push, env_sensor, env_target, episodes, named_draw
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENSOR = {"DELAY": [0, 3], "HOLD": [0.0, 0.2], "NOISE_STD": [0.0, 0.01], "PER_EPISODE": True}
PUSH = {"RATE": 0.2, "IMPULSE": [0.0, 0.01], "PER_EPISODE": True}
TARGET = {"VEL_ALONG": [-0.3, 0.3], "SPAN_ALONG": [0.03, 0.04], "PER_EPISODE": True}
NAMES = {"SENSOR_DELAY": {"START": [1, 1], "STEP": 1}, "PUSH_IMPULSE": {"START": [0.002, 0.004], "STEP": 0.004},
         "TARGET_VEL_ALONG": {"START": [0.0, 0.0], "STEP": 0.05}}
SLOT = env_draw_adr.NAMES.index
CDT = np.float32(1.0 / 30.0)
MODULES = (env_sensor, env_push, env_target)


def env_cfg(names=NAMES, sensor=SENSOR, push=PUSH, target=TARGET, **keys):
    return {"ENV_SENSOR": sensor, "ENV_PUSH": push, "ENV_TARGET": target, "ENV_DRAW_ADR": dict({"NAMES": names}, **keys)}


def observer_cfgs(env):
    return (env_sensor.sensor_config(env, 28), env_push.push_config(env), env_target.target_config(env, CDT))


def adr_of(names=NAMES, multi_gpu=False, **keys):
    env = env_cfg(names, **{k: keys.pop(k) for k in ("sensor", "push", "target") if k in keys}, **keys)
    return env_draw_adr.draw_adr_config(env, *observer_cfgs(env), multi_gpu=multi_gpu)


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.load()


@pytest.fixture()
def vcfg(lib):
    c = abi.VineConfig()
    assert lib.vine_config_default(C.byref(c)) == 0
    c.seed = 42
    return c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tables_at_start(adr, cfgs, seed, gids):
    """The three observers' tables of episode 0 with the START rows in them: what ``EnvDrawAdr`` leaves at construction."""
    tables = [named_draw.draw(named_draw.named(m.NAMES, m.DRAW_NAMES, c), seed, gids, 0, env_draw_adr.INTEGER).astype(np.float32)
              for m, c in zip(MODULES, cfgs)]
    for name, row in env_draw_adr.start_rows(adr, seed, gids).items():
        g, r, _ = env_draw_adr.place_of(name)
        tables[g][r] = row
    return tables


def observer_specs(lib, vcfg, cfgs):
    return (env_sensor.sensor_spec(lib, vcfg, cfgs[0]), env_push.push_spec(lib, vcfg, cfgs[1]), env_target.target_spec(lib, vcfg, cfgs[2]))


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_equals_the_mirror_the_keys_and_the_build_plumbing(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vine_env_draw_adr.h")).read(), flags=re.S)
    for macro, value in (("ABI_VERSION", abi.ENV_DRAW_ADR_ABI_VERSION), ("THREADS", abi.ENV_DRAW_ADR_THREADS),
                         ("HISTORY_WORDS", abi.ENV_DRAW_ADR_HISTORY_WORDS), ("KEY_PROBE", abi.ENV_DRAW_ADR_KEY_PROBE),
                         ("KEY_WHICH", abi.ENV_DRAW_ADR_KEY_WHICH)):
        assert int(re.search(r"#define VINE_ENV_DRAW_ADR_%s (\w+?)(ull)?\s" % macro, text).group(1), 0) == value, macro
    for word, key in (("DRAW_ADR_PROBE", abi.ENV_DRAW_ADR_KEY_PROBE), ("DRAW_ADR_WHICH", abi.ENV_DRAW_ADR_KEY_WHICH)):
        assert key == named_draw.name_key(word) == int.from_bytes(hashlib.sha256(word.encode()).digest()[:8], "little")
    assert len({abi.ENV_DRAW_ADR_KEY_PROBE, abi.ENV_DRAW_ADR_KEY_WHICH, abi.ENV_ADR_KEY_PROBE, abi.ENV_ADR_KEY_WHICH}) == 4
    for struct, mirror in (("VineEnvDrawAdrSlot", abi.VineEnvDrawAdrSlot), ("VineEnvDrawAdrSpec", abi.VineEnvDrawAdrSpec)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        fields = [f for decl in body.split(";") if decl.strip()
                  for f in re.sub(r"\[.*?\]", "", decl.strip().split(None, 1)[-1]).replace(" ", "").split(",")]
        assert fields == [f[0] for f in mirror._fields_], struct
    assert C.sizeof(abi.VineEnvDrawAdrSlot) == 104
    assert lib.vine_env_draw_adr_spec_size() == C.sizeof(abi.VineEnvDrawAdrSpec) == 1024
    slots = re.search(r"typedef enum VineEnvDrawAdrSlotIndex \{(.*?)\}", text, flags=re.S).group(1)
    assert [w.split("=")[0].strip()[4:] for w in slots.split(",")][:-1] == list(env_draw_adr.NAMES) and abi.VDA_NAMES == 9
    assert env_draw_adr.NAMES == env_sensor.DRAW_NAMES + env_push.DRAW_NAMES + env_target.DRAW_NAMES
    assert [env_draw_adr.place_of(n)[:2] for n in env_draw_adr.NAMES] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3)]
    functions = sorted(set(re.findall(r"\b(vine_env_draw_adr[a-z_0-9]*)\s*\(", text)))
    assert functions == sorted(abi.ENV_DRAW_ADR_PROTOTYPES) and len(functions) == 3
    for name in functions:
        assert hasattr(lib, name), name
    for name, count in (("vine_env_draw_adr_spec", 11), ("vine_env_draw_adr_scheduled", 13)):
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert len(decl.split(",")) == len(abi.ENV_DRAW_ADR_PROTOTYPES[name][1]) == count, name
    assert "declare_env_draw_adr" in inspect.getsource(abi.declare_all)
    # nothing of it went into the three observers' own headers, whose functions existing tests count
    for header in ("vine_env_sensor.h", "vine_env_push.h", "vine_env_target.h", "vine_env_adr.h"):
        assert "draw_adr" not in open(os.path.join(REPO, "include", header)).read(), header
    # the eighteenth translation unit: compiled by the loop's body behind the loop, side by side with the others
    build = inspect.getsource(native.build)
    assert native.LATER_UNITS == (native.SRC_DRAW_ADR,) and "map(compile_unit, LATER_UNITS)" in build
    assert build.index("map(compile_unit, LATER_UNITS)") < build.index("proc.wait()")
    assert os.path.basename(native.SRC_DRAW_ADR) == "vine_env_draw_adr.hip" and os.path.exists(native.SRC_DRAW_ADR)
    assert native.SRC_DRAW_ADR in native.DEPS
    for header in ("vine_env_draw_adr.h", "vine_adr_shared.h"):
        assert any(d.endswith(header) for d in native.DEPS), header
    headers = {os.path.basename(h) for h in native._SOURCE_HEADERS[native.SRC_DRAW_ADR]}
    assert {"vine_env_draw_adr.h", "vine_env_adr.h", "vine_env_sensor.h", "vine_env_push.h", "vine_env_target.h", "vine_env_redraw.h",
            "vine_named_draw.h", "vine_adr_shared.h"} <= headers
    assert "vine_adr_shared.h" in {os.path.basename(h) for h in native._SOURCE_HEADERS[native.SRC_ADR]}
    assert native._SOURCE_FLAGS[native.SRC_DRAW_ADR] == ["-ffp-contract=fast-honor-pragmas"]
    flags = native._flags(native.SRC_DRAW_ADR)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast") and "-ffp-contract=off" not in flags
    assert [s for s, f in native._SOURCE_FLAGS.items() if "-ffp-contract=off" in f] == [native.SRC_REDRAW]
    source = open(native.SRC_DRAW_ADR).read()
    assert source.index("#pragma clang fp contract(off)") < source.index("#include")
    # the decide rule and the boundary are stated once, and both units include the statement
    shared = open(os.path.join(os.path.dirname(native.SRC_ADR), "vine_adr_shared.h")).read()
    assert "adr_decide_lane" in shared and "adr_bound_lo" in shared and "__ballot" in shared
    for unit in (native.SRC_ADR, native.SRC_DRAW_ADR):
        unit_text = open(unit).read()
        assert '#include "vine_adr_shared.h"' in unit_text and "adr_decide_lane(" in unit_text and "adr_bound_lo(" in unit_text
        assert "__ballot" not in unit_text and "narrow_at * (double)n" not in unit_text, unit
    # the step kernels, the PPO kernels and the three observers' units know nothing of it
    for other in (native.SRC, native.SRC_PPO, native.SRC_SENSOR, native.SRC_PUSH, native.SRC_TARGET):
        assert "draw_adr" not in open(other).read().lower(), other


# ------------------------------------------------------------------------------------------------------------ the spec
def call(lib, vcfg, names=None, specs=None, fraction=0.25, queue=4, widen_at=0.8, narrow_at=0.4, capacity=16, cfg=True, out=True,
         pass_names=True):
    specs = observer_specs(lib, vcfg, observer_cfgs(env_cfg())) if specs is None else specs
    names = env_draw_adr.draw_adr_names({"NAMES": NAMES}) if names is None else names
    a = abi.VineEnvDrawAdrSpec()
    rc = lib.vine_env_draw_adr_spec(C.byref(vcfg) if cfg else None, *[C.byref(s) if s is not None else None for s in specs],
                                    names if pass_names else None, fraction, queue, widen_at, narrow_at, capacity, C.byref(a) if out else None)
    return rc, lib.vine_last_error().decode(), a


def names_with(**entries):
    """The C names with ``NAME=(lo, hi, step)`` entries on, on top of nothing."""
    return env_draw_adr.draw_adr_names({"NAMES": {n: {"START": [v[0], v[1]], "STEP": v[2]} for n, v in entries.items()}})


def test_the_spec_and_every_refusal_by_name(lib, vcfg):
    rc, _, a = call(lib, vcfg)
    assert rc == abi.OK and a.checked == 1 and a.num_adr == 3 and a.queue == 4 and a.history_capacity == 16 and a.seed == 42
    assert (a.boundary_fraction, a.widen_at, a.narrow_at) == (0.25, 0.8, 0.4)
    assert list(a.adr_slot)[:3] == [SLOT("SENSOR_DELAY"), SLOT("PUSH_IMPULSE"), SLOT("TARGET_VEL_ALONG")] and set(list(a.adr_slot)[3:]) == {-1}
    adr = adr_of()
    want = env_draw_adr.draw_adr_max_widen(adr)
    assert np.array_equal(np.array([list(s.max_widen) for s in a.slot]), want) and want[SLOT("TARGET_VEL_ALONG")].tolist() == [6, 6]
    for s, name in enumerate(env_draw_adr.NAMES):
        g, r, own = env_draw_adr.place_of(name)
        sl = a.slot[s]
        assert (sl.group, sl.row, sl.integer, sl.adr.on) == (g, r, int(name == "SENSOR_DELAY"), int(name in NAMES)), name
        assert sl.limits.key == named_draw.name_key(name), name
    assert (a.slot[SLOT("TARGET_VEL_ALONG")].limits.lo, a.slot[SLOT("TARGET_VEL_ALONG")].limits.hi) == (-0.3, 0.3)
    assert env_draw_adr.draw_adr_spec(lib, vcfg, adr, *observer_specs(lib, vcfg, observer_cfgs(env_cfg()))).num_adr == 3

    specs = observer_specs(lib, vcfg, observer_cfgs(env_cfg()))
    null = "null argument to vine_env_draw_adr_spec"
    assert call(lib, vcfg, cfg=False)[:2] == (abi.ERR_INVALID_ARG, null)
    assert call(lib, vcfg, out=False)[:2] == (abi.ERR_INVALID_ARG, null)
    assert call(lib, vcfg, pass_names=False)[:2] == (abi.ERR_INVALID_ARG, null)

    def altered(k, **fields):
        out = [type(s).from_buffer_copy(s) for s in specs]
        for f, v in fields.items():
            setattr(out[k], f, v)
        return out

    bad_cfg = abi.VineConfig.from_buffer_copy(vcfg)
    bad_cfg.abi_version = 99
    assert "VineConfig.abi_version mismatch" in call(lib, bad_cfg)[1]
    for k, struct, maker in ((0, "VineEnvSensorSpec", "vine_env_sensor_spec"), (1, "VineEnvPushSpec", "vine_env_push_spec"),
                             (2, "VineEnvTargetSpec", "vine_env_target_spec")):
        rc, msg, a = call(lib, vcfg, specs=altered(k, abi_version=9))
        assert rc == abi.ERR_INVALID_ARG and msg == struct + ".abi_version mismatch" and a.checked == 0
        rc, msg, _ = call(lib, vcfg, specs=altered(k, checked=0))
        assert rc == abi.ERR_INVALID_ARG and msg == "env draw adr spec: the %s was not filled by %s" % (struct, maker)
        rc, msg, _ = call(lib, vcfg, specs=altered(k, seed=43))
        assert rc == abi.ERR_INVALID_ARG and "seed is not the configuration's" in msg
        name = ("SENSOR_DELAY", "PUSH_IMPULSE", "TARGET_VEL_ALONG")[k]
        rc, msg, _ = call(lib, vcfg, specs=[None if j == k else s for j, s in enumerate(specs)])
        assert rc == abi.ERR_INVALID_ARG and msg == "env draw adr spec: %s: a name under ADR needs its observer's spec: the observer is off" % name
        rc, msg, _ = call(lib, vcfg, specs=altered(k, per_episode=0))
        assert rc == abi.ERR_INVALID_ARG and msg.startswith("env draw adr spec: %s: a name under ADR needs PER_EPISODE of its observer" % name)
    for names, text in (
            (names_with(PUSH_RATE=(0.2, 0.2, 0.1)), "PUSH_RATE: a name under ADR must be a [lo, hi] range of its observer"),
            (names_with(PUSH_IMPULSE=(np.nan, 0.004, 0.004)), "PUSH_IMPULSE: START needs finite lo <= hi"),
            (names_with(PUSH_IMPULSE=(0.0, np.inf, 0.004)), "PUSH_IMPULSE: START needs finite lo <= hi"),
            (names_with(PUSH_IMPULSE=(0.004, 0.002, 0.004)), "PUSH_IMPULSE: START needs finite lo <= hi"),
            (names_with(PUSH_IMPULSE=(-0.001, 0.002, 0.004)), "PUSH_IMPULSE: START lies outside the limits"),
            (names_with(TARGET_VEL_ALONG=(0.0, 0.31, 0.05)), "TARGET_VEL_ALONG: START lies outside the limits"),
            (names_with(SENSOR_NOISE_STD=(0.0, 0.0, 0.0)), "SENSOR_NOISE_STD: STEP must be positive"),
            (names_with(SENSOR_NOISE_STD=(0.0, 0.0, -0.1)), "SENSOR_NOISE_STD: STEP must be positive"),
            (names_with(SENSOR_NOISE_STD=(0.0, 0.0, np.nan)), "SENSOR_NOISE_STD: STEP must be positive"),
            (names_with(SENSOR_NOISE_STD=(0.0, 0.0, np.inf)), "SENSOR_NOISE_STD: STEP must be positive"),
            (names_with(SENSOR_DELAY=(0.5, 1.0, 1.0)), "SENSOR_DELAY: an integer parameter takes an integer START and STEP"),
            (names_with(SENSOR_DELAY=(1.0, 1.0, 0.5)), "SENSOR_DELAY: an integer parameter takes an integer START and STEP"),
            (names_with(TARGET_VEL_ALONG=(0.0, 0.0, 1e-11)), "TARGET_VEL_ALONG: more than 2^30 STEPs between START and a limit"),
            (names_with(), "no name is under ADR")):
        rc, msg, a = call(lib, vcfg, names=names)
        assert rc == abi.ERR_INVALID_ARG and msg.startswith("env draw adr spec: " + text) and a.checked == 0, text
    off = names_with(**{n: (v["START"][0], v["START"][1], v["STEP"]) for n, v in NAMES.items()})
    off[SLOT("SENSOR_HOLD")].step = 0.1
    assert "SENSOR_HOLD: START and STEP of a name that is not under ADR must be 0" in call(lib, vcfg, names=off)[1]
    off[SLOT("SENSOR_HOLD")].step, off[SLOT("TARGET_SPAN_ACROSS")].start_hi = 0.0, 1.0
    assert "TARGET_SPAN_ACROSS: START and STEP of a name that is not under ADR must be 0" in call(lib, vcfg, names=off)[1]
    off[SLOT("TARGET_SPAN_ACROSS")].start_hi, off[SLOT("PUSH_RATE")].reserved = 0.0, 1
    assert "PUSH_RATE: reserved must be 0" in call(lib, vcfg, names=off)[1]
    values = observer_cfgs(env_cfg(sensor=dict(SENSOR, HOLD={"values": [0.0, 0.1]})))
    vspecs = (env_sensor.sensor_spec(lib, vcfg, values[0], 0x1000),) + tuple(specs[1:])
    assert "SENSOR_HOLD: a name under ADR must be a [lo, hi] range" in call(lib, vcfg, names=names_with(SENSOR_HOLD=(0.0, 0.1, 0.1)), specs=vspecs)[1]
    for keys, text in ((dict(fraction=1.0), "BOUNDARY_FRACTION must lie in [0, 1)"), (dict(fraction=-0.1), "BOUNDARY_FRACTION must lie in [0, 1)"),
                       (dict(fraction=np.nan), "BOUNDARY_FRACTION must lie in [0, 1)"), (dict(queue=0), "QUEUE must be at least 1"),
                       (dict(widen_at=0.4), "NARROW_AT must be below WIDEN_AT"), (dict(widen_at=np.nan), "NARROW_AT must be below WIDEN_AT"),
                       (dict(narrow_at=-np.inf), "NARROW_AT must be below WIDEN_AT"), (dict(capacity=0), "the history capacity must be at least 1")):
        rc, msg, a = call(lib, vcfg, **keys)
        assert rc == abi.ERR_INVALID_ARG and msg == "env draw adr spec: " + text and a.checked == 0, keys
    with pytest.raises(ValueError, match="ENV_DRAW_ADR: env draw adr spec: QUEUE must be at least 1"):
        env_draw_adr.draw_adr_spec(lib, vcfg, dict(adr, QUEUE=0), *specs)
    # the launch refuses before it asks for a handle's tables: null pointers, a spec nobody checked, another ABI
    rc, _, a = call(lib, vcfg)
    tables = (C.c_void_p * 3)(8, 8, 8)
    args = [8, C.byref(a), 8, tables, None] + [8] * 7 + [None]
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11):
        bad = list(args)
        bad[k] = None
        assert lib.vine_env_draw_adr_scheduled(*bad) == abi.ERR_INVALID_ARG and b"null argument to vine_env_draw_adr_scheduled" in lib.vine_last_error(), k
    for g, word in enumerate((b"SENSOR_DELAY is under ADR and needs the table of ENV_SENSOR", b"PUSH_IMPULSE is under ADR and needs the table of ENV_PUSH",
                              b"TARGET_VEL_ALONG is under ADR and needs the table of ENV_TARGET")):
        bad = list(args)
        bad[3] = (C.c_void_p * 3)(*[None if j == g else 8 for j in range(3)])
        assert lib.vine_env_draw_adr_scheduled(*bad) == abi.ERR_INVALID_ARG and word in lib.vine_last_error()
    for change, text in ((dict(checked=0), b"not filled by vine_env_draw_adr_spec"), (dict(abi_version=7), b"VineEnvDrawAdrSpec.abi_version mismatch"),
                         (dict(num_adr=4), b"lies outside what vine_env_draw_adr_spec fills")):
        spec = abi.VineEnvDrawAdrSpec.from_buffer_copy(a)
        for k, v in change.items():
            setattr(spec, k, v)
        bad = list(args)
        bad[1] = C.byref(spec)
        assert lib.vine_env_draw_adr_scheduled(*bad) == abi.ERR_INVALID_ARG and text in lib.vine_last_error(), change


def test_the_refusals_through_the_stand_alone_host_check(tmp_path):
    """scripts/env_draw_adr_host_check.cpp, built as its head says -- the unit's HOST code under AddressSanitizer and UBSan, with
    a stand-in handle -- walks every refusal of the spec by name and those of the launch, the ones that need a handle
    included.  A few seconds of hipcc.  Nothing is loaded into Python under a sanitizer."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "env_draw_adr_host_check")
    source = os.path.join(REPO, "scripts", "env_draw_adr_host_check.cpp")
    text = open(source).read()
    for word in ("null argument to vine_env_draw_adr_spec", "VineConfig.abi_version mismatch", "VineEnvSensorSpec.abi_version mismatch",
                 "VineEnvPushSpec.abi_version mismatch", "VineEnvTargetSpec.abi_version mismatch", "was not filled by vine_env_sensor_spec",
                 "was not filled by vine_env_push_spec", "was not filled by vine_env_target_spec", "a name under ADR needs its observer's spec",
                 "a name under ADR needs PER_EPISODE", "a name under ADR must be a [lo, hi] range", "START needs finite lo <= hi",
                 "START lies outside the limits", "STEP must be positive", "an integer parameter takes an integer START and STEP",
                 "START and STEP of a name that is not under ADR must be 0", "no name is under ADR", "BOUNDARY_FRACTION must lie in [0, 1)",
                 "QUEUE must be at least 1", "NARROW_AT must be below WIDEN_AT", "the history capacity must be at least 1", "more than 2^30 STEPs",
                 "null argument to vine_env_draw_adr_scheduled", "was not filled by vine_env_draw_adr_spec", "VineEnvDrawAdrSpec.abi_version mismatch",
                 "needs a reward matrix bound to the handle", "needs the table of ENV_SENSOR"):
        assert word in text, word
    subprocess.check_call([hipcc, "--offload-arch=" + native.ARCH, "-O1", "-g", "-std=c++17", "-ffp-contract=fast-honor-pragmas",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-x", "hip",
                           source, native.SRC_DRAW_ADR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "env draw adr host check ok" in out.stdout, out.stdout + out.stderr


# --------------------------------------------------------------------------------------------------- the configuration
def test_defaults_and_every_config_error(caplog):
    env = load_config(overrides=[])["task"]["env"]
    assert env["ENV_DRAW_ADR"] == {} and env_draw_adr.draw_adr_config(env, None, None, None) is None
    adr = adr_of()
    assert list(adr["NAMES"]) == ["SENSOR_DELAY", "PUSH_IMPULSE", "TARGET_VEL_ALONG"] and adr["LIMITS"]["TARGET_VEL_ALONG"] == [-0.3, 0.3]
    assert {k: adr[k] for k in env_draw_adr.DEFAULTS} == env_params.ADR_DEFAULTS and adr["NAMES"]["SENSOR_DELAY"] == {"START": [1.0, 1.0], "STEP": 1.0}
    K = r"task\.env\.ENV_DRAW_ADR"
    one = lambda name, lo, hi, step: {name: {"START": [lo, hi], "STEP": step}}      # noqa: E731
    for keys, text in (
            (dict(multi_gpu=True), K + " with multi_gpu=True"),
            (dict(names={}), K + r"\.NAMES must map at least one draw name"),
            (dict(names=one("DAMPING", 0, 0, 1)), K + r"\.NAMES\.DAMPING: unknown draw name"),
            (dict(SPEED=3), K + r": unknown key\(s\) SPEED"),
            (dict(sensor={}), K + r"\.NAMES\.SENSOR_DELAY needs task\.env\.ENV_SENSOR"),
            (dict(push={}), K + r"\.NAMES\.PUSH_IMPULSE needs task\.env\.ENV_PUSH"),
            (dict(target={}), K + r"\.NAMES\.TARGET_VEL_ALONG needs task\.env\.ENV_TARGET"),
            (dict(target=dict(TARGET, PER_EPISODE=False)), K + r"\.NAMES\.TARGET_VEL_ALONG needs task\.env\.ENV_TARGET\.PER_EPISODE"),
            (dict(names=one("PUSH_RATE", 0.2, 0.2, 0.1)), K + r"\.NAMES\.PUSH_RATE: the name must be a \[lo, hi\] range in task\.env\.ENV_PUSH\.RATE"),
            (dict(names=one("SENSOR_HOLD", 0.0, 0.1, 0.1), sensor=dict(SENSOR, HOLD={"values": [0.0, 0.1]})),
             K + r"\.NAMES\.SENSOR_HOLD: the name must be a \[lo, hi\] range"),
            (dict(names={"PUSH_IMPULSE": {"START": [0, 0]}}), K + r"\.NAMES\.PUSH_IMPULSE must hold START and STEP"),
            (dict(names={"PUSH_IMPULSE": {"START": 0.0, "STEP": 0.1}}), K + r"\.NAMES\.PUSH_IMPULSE\.START is \[lo, hi\]"),
            (dict(names=one("PUSH_IMPULSE", "a", 0.0, 0.1)), K + r"\.NAMES\.PUSH_IMPULSE\.START: 'a' is not a number"),
            (dict(names=one("PUSH_IMPULSE", 0.004, 0.002, 0.1)), K + r"\.NAMES\.PUSH_IMPULSE\.START: lo > hi"),
            (dict(names=one("PUSH_IMPULSE", float("nan"), 0.002, 0.1)), K + r"\.NAMES\.PUSH_IMPULSE\.START: lo > hi"),
            (dict(names=one("PUSH_IMPULSE", 0.0, 0.02, 0.1)), K + r"\.NAMES\.PUSH_IMPULSE\.START \[0, 0\.02\] lies outside the limits \[0, 0\.01\]"),
            (dict(names=one("PUSH_IMPULSE", 0.0, 0.0, 0.0)), K + r"\.NAMES\.PUSH_IMPULSE\.STEP must be positive"),
            (dict(names=one("PUSH_IMPULSE", 0.0, 0.0, float("inf"))), K + r"\.NAMES\.PUSH_IMPULSE\.STEP must be positive"),
            (dict(names=one("SENSOR_DELAY", 1, 1, 0.5)), K + r"\.NAMES\.SENSOR_DELAY: an integer parameter takes an integer START and STEP"),
            (dict(names=one("SENSOR_DELAY", 0.5, 1, 1)), K + r"\.NAMES\.SENSOR_DELAY: an integer parameter takes an integer START and STEP"),
            (dict(names=one("TARGET_VEL_ALONG", 0.0, 0.0, 1e-11)), K + r"\.NAMES\.TARGET_VEL_ALONG: more than 2\^30 STEPs"),
            (dict(BOUNDARY_FRACTION=1.0), K + r"\.BOUNDARY_FRACTION must lie in \[0, 1\)"),
            (dict(BOUNDARY_FRACTION=-0.5), K + r"\.BOUNDARY_FRACTION must lie in \[0, 1\)"),
            (dict(QUEUE=0), K + r"\.QUEUE must be an integer >= 1"), (dict(QUEUE=2.5), K + r"\.QUEUE must be an integer >= 1"),
            (dict(HISTORY_CAPACITY=0), K + r"\.HISTORY_CAPACITY must be an integer >= 1"),
            (dict(WIDEN_AT=0.4, NARROW_AT=0.4), K + r"\.NARROW_AT \(0\.4\) must be below WIDEN_AT"),
            (dict(WIDEN_AT=float("nan")), K + r"\.NARROW_AT \(0\.4\) must be below WIDEN_AT"),
            (dict(QUEUE="many"), K + r"\.QUEUE: 'many' is not a number")):
        with pytest.raises(ConfigError, match=text):
            adr_of(**keys)
    with pytest.raises(ConfigError, match=K + " must be a mapping"):
        env_draw_adr.draw_adr_config({"ENV_DRAW_ADR": 3}, None, None, None)
    # forced off where a configuration is derived for something that is not training
    from vine_robot_isaacgymenvs_amd.utils import mpc, sysid
    assert ("env", "ENV_DRAW_ADR", {}) in sysid.FORCED and ("env", "ENV_DRAW_ADR", {}) in mpc.FORCED
    from vine_robot_isaacgymenvs_amd import load_task_config
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=4"])
    cfg["env"].update(env_cfg())
    with caplog.at_level(logging.INFO):
        out = mpc.model_config(cfg, 4, 16)
    assert out["env"]["ENV_DRAW_ADR"] == {} and cfg["env"]["ENV_DRAW_ADR"] != {}
    assert any("ENV_DRAW_ADR forced from" in r.getMessage() for r in caplog.records)
    source = inspect.getsource(mpc)
    assert "plant env.ENV_DRAW_ADR is forced off" in source
    from vine_robot_isaacgymenvs_amd import train
    assert "task.env.ENV_DRAW_ADR is forced off" in inspect.getsource(train.launch)


def test_train_entry_forces_the_key_off_under_test_and_refuses_multi_gpu(monkeypatch, caplog):
    from vine_robot_isaacgymenvs_amd import train
    seen = {}

    class Stop(Exception):
        pass

    def stop(seed, **kw):
        raise Stop()
    import vine_robot_isaacgymenvs_amd.utils.utils as uu
    monkeypatch.setattr(uu, "set_seed", stop)
    args = ["task=Vine5LinkMovingBase", "num_envs=4", "headless=True",
            "task.env.ENV_PUSH={RATE: 0.1, IMPULSE: [0, 0.01], PER_EPISODE: True}",
            "task.env.ENV_DRAW_ADR={NAMES: {PUSH_IMPULSE: {START: [0, 0], STEP: 0.002}}}"]
    cfg = load_config(overrides=args + ["test=True"])
    with caplog.at_level(logging.INFO), pytest.raises(Stop):
        train.launch(cfg)
    assert cfg["task"]["env"]["ENV_DRAW_ADR"] == {}
    assert any("ENV_DRAW_ADR is forced off" in r.getMessage() for r in caplog.records)
    cfg = load_config(overrides=args + ["multi_gpu=True"])
    with pytest.raises(ConfigError, match="ENV_DRAW_ADR with multi_gpu=True"):
        train.launch(cfg)
    del seen


# ------------------------------------------------------------------------------------------------------------ the replay
def test_replay_with_start_at_the_limits_and_no_probe_is_the_three_observers_draw():
    """START = the limits and BOUNDARY_FRACTION 0 over 10 episodes of 70 envs: every table behind every step is
    ``named_draw.draw`` of the three observers, bit for bit, and nothing else moves."""
    n, T = 70, 50
    names = {"SENSOR_DELAY": {"START": [0, 3], "STEP": 1}, "SENSOR_NOISE_STD": {"START": [0.0, 0.01], "STEP": 0.003},
             "PUSH_IMPULSE": {"START": [0.0, 0.01], "STEP": 0.004}, "TARGET_VEL_ALONG": {"START": [-0.3, 0.3], "STEP": 0.05}}
    env = env_cfg(names, BOUNDARY_FRACTION=0.0)
    cfgs = observer_cfgs(env)
    adr = env_draw_adr.draw_adr_config(env, *cfgs)
    gids = np.arange(n) + 1000
    own = [named_draw.draw(named_draw.named(m.NAMES, m.DRAW_NAMES, c), 42, gids, 0, env_draw_adr.INTEGER).astype(np.float32)
           for m, c in zip(MODULES, cfgs)]
    tables = tables_at_start(adr, cfgs, 42, gids)
    for g in range(3):
        assert np.array_equal(bits(tables[g]), bits(own[g]))
    resets = np.zeros((T, n), dtype=bool)
    for e in range(n):
        resets[(4 + e % 3)::5, e] = True
    steps = env_draw_adr.draw_adr_replay(adr, 42, gids, resets, np.ones((T, n), dtype=bool), tables, cfgs)
    assert steps[-1]["episode_index"].min() >= 8
    for t in (0, 4, 5, 6, 23, T - 1):
        k = steps[t]["episode_index"]
        for g, (m, c) in enumerate(zip(MODULES, cfgs)):
            want = named_draw.draw(named_draw.named(m.NAMES, m.DRAW_NAMES, c), 42, gids, k, env_draw_adr.INTEGER).astype(np.float32)
            assert np.array_equal(bits(steps[t]["tables"][g]), bits(want)), (t, g)
    last = steps[-1]
    assert not last["widen"].any() and not last["counts"].any() and (last["probe"] == -1).all() and last["cursor"] == 0
    assert not env_draw_adr.draw_adr_max_widen(adr).any()


def scripted(adr, cfgs, reach, n=24, T=240, every=4, seed=42, **keys):
    resets = np.zeros((T, n), dtype=bool)
    resets[every - 1::every] = True
    gids = np.arange(n)
    return env_draw_adr.draw_adr_replay(adr, seed, gids, resets, reach(T, n), tables_at_start(adr, cfgs, seed, gids), cfgs, **keys), resets


def test_replay_on_hand_made_flags():
    env = env_cfg(dict(NAMES, SENSOR_NOISE_STD={"START": [0.0, 0.0], "STEP": 0.003}), QUEUE=2, BOUNDARY_FRACTION=0.6)
    cfgs = observer_cfgs(env)
    adr = env_draw_adr.draw_adr_config(env, *cfgs)
    top = env_draw_adr.draw_adr_max_widen(adr)
    assert top[SLOT("SENSOR_DELAY")].tolist() == [1, 2] and top[SLOT("SENSOR_NOISE_STD")].tolist() == [0, 4]
    assert top[SLOT("PUSH_IMPULSE")].tolist() == [1, 2] and top[SLOT("TARGET_VEL_ALONG")].tolist() == [6, 6]
    # all reached: widens and stops at every limit
    steps, resets = scripted(adr, cfgs, lambda T, n: np.ones((T, n), dtype=bool))
    assert np.array_equal(steps[-1]["widen"], top)
    ranges = env_draw_adr.draw_adr_ranges(adr, steps[-1]["widen"])
    assert ranges == {name: tuple(adr["LIMITS"][name]) for name in adr["NAMES"]}
    assert all(w <= top[b >> 1, b & 1] for _, b, w, _ in steps[-1]["history"]) and len(steps[-1]["history"]) == top.sum()
    # SENSOR_DELAY hits both integer ends, and a probing episode's value is exactly its boundary
    seen = set()
    for t in np.flatnonzero(resets.any(axis=1)):
        s = steps[t]
        in_force = env_draw_adr.draw_adr_ranges(adr, s["widen"])
        for name, (lo, hi) in in_force.items():
            g, r, _ = env_draw_adr.place_of(name)
            row, b = s["tables"][g][r], 2 * SLOT(name)
            assert np.array_equal(bits(row[s["probe"] == b]), bits(np.full((s["probe"] == b).sum(), lo)))
            assert np.array_equal(bits(row[s["probe"] == b + 1]), bits(np.full((s["probe"] == b + 1).sum(), hi)))
            assert row.min() >= np.float32(lo) and row.max() <= np.float32(hi), (t, name)
        seen |= set(s["tables"][0][0].tolist())
        assert np.array_equal(s["tables"][0][0], np.floor(s["tables"][0][0]))
    assert seen == {0.0, 1.0, 2.0, 3.0}
    # a symmetric START [0, 0] of TARGET_VEL_ALONG widens to both signs
    vel = steps[-1]["tables"][2][0]
    assert vel.min() < -0.1 and vel.max() > 0.1 and steps[-1]["widen"][SLOT("TARGET_VEL_ALONG")].tolist() == [6, 6]
    # none reached: never leaves START
    steps, _ = scripted(adr, cfgs, lambda T, n: np.zeros((T, n), dtype=bool))
    assert not steps[-1]["widen"].any() and len(steps[-1]["history"]) == 0 and steps[-1]["consumed"][..., 0].sum() > 20
    assert steps[-1]["consumed"][..., 1].sum() == 0
    assert (steps[-1]["tables"][2][0] == 0.0).all() and (steps[-1]["tables"][0][0] == 1.0).all()
    # reached, then not: comes back one step per decision and stops at START
    def there_and_back(T, n):
        reach = np.ones((T, n), dtype=bool)
        reach[T // 2:] = False
        return reach
    steps, _ = scripted(adr, cfgs, there_and_back, T=480)
    assert np.array_equal(steps[239]["widen"], top) and not steps[-1]["widen"].any()
    last = {}
    for _, b, w, _ in steps[-1]["history"]:
        assert abs(w - last.get(b, 0)) == 1 and 0 <= w <= top[b >> 1, b & 1]
        last[b] = w
    assert set(last.values()) == {0} and len(steps[-1]["history"]) == 2 * top.sum()


def test_the_range_formula_stays_inside_the_limits():
    rng = np.random.default_rng(3)
    for _ in range(200):
        lo, hi = np.sort(rng.uniform(-3.0, 3.0, 2))
        s_lo, s_hi = np.sort(rng.uniform(lo, hi, 2))
        step = float(rng.choice([1e-3, 0.05, 0.3, 7.0]))
        adr = {"NAMES": {"TARGET_VEL_ALONG": {"START": [float(s_lo), float(s_hi)], "STEP": step}},
               "LIMITS": {"TARGET_VEL_ALONG": [float(lo), float(hi)]}}
        s = SLOT("TARGET_VEL_ALONG")
        top = env_draw_adr.draw_adr_max_widen(adr)[s]
        assert top.min() >= 0
        for w_lo in sorted({0, 1, int(top[0]) // 2, max(int(top[0]) - 1, 0), int(top[0])}):
            for w_hi in sorted({0, 1, int(top[1]) // 2, max(int(top[1]) - 1, 0), int(top[1])}):
                widen = np.zeros((abi.VDA_NAMES, 2), dtype=np.int64)
                widen[s] = min(w_lo, top[0]), min(w_hi, top[1])
                a, b = env_draw_adr.draw_adr_ranges(adr, widen)["TARGET_VEL_ALONG"]
                assert lo <= a <= s_lo <= s_hi <= b <= hi
                if widen[s, 0] == top[0]:
                    assert a == lo
                if widen[s, 1] == top[1]:
                    assert b == hi


# ------------------------------------------------------------------------------------------------ the episode-log join
def stand_in(adr):
    """An ``EnvDrawAdr`` that holds host tensors: what ``state_dict`` / ``load_state_dict`` and the join touch."""
    import torch
    a = env_draw_adr.EnvDrawAdr.__new__(env_draw_adr.EnvDrawAdr)
    a.adr, a.widen = adr, torch.zeros((abi.VDA_NAMES, 2), dtype=torch.int32)
    a.widen0, a.cursor, a.history_harvested = np.zeros((abi.VDA_NAMES, 2), dtype=np.int64), torch.zeros(1, dtype=torch.int64), 0
    a.history_rows, a.seed, a.env_id_offset = np.zeros((0, 4), dtype=np.int64), 42, 0
    return a


def test_rows_join_the_range_in_force_with_a_dropped_predecessor_and_a_restored_widen(tmp_path):
    """A scripted all-reaching run with QUEUE 1 resumed from a widen that is not zero: the rows (env, end step, episode)
    joined through the history and ``widen0`` give the replay's own value of that episode; with one row dropped, the episode
    behind it is NaN with draw_probe -2 and is counted; the names not under ADR keep the observer's own join."""
    n, T = 6, 60
    env = env_cfg(QUEUE=1, BOUNDARY_FRACTION=0.6)
    cfgs = observer_cfgs(env)
    adr = env_draw_adr.draw_adr_config(env, *cfgs)
    first = stand_in(adr)
    first.widen[SLOT("TARGET_VEL_ALONG"), 0], first.widen[SLOT("TARGET_VEL_ALONG"), 1], first.widen[SLOT("SENSOR_DELAY"), 1] = 1, 3, 1
    resumed = stand_in(adr)
    resumed.load_state_dict(first.state_dict())
    widen0 = resumed.widen0
    assert widen0.sum() == 5

    def reach(T, n):
        r = np.ones((T, n), dtype=bool)
        r[T // 2:] = False
        return r
    steps, resets = scripted(adr, cfgs, reach, n=n, T=T, every=5, widen0=widen0)
    history = steps[-1]["history"]
    assert len(history) >= 6 and np.array_equal(steps[0]["widen"], widen0)
    envs, end = np.nonzero(resets.T)
    episode = np.concatenate([np.arange(resets[:, e].sum()) for e in range(n)])
    at = episodes.drawn_at(envs, episode, end)
    resumed.history_rows = history
    params, probe = resumed.episode_params(envs, episode, at)
    wrong = env_draw_adr.draw_adr_episode_params(adr, 42, envs, episode, at, history)[0]
    start = env_draw_adr.start_rows(adr, 42, np.arange(n))
    for r in range(len(envs)):
        for name in adr["NAMES"]:
            g, row, _ = env_draw_adr.place_of(name)
            want = steps[at[r]]["tables"][g][row, envs[r]] if episode[r] else start[name][envs[r]]
            assert np.float32(params[name][r]) == want and params[name][r] == np.float64(want), (r, name)
        assert probe[r] == (steps[at[r]]["probe"][envs[r]] if episode[r] else -1)
    assert (probe >= 0).any() and not np.array_equal(params["TARGET_VEL_ALONG"], wrong["TARGET_VEL_ALONG"])
    rows = {name: np.zeros(len(envs), dtype=np.int64 if name in episodes.INT_COLUMNS else np.float32) for name in episodes.COLUMNS}
    rows.update(env=envs, end_step=end, episode=episode)
    joined = episodes.with_draw_params(rows, lambda e, k: env_sensor.episode_params(cfgs[0], 42, np.asarray(e), k))
    out, unknown = episodes.with_draw_adr_params(joined, resumed.episode_params)
    assert unknown == 0 and np.array_equal(out["draw_probe"], probe)
    for name in adr["NAMES"]:
        assert np.array_equal(out["param_" + name], params[name]), name
    assert np.array_equal(out["param_SENSOR_HOLD"], joined["param_SENSOR_HOLD"])      # not under ADR: today's join
    assert not np.array_equal(out["param_SENSOR_DELAY"], joined["param_SENSOR_DELAY"])
    keep = ~((envs == 1) & (episode == 2))
    kept = {k: v[keep] for k, v in rows.items()}
    out, unknown = episodes.with_draw_adr_params(kept, resumed.episode_params)
    lost = (kept["env"] == 1) & (kept["episode"] == 3)
    assert unknown == 1 and lost.sum() == 1 and out["draw_probe"][lost].tolist() == [-2]
    assert all(np.isnan(out["param_" + name][lost]).all() and not np.isnan(out["param_" + name][~lost]).any() for name in adr["NAMES"])
    empty = {k: v[:0] for k, v in rows.items()}
    assert episodes.with_draw_adr_params(empty, resumed.episode_params)[1] == 0

    # the file: configuration, complete history, history_dropped and widen0 ride along, and the offline reader rebuilds the columns
    path = str(tmp_path / "e.npz")
    observers = [{"spec": c, "seed": 42, "env_id_offset": 0} for c in cfgs]
    episodes.save(path, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {"maxEpisodeLength": 5}, sensor=observers[0], push=observers[1],
                  target=observers[2], draw_adr={"config": adr, "history": history, "history_dropped": 2, "widen0": widen0, "seed": 42,
                                                 "env_id_offset": 0})
    config, stored, dropped, stored0, reader = episodes.load_env_draw_adr(path)
    assert config == adr and np.array_equal(stored, history) and dropped == 2 and np.array_equal(stored0, widen0)
    p3, probe3 = reader(envs, episode, at)
    assert np.array_equal(probe3, probe) and all(np.array_equal(p3[name], params[name]) for name in adr["NAMES"])
    back = episodes.load_rows_with_params(path)
    assert np.array_equal(back["draw_probe"], probe) and np.array_equal(back["param_TARGET_VEL_ALONG"], params["TARGET_VEL_ALONG"])
    assert np.array_equal(back["param_SENSOR_HOLD"], joined["param_SENSOR_HOLD"]) and np.array_equal(back["episode"], episode)
    plain = str(tmp_path / "plain.npz")
    episodes.save(plain, rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {}, sensor=observers[0])
    assert episodes.load_env_draw_adr(plain) == (None, None, 0, None, None) and "draw_probe" not in episodes.load_rows_with_params(plain)


def test_the_checkpoint_entry_round_trip():
    """``EnvDrawAdr.state_dict`` / ``load_state_dict`` on a stand-in: what the checkpoint keeps is ``widen``; a widen that does
    not fit the configuration is refused, and so is a restore into a run under way; ``scalars_of`` states the ranges."""
    import torch
    adr = adr_of()
    a = stand_in(adr)
    a.widen[SLOT("TARGET_VEL_ALONG"), 1], a.widen[SLOT("SENSOR_DELAY"), 0] = 5, 1
    state = a.state_dict()
    assert state["names"] == list(NAMES) and state["widen"][SLOT("TARGET_VEL_ALONG")].tolist() == [0, 5] and state["widen"].shape == (9, 2)
    b = stand_in(adr)
    b.load_state_dict(state)
    assert torch.equal(a.widen, b.widen) and np.array_equal(b.widen0, state["widen"])
    ints = np.concatenate([state["widen"].reshape(-1), np.zeros(36, dtype=np.int64)])
    ints[18 + 4 * SLOT("PUSH_IMPULSE")], ints[18 + 4 * SLOT("PUSH_IMPULSE") + 1] = 4, 3
    scalars = env_draw_adr.scalars_of(adr, ints)
    assert scalars["draw_adr/TARGET_VEL_ALONG_hi"] == 0.25 and scalars["draw_adr/TARGET_VEL_ALONG_lo"] == 0.0
    assert scalars["draw_adr/SENSOR_DELAY_lo"] == 0.0 and scalars["draw_adr/SENSOR_DELAY_hi"] == 1.0
    assert scalars["draw_adr/probing_reach_rate"] == 0.75 and len(scalars) == 7
    assert "draw_adr/probing_reach_rate" not in env_draw_adr.scalars_of(adr, np.zeros(54, dtype=np.int64))
    state["widen"][SLOT("SENSOR_DELAY"), 0] = 2                    # beyond the limit: one step from START 1 to 0
    with pytest.raises(ValueError, match="ENV_DRAW_ADR: the checkpoint's widen does not fit this configuration"):
        b.load_state_dict(state)
    with pytest.raises(ValueError, match="does not fit"):
        b.load_state_dict({"widen": a.state_dict()["widen"], "names": ["PUSH_IMPULSE"]})
    with pytest.raises(ValueError, match="does not fit"):
        b.load_state_dict({"widen": np.zeros((abi.VR_NAMES, 2), dtype=np.int64)})      # ENV_PARAMS_ADR's entry is not this one
    b.cursor[0] = 3
    with pytest.raises(RuntimeError, match="before the first step"):
        b.load_state_dict(a.state_dict())
    import vine_robot_isaacgymenvs_amd.learning.a2c_continuous as a2c
    source = inspect.getsource(a2c)
    assert 'state["draw_adr"]' in source and 'load_state_dict(ckpt["draw_adr"])' in source
