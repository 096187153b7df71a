"""ENV_TARGET without a GPU: include/vine_env_target.h against its ctypes mirror and the build plumbing of the sixteenth unit,
every refusal of the host entry point (those that need a handle through the stand-alone scripts/env_target_host_check.cpp,
built with the host's sanitizers) and every ``ConfigError`` by name, the draw against ``redraw_value``, and
utils/env_target.py target_replay on hand-made rows: first frames, reflections, a landing exactly on the span, resting envs,
the per-episode rewrite, the three modes, POS_ONLY and a clamped column."""
import ctypes as C
import hashlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, load_config, native
from vine_robot_isaacgymenvs_amd.utils import env_params, env_target, episodes
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 42
F = abi
f32 = np.float32
CDT = env_target.control_period(0.00833, 4)


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


def config(mode="free", cdt=CDT, **keys):
    env = {"ENV_TARGET": keys, "CREATE_SHELF": mode == "shelf", "CREATE_PIPE": mode == "pipe"}
    return env_target.target_config(env, cdt)


def layout(mode, col=22, inv=(0.5, 1.25), clip=5.0, cdt=CDT):
    return {"mode": mode, "vel_column": col, "inv_obs_scale": np.asarray(inv, dtype=f32), "clip": f32(clip), "cdt": f32(cdt)}


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_equals_the_mirror_the_struct_size_and_the_build_wiring(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vine_env_target.h")).read(), flags=re.S)
    for macro, value in (("VINE_ENV_TARGET_ABI_VERSION", abi.ENV_TARGET_ABI_VERSION), ("VINE_ENV_TARGET_THREADS", abi.ENV_TARGET_THREADS)):
        assert int(re.search(r"#define %s (\d+)\s" % macro, text).group(1)) == value, macro
    assert abi.ENV_TARGET_THREADS == 256
    for enum, prefix, names in (("VineEnvTargetSlot", "VTG_", abi.ENV_TARGET_NAMES + ["NAMES"]),
                                ("VineEnvTargetRow", "VTM_", ["ANCHOR_Y", "ANCHOR_Z", "DEPTH0", "AXIS_C", "AXIS_S", "OFF_ALONG", "OFF_ACROSS",
                                                              "VEL_ALONG", "VEL_ACROSS", "COUNT"]),
                                ("VineEnvTargetMode", "VINE_TARGET_", ["FREE", "SHELF", "PIPE"])):
        body = re.search(r"typedef enum %s \{(.*?)\}" % enum, text, flags=re.S).group(1)
        assert [w.split("=")[0].strip() for w in body.split(",")] == [prefix + n for n in names], enum
    assert abi.ENV_TARGET_NAMES == ["VEL_ALONG", "VEL_ACROSS", "SPAN_ALONG", "SPAN_ACROSS"] and abi.VTG_NAMES == 4 and abi.VTM_COUNT == 9
    assert [getattr(abi, "VTG_" + n) for n in abi.ENV_TARGET_NAMES] == [0, 1, 2, 3]
    assert (abi.VTM_ANCHOR_Y, abi.VTM_DEPTH0, abi.VTM_AXIS_C, abi.VTM_OFF_ALONG, abi.VTM_VEL_ALONG, abi.VTM_VEL_ACROSS) == (0, 2, 3, 5, 7, 8)
    assert (abi.TARGET_FREE, abi.TARGET_SHELF, abi.TARGET_PIPE) == (0, 1, 2)
    body = re.search(r"typedef struct VineEnvTargetSpec \{(.*?)\} VineEnvTargetSpec;", text, flags=re.S).group(1)
    fields = [re.sub(r"\[.*?\]", "", decl.strip()).replace("*", " ").split()[-1] for decl in body.split(";") if decl.strip()]
    assert fields == [f[0] for f in abi.VineEnvTargetSpec._fields_]
    assert lib.vine_env_target_spec_size() == C.sizeof(abi.VineEnvTargetSpec) == 24 + 4 * 48 + 4 * 4 + 4 * 4 + 8 == 256
    functions = sorted(set(re.findall(r"\b(vine_env_target[a-z_0-9]*)\s*\(", text)))
    assert functions == sorted(abi.ENV_TARGET_PROTOTYPES) and len(functions) == 3
    for name in functions:
        assert hasattr(lib, name), name
    decl = re.search(r"int vine_env_target_scheduled\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == len(abi.ENV_TARGET_PROTOTYPES["vine_env_target_scheduled"][1]) == 10
    assert "declare_env_target" in inspect.getsource(abi.declare_all)
    # the sixteenth translation unit, behind the fifteen; its pragma, the flag that makes the compiler honour it, its headers
    assert "for src in POLICY_UNITS + (SRC_MPC_OBSERVE,) + (SRC_MPC_FILTER,) + (SRC_TARGET,):" in inspect.getsource(native.build)
    assert os.path.basename(native.SRC_TARGET) == "vine_env_target.hip" and os.path.exists(native.SRC_TARGET)
    assert native.SRC_TARGET in native.DEPS and any(d.endswith("vine_env_target.h") for d in native.DEPS)
    headers = native._SOURCE_HEADERS[native.SRC_TARGET]
    assert any(d.endswith("vine_env_target.h") for d in headers) and any(d.endswith("vine_named_draw.h") for d in headers)
    assert native._SOURCE_FLAGS[native.SRC_TARGET] == ["-ffp-contract=fast-honor-pragmas"]
    flags = native._flags(native.SRC_TARGET)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast") and "-ffp-contract=off" not in flags
    source = open(native.SRC_TARGET).read()
    assert source.index("#pragma clang fp contract(off)") < source.index("#include")
    assert "__shared__" not in source and "atomic" not in source.replace("no atomics", "")
    for slot, word in enumerate(("TARGET_VEL_ALONG", "TARGET_VEL_ACROSS", "TARGET_SPAN_ALONG", "TARGET_SPAN_ACROSS")):
        assert env_target.DRAW_NAMES[slot] == word
        assert env_params.name_key(word) == int.from_bytes(hashlib.sha256(word.encode()).digest()[:8], "little")
    # the step kernels and the PPO kernels know nothing of it
    for other in (native.SRC, native.SRC_PPO, native.SRC_PUSH, native.SRC_SENSOR):
        assert "env_target" not in open(other).read().lower(), other


# ------------------------------------------------------------------------------------------- refusals of the entry point
def spec_call(lib, vcfg, spec, per_episode=None, mutate=None, device_values=0x1000):
    names, values = env_target.target_names(spec)
    if mutate:
        mutate(names)
    out = abi.VineEnvTargetSpec()
    rc = lib.vine_env_target_spec(C.byref(vcfg), names, values.ctypes.data if len(values) else None,
                                  device_values if len(values) else None, len(values),
                                  int(spec["PER_EPISODE"]) if per_episode is None else per_episode, C.byref(out))
    return rc, lib.vine_last_error().decode(), out


def test_spec_entry_point_fills_and_refuses_by_name(lib, vcfg):
    good = config(VEL_ALONG={"values": [0.0, 0.05, -0.05]}, VEL_ACROSS=[-0.02, 0.02], SPAN_ALONG=0.03, SPAN_ACROSS=[0.01, 0.02])
    rc, msg, out = spec_call(lib, vcfg, good)
    assert rc == abi.OK and out.checked == 1 and out.seed == SEED and out.per_episode == 0 and out.num_values == 3, msg
    assert out.mode == abi.TARGET_FREE and out.num_obs == 28 and out.vel_column == 28 - 16 + 10
    assert [out.name[s].form for s in range(4)] == [abi.REDRAW_VALUES, abi.REDRAW_RANGE, abi.REDRAW_NUMBER, abi.REDRAW_RANGE]
    assert [out.name[s].key for s in range(4)] == [env_params.name_key(n) for n in env_target.DRAW_NAMES]
    # cdt and the reciprocals are the step kernels' own words (vine_hip.hip make_params: c.dt * (float)cfi; (float)(1.0 / (double)s))
    assert bits(out.cdt) == bits(f32(vcfg.dt) * f32(vcfg.control_freq_inv))
    assert list(vcfg.obs_scaling[22:24]) == [f32(2.0), f32(0.732)]
    assert np.array_equal(bits(np.array(out.inv_obs_scale)), bits((1.0 / np.asarray(vcfg.obs_scaling[22:24], dtype=np.float64)).astype(f32)))
    assert bits(out.clip_observations) == bits(vcfg.clip_observations)
    lay = env_target.layout_of(out)
    assert lay["mode"] == 0 and lay["vel_column"] == 22 and bits(lay["cdt"]) == bits(out.cdt)
    for obs_type, column, num_obs in ((1, 12, 18), (2, -1, 14), (3, 22, 26), (4, 22, 26), (5, 22, 26)):
        c = type(vcfg).from_buffer_copy(vcfg)
        assert lib.vine_config_set_obs_type(C.byref(c), obs_type, int(obs_type in abi.SCALABLE_OBS_TYPES)) == 0
        rc, msg, o = spec_call(lib, c, good)
        assert rc == abi.OK and (o.vel_column, o.num_obs) == (column, num_obs), msg

    def setter(slot, **fields):
        def mutate(names):
            for k, v in fields.items():
                setattr(names[slot], k, v)
        return mutate
    refusals = [
        (dict(mutate=setter(0, form=abi.REDRAW_ABSENT)), "TARGET_VEL_ALONG: absent"),
        (dict(mutate=setter(3, form=7)), "TARGET_SPAN_ACROSS: unknown form"),
        (dict(mutate=setter(2, reserved=1)), "TARGET_SPAN_ALONG: reserved must be 0"),
        (dict(mutate=setter(1, lo=2.0, hi=1.0)), "TARGET_VEL_ACROSS: a range needs finite lo <= hi"),
        (dict(mutate=setter(3, hi=float("inf"))), "TARGET_SPAN_ACROSS: a range needs finite lo <= hi"),
        (dict(mutate=setter(2, lo=float("nan"))), "TARGET_SPAN_ALONG: the number is not finite"),
        (dict(mutate=setter(2, lo=-0.03)), "TARGET_SPAN_ALONG: must not be negative"),
        (dict(mutate=setter(3, lo=-0.001)), "TARGET_SPAN_ACROSS: must not be negative"),
        (dict(mutate=setter(0, values_count=4)), "TARGET_VEL_ALONG: the extent of the value list lies outside the values array"),
        (dict(mutate=setter(0, values_first=-1)), "TARGET_VEL_ALONG: the extent of the value list lies outside the values array"),
        (dict(mutate=setter(0, radix=0)), "TARGET_VEL_ALONG: radix must be at least 1"),
        (dict(mutate=setter(2, lo=0.0008)), "TARGET_VEL_ALONG: max|VEL| * cdt exceeds 2 * min SPAN_ALONG"),
        (dict(mutate=setter(2, lo=0.0)), "TARGET_VEL_ALONG: max|VEL| * cdt exceeds 2 * min SPAN_ALONG"),
        (dict(mutate=setter(3, lo=0.0)), "TARGET_VEL_ACROSS: max|VEL| * cdt exceeds 2 * min SPAN_ACROSS"),
        (dict(mutate=setter(1, lo=-2.0)), "TARGET_VEL_ACROSS: max|VEL| * cdt exceeds 2 * min SPAN_ACROSS"),
        (dict(device_values=None), "the value lists need a host and a device array"),
    ]
    for kw, match in refusals:
        rc, msg, out = spec_call(lib, vcfg, good, **kw)
        assert rc == abi.ERR_INVALID_ARG and match in msg and out.checked == 0, (kw, msg)
    for keys, match in ((dict(VEL_ALONG={"values": [0.01, float("nan")]}), "TARGET_VEL_ALONG: a listed value is not finite"),
                        (dict(SPAN_ALONG={"values": [0.03, -0.03]}), "TARGET_SPAN_ALONG: must not be negative"),
                        (dict(VEL_ACROSS=float("nan")), "TARGET_VEL_ACROSS: the number is not finite")):
        rc, msg, _ = spec_call(lib, vcfg, dict(good, **keys))
        assert rc == abi.ERR_INVALID_ARG and match in msg, msg
    # nothing to do, unless per episode
    zero = dict(good, VEL_ALONG={"values": [0.0]}, VEL_ACROSS=[0.0, 0.0], SPAN_ALONG=0.0, SPAN_ACROSS=0.0)
    rc, msg, _ = spec_call(lib, vcfg, zero)
    assert rc == abi.ERR_INVALID_ARG and "TARGET_VEL_ALONG and TARGET_VEL_ACROSS are both constant zero: nothing to do" in msg
    assert spec_call(lib, vcfg, zero, per_episode=1)[0] == abi.OK
    # one axis at rest needs no span
    assert spec_call(lib, vcfg, dict(good, VEL_ACROSS=0.0, SPAN_ACROSS=0.0))[0] == abi.OK
    # with an obstacle nothing moves across; the two obstacles at once
    along = dict(good, VEL_ACROSS=0.0, SPAN_ACROSS=0.0)
    for flag, mode in ((abi.FLAG_CREATE_SHELF, abi.TARGET_SHELF), (abi.FLAG_CREATE_PIPE, abi.TARGET_PIPE)):
        c = type(vcfg).from_buffer_copy(vcfg)
        c.set_flag(flag, True)
        rc, msg, out = spec_call(lib, c, along)
        assert rc == abi.OK and out.mode == mode, msg
        rc, msg, _ = spec_call(lib, c, good)
        assert rc == abi.ERR_INVALID_ARG and "TARGET_VEL_ACROSS: must be constant zero with an obstacle" in msg
        rc, msg, _ = spec_call(lib, c, dict(along, SPAN_ACROSS=0.01))
        assert rc == abi.ERR_INVALID_ARG and "TARGET_SPAN_ACROSS: must be constant zero with an obstacle" in msg
    c = type(vcfg).from_buffer_copy(vcfg)
    c.set_flag(abi.FLAG_CREATE_SHELF, True)
    c.set_flag(abi.FLAG_CREATE_PIPE, True)
    rc, msg, _ = spec_call(lib, c, along)
    assert rc == abi.ERR_INVALID_ARG and "CREATE_SHELF together with CREATE_PIPE" in msg
    # the step's velocity-success term assumes a resting target
    c = type(vcfg).from_buffer_copy(vcfg)
    c.reward_weights[3] = 0.25
    rc, msg, _ = spec_call(lib, c, good)
    assert rc == abi.ERR_INVALID_ARG and "VELOCITY_SUCCESS_REWARD_WEIGHT must be 0" in msg
    assert lib.vine_env_target_spec(None, None, None, None, 0, 0, None) == abi.ERR_INVALID_ARG
    assert "null argument to vine_env_target_spec" in lib.vine_last_error().decode()
    # the launch entry point: null pointers and an unchecked spec, refused before anything touches a device
    out = spec_call(lib, vcfg, good)[2]
    assert lib.vine_env_target_scheduled(None, C.byref(out), *([16] * 7), None) == abi.ERR_INVALID_ARG
    assert "null argument to vine_env_target_scheduled" in lib.vine_last_error().decode()
    for k in range(7):                               # each of the seven buffers in turn
        args = [16] * 7
        args[k] = None
        assert lib.vine_env_target_scheduled(0x10, C.byref(out), *args, None) == abi.ERR_INVALID_ARG
        assert "null argument to vine_env_target_scheduled" in lib.vine_last_error().decode()
    unchecked = abi.VineEnvTargetSpec()
    unchecked.abi_version = abi.ENV_TARGET_ABI_VERSION
    assert lib.vine_env_target_scheduled(0x10, C.byref(unchecked), *([16] * 7), None) == abi.ERR_INVALID_ARG
    assert "was not filled by vine_env_target_spec" in lib.vine_last_error().decode()


def test_the_refusals_through_the_stand_alone_host_check(tmp_path):
    """scripts/env_target_host_check.cpp, built as its head says -- the unit's HOST code under AddressSanitizer and UBSan, with a
    stand-in handle -- walks every refusal of the spec by name and those of the launch that need a handle.  A few seconds of
    hipcc."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "env_target_host_check")
    source = os.path.join(REPO, "scripts", "env_target_host_check.cpp")
    text = open(source).read()
    for word in ("TARGET_VEL_ALONG: absent", "a range needs finite lo <= hi", "must not be negative", "max|VEL| * cdt exceeds 2 * min SPAN_ALONG",
                 "max|VEL| * cdt exceeds 2 * min SPAN_ACROSS", "must be constant zero with an obstacle", "CREATE_SHELF together with CREATE_PIPE",
                 "both constant zero: nothing to do", "VELOCITY_SUCCESS_REWARD_WEIGHT must be 0", "mode is not that of the handle's obstacle flags",
                 "was not filled by vine_env_target_spec", "vel_column lies outside the observation row"):
        assert word in text, word
    subprocess.check_call([hipcc, "--offload-arch=" + native.ARCH, "-O1", "-g", "-std=c++17", "-ffp-contract=fast-honor-pragmas",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-x", "hip",
                           source, native.SRC_TARGET, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "env target host check ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------- the configuration
def test_default_is_off_and_every_config_error_names_the_key():
    cfg = load_config()["task"]
    assert cfg["env"]["ENV_TARGET"] == {} and env_target.target_config(cfg["env"], CDT) is None and env_target.target_config({}, CDT) is None
    assert "task.env.ENV_TARGET" in __import__("vine_robot_isaacgymenvs_amd.cfg.defaults", fromlist=["x"]).__doc__
    assert bits(CDT) == bits(f32(0.00833) * f32(4))
    good = config(VEL_ALONG=[-0.05, 0.05], SPAN_ALONG={"values": [0.02, 0.03]}, PER_EPISODE=True)
    assert good == {"VEL_ALONG": [-0.05, 0.05], "VEL_ACROSS": 0.0, "SPAN_ALONG": {"values": [0.02, 0.03]}, "SPAN_ACROSS": 0.0,
                    "PER_EPISODE": True, "MODE": abi.TARGET_FREE}
    assert config("shelf", VEL_ALONG=0.05, SPAN_ALONG=0.03)["MODE"] == abi.TARGET_SHELF
    assert config("pipe", VEL_ALONG=0.05, SPAN_ALONG=0.03)["MODE"] == abi.TARGET_PIPE
    assert env_target.varying_names(good) == ["VEL_ALONG", "SPAN_ALONG"]
    for mode, keys, match in (
            ("free", dict(VEL_ALONG=0.05, SPAN_ALONG=0.03, SPEED=2), "ENV_TARGET: unknown key.* SPEED"),
            ("free", dict(VEL_ALONG={"value": [1]}, SPAN_ALONG=0.03), "ENV_TARGET.VEL_ALONG: a mapping must hold the one key 'values'"),
            ("free", dict(VEL_ALONG={"values": []}, SPAN_ALONG=0.03), "ENV_TARGET.VEL_ALONG: 'values' must be a non-empty list"),
            ("free", dict(VEL_ALONG=[0.1, 0.2, 0.3], SPAN_ALONG=0.03), "ENV_TARGET.VEL_ALONG: a range is"),
            ("free", dict(VEL_ALONG=[0.05, -0.05], SPAN_ALONG=0.03), "ENV_TARGET.VEL_ALONG: lo > hi"),
            ("free", dict(VEL_ALONG="fast", SPAN_ALONG=0.03), "ENV_TARGET.VEL_ALONG: 'fast' is not a finite number"),
            ("free", dict(VEL_ALONG=True, SPAN_ALONG=0.03), "ENV_TARGET.VEL_ALONG: True is not a finite number"),
            ("free", dict(VEL_ALONG=float("inf"), SPAN_ALONG=0.03), "ENV_TARGET.VEL_ALONG: inf is not a finite number"),
            ("free", dict(VEL_ALONG=1e300, SPAN_ALONG=0.03), "ENV_TARGET.VEL_ALONG: 1e\\+300 does not fit a float32"),
            ("free", dict(VEL_ALONG=0.05, SPAN_ALONG={"values": [0.03, float("nan")]}), "ENV_TARGET.SPAN_ALONG: nan is not a finite number"),
            ("free", dict(VEL_ALONG=0.05, SPAN_ALONG=-0.03), "ENV_TARGET.SPAN_ALONG: -0.03 is negative"),
            ("free", dict(VEL_ALONG=0.05, SPAN_ALONG=0.03, SPAN_ACROSS=[-0.01, 0.01]), "ENV_TARGET.SPAN_ACROSS: -0.01 is negative"),
            ("free", dict(VEL_ALONG=0.05, SPAN_ALONG=0.03, PER_EPISODE="yes"), "ENV_TARGET.PER_EPISODE must be a bool"),
            ("free", dict(VEL_ALONG=0.05), r"ENV_TARGET.VEL_ALONG: max\|VEL\| \* cdt = .* exceeds 2 \* min SPAN_ALONG"),
            ("free", dict(VEL_ALONG=[-2.0, 0.05], SPAN_ALONG=0.03), r"ENV_TARGET.VEL_ALONG: max\|VEL\| \* cdt = .* exceeds 2 \* min SPAN_ALONG"),
            ("free", dict(VEL_ALONG=0.05, SPAN_ALONG={"values": [0.03, 0.0005]}), r"ENV_TARGET.VEL_ALONG: max\|VEL\| \* cdt"),
            ("free", dict(VEL_ACROSS=0.05, SPAN_ALONG=0.03), r"ENV_TARGET.VEL_ACROSS: max\|VEL\| \* cdt = .* exceeds 2 \* min SPAN_ACROSS"),
            ("shelf", dict(VEL_ALONG=0.05, SPAN_ALONG=0.03, VEL_ACROSS=0.01, SPAN_ACROSS=0.01), "ENV_TARGET.VEL_ACROSS must be constant zero with an obstacle"),
            ("pipe", dict(VEL_ALONG=0.05, SPAN_ALONG=0.03, SPAN_ACROSS=0.01), "ENV_TARGET.SPAN_ACROSS must be constant zero with an obstacle"),
            ("free", dict(SPAN_ALONG=0.03), "ENV_TARGET: VEL_ALONG and VEL_ACROSS are both constant zero: nothing to do"),
            ("free", dict(VEL_ALONG=[0, 0], VEL_ACROSS={"values": [0.0]}), "ENV_TARGET: VEL_ALONG and VEL_ACROSS are both constant zero")):
        with pytest.raises(ConfigError, match=match):
            config(mode, **keys)
    with pytest.raises(ConfigError, match="ENV_TARGET must be a mapping"):
        env_target.target_config({"ENV_TARGET": [1, 2]}, CDT)
    with pytest.raises(ConfigError, match="CREATE_SHELF together with CREATE_PIPE"):
        env_target.target_config({"ENV_TARGET": {"VEL_ALONG": 0.05, "SPAN_ALONG": 0.03}, "CREATE_SHELF": True, "CREATE_PIPE": True}, CDT)
    with pytest.raises(ConfigError, match="VELOCITY_SUCCESS_REWARD_WEIGHT must be 0"):
        env_target.target_config({"ENV_TARGET": {"VEL_ALONG": 0.05, "SPAN_ALONG": 0.03}, "VELOCITY_SUCCESS_REWARD_WEIGHT": 0.5}, CDT)
    with pytest.raises(ConfigError, match="control period must be positive"):
        config(cdt=0.0, VEL_ALONG=0.05, SPAN_ALONG=0.03)
    assert config(PER_EPISODE=True)["PER_EPISODE"] is True               # per episode, constant zero is allowed to run
    # a step that lands exactly on 2 * SPAN is a path one reflection keeps
    assert config(VEL_ALONG=1.0, SPAN_ALONG=float(CDT) / 2)["SPAN_ALONG"] == float(CDT) / 2


def test_python_and_library_refuse_the_same_specs(lib, vcfg):
    """Every spec ``target_config`` lets through is one ``vine_env_target_spec`` fills, at the edge of the path check too."""
    cdt = f32(vcfg.dt) * f32(vcfg.control_freq_inv)
    for vel in (0.05, 0.7, 1.0, 1.3):
        for span in (float(cdt) * 0.35, float(cdt) / 2, float(cdt) * 0.65):
            keys = dict(VEL_ALONG=[-vel, vel / 2], SPAN_ALONG=span)
            try:
                spec = config(cdt=cdt, **keys)
            except ConfigError:
                names = dict(VEL_ALONG=[-vel, vel / 2], VEL_ACROSS=0.0, SPAN_ALONG=span, SPAN_ACROSS=0.0, PER_EPISODE=False)
                assert spec_call(lib, vcfg, names)[0] == abi.ERR_INVALID_ARG, (vel, span)
                assert f32(vel) * cdt > f32(2.0) * f32(span)
            else:
                assert spec_call(lib, vcfg, spec)[0] == abi.OK, (vel, span)
                assert f32(vel) * cdt <= f32(2.0) * f32(span)


def test_sysid_and_mpc_force_it_off_and_the_test_entry_keeps_it_on(caplog, monkeypatch, tmp_path):
    import logging
    from vine_robot_isaacgymenvs_amd import train
    from vine_robot_isaacgymenvs_amd.learning import a2c_continuous
    from vine_robot_isaacgymenvs_amd.utils import mpc, sysid
    assert ("env", "ENV_TARGET", {}) in sysid.FORCED and ("env", "ENV_TARGET", {}) in mpc.FORCED
    moving = {"VEL_ALONG": 0.05, "SPAN_ALONG": 0.03}
    cfg = load_config()["task"]
    cfg["env"]["ENV_TARGET"] = dict(moving)
    with caplog.at_level(logging.INFO):
        out = sysid.candidate_config(cfg, {"DAMPING": [0.01, 0.05]}, 70, 12)
        model = mpc.model_config(cfg, 4, 16)
    assert out["env"]["ENV_TARGET"] == {} and model["env"]["ENV_TARGET"] == {} and cfg["env"]["ENV_TARGET"] == moving
    assert sum("ENV_TARGET forced from" in r.getMessage() for r in caplog.records) == 2
    seen = {}
    monkeypatch.setattr(a2c_continuous.Runner, "run", lambda self, args: seen.update(args) or "ran")
    monkeypatch.chdir(tmp_path)
    cfg = load_config("config", overrides=["task.env.ENV_TARGET={VEL_ALONG: {values: [0, 0.05, -0.05]}, SPAN_ALONG: 0.03}", "test=True",
                                           "multi_gpu=False"])
    assert train.launch(cfg) == "ran" and seen["play"] is True
    assert cfg["task"]["env"]["ENV_TARGET"] == {"VEL_ALONG": {"values": [0, 0.05, -0.05]}, "SPAN_ALONG": 0.03}


# ----------------------------------------------------------------------------------------------------------- the draw
def redraw_value64(form, key_name, seed, g, k, radix=1):
    """``redraw_value`` of csrc/vine_named_draw.h in Python integers and floats, one (g, k) at a time."""
    m64 = (1 << 64) - 1

    def mix(x):
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m64
        return x ^ (x >> 31)
    if not isinstance(form, (dict, list)):
        return float(form)
    pre = (mix((seed ^ env_params.name_key(key_name)) & m64) + g * 0x9E3779B97F4A7C15) & m64
    u = float(mix(pre ^ mix(k)) >> 11) * (1.0 / 9007199254740992.0)
    if isinstance(form, dict):
        vals = form["values"]
        return vals[(g // radix) % len(vals)] if k == 0 else vals[min(int(np.floor(u * len(vals))), len(vals) - 1)]
    return form[0] + (form[1] - form[0]) * u


def test_the_draw_is_redraw_value_keyed_by_the_global_id_and_the_episode():
    spec = config(VEL_ALONG={"values": [0.0, 0.05, -0.05]}, VEL_ACROSS=[-0.02, 0.02], SPAN_ALONG={"values": [0.03, 0.04]}, SPAN_ACROSS=0.01,
                  PER_EPISODE=True)
    gids = np.asarray([0, 1, 2, 3, 5, 69, 1000, 1069, 2 ** 31 + 5])
    for k in (0, 1, 2, 7):
        got = env_target.draw_target(spec, SEED, gids, k)
        assert got.shape == (4, len(gids)) and got.dtype == np.float64
        for i, g in enumerate(gids.tolist()):
            radix = 1
            for s, (name, draw_name) in enumerate(zip(env_target.NAMES, env_target.DRAW_NAMES)):
                assert got[s, i] == redraw_value64(spec[name], draw_name, SEED, g, k, radix), (k, g, name)
                radix *= len(spec[name]["values"]) if isinstance(spec[name], dict) else 1
    first = env_target.draw_target(spec, SEED, np.arange(12), 0)
    assert list(first[0]) == [0.0, 0.05, -0.05] * 4 and list(first[2]) == [0.03] * 3 + [0.04] * 3 + [0.03] * 3 + [0.04] * 3      # the mixed radix
    later = env_target.draw_target(spec, SEED, np.arange(600), 3)
    assert set(later[0]) == {0.0, 0.05, -0.05} and (np.abs(later[1]) <= 0.02).all() and len(set(later[1])) == 600
    assert np.array_equal(env_target.draw_target(spec, SEED, np.arange(8) + 1000, 2), env_target.draw_target(spec, SEED, np.arange(1008), 2)[:, 1000:])
    assert not np.array_equal(later[1], env_target.draw_target(spec, SEED + 1, np.arange(600), 3)[1])
    params = env_target.episode_params(spec, SEED, np.arange(6), np.asarray([0, 0, 1, 1, 2, 2]))
    assert sorted(params) == ["TARGET_SPAN_ALONG", "TARGET_VEL_ACROSS", "TARGET_VEL_ALONG"] and params["TARGET_VEL_ALONG"].dtype == np.float32
    held = dict(spec, PER_EPISODE=False)
    assert np.array_equal(env_target.episode_params(held, SEED, np.arange(6), np.arange(6))["TARGET_VEL_ALONG"],
                          env_target.draw_target(spec, SEED, np.arange(6), 0)[0].astype(f32))


# -------------------------------------------------------------------------------------------------- the replay, by hand
def hand_state(n, steps=1, ty=-0.25, tz=0.6, depth=0.05, angle=0.3):
    f, e = np.meshgrid(np.arange(F.VF_COUNT), np.arange(n), indexing="ij")
    st = ((f + 1) / 8.0 + e / 65536.0).astype(f32)
    st[F.VF_TARGET_Y], st[F.VF_TARGET_Z], st[F.VF_OBJ_DEPTH], st[F.VF_OBJ_ANGLE] = ty, tz, depth, angle
    return np.repeat(st[None], steps, axis=0)


def run(spec, lay, state, obs, progress, resets, table, **kw):
    return env_target.target_replay(spec, SEED, np.arange(state.shape[2]), lay, state, obs, progress, resets, table=table, **kw)


def _continue(spec, lay, st, obs, progress, resets, prev, first):
    """One more launch behind ``prev``, stated with scalars: the header's five steps, env by env, independent of the array code."""
    mode, col, inv, clip, cdt = lay["mode"], lay["vel_column"], lay["inv_obs_scale"], lay["clip"], lay["cdt"]
    st, ob, motion, table = st.copy(), obs.copy(), prev["motion"].copy(), prev["table"].copy()
    n = st.shape[1]
    reflected, moving = np.zeros(n, bool), np.zeros(n, bool)
    for e in range(n):
        m = motion[:, e]
        if first[e]:
            m[F.VTM_ANCHOR_Y], m[F.VTM_ANCHOR_Z] = st[F.VF_TARGET_Y, e], st[F.VF_TARGET_Z, e]
            m[F.VTM_DEPTH0] = st[F.VF_OBJ_DEPTH, e] if mode else 0
            if mode == F.TARGET_PIPE:
                m[F.VTM_AXIS_C], m[F.VTM_AXIS_S] = np.cos(np.float64(st[F.VF_OBJ_ANGLE, e])), np.sin(np.float64(st[F.VF_OBJ_ANGLE, e]))
            else:
                m[F.VTM_AXIS_C], m[F.VTM_AXIS_S] = 1, 0
            m[F.VTM_OFF_ALONG] = m[F.VTM_OFF_ACROSS] = 0
            m[F.VTM_VEL_ALONG], m[F.VTM_VEL_ACROSS] = table[0, e], table[1, e]
        ay, az, d0, c, s, oa, oc, va, vc = (f32(x) for x in m)
        if va == 0 and vc == 0:
            continue
        moving[e] = True
        if col >= 0:
            wy, wz = ((va, vc), (-va, f32(0)), (f32(-va) * c, f32(-va) * s))[mode]
            ob[e, col] = min(max(f32(ob[e, col] + f32(wy * inv[0])), -clip), clip)
            ob[e, col + 1] = min(max(f32(ob[e, col + 1] + f32(wz * inv[1])), -clip), clip)
        axes = [(F.VTM_OFF_ALONG, F.VTM_VEL_ALONG, 2)] + ([(F.VTM_OFF_ACROSS, F.VTM_VEL_ACROSS, 3)] if mode == F.TARGET_FREE else [])
        for off_row, vel_row, span_row in axes:
            S, v = table[span_row, e], f32(m[vel_row])
            nx = f32(f32(m[off_row]) + f32(v * cdt))
            if nx > S:
                nx, v, reflected[e] = f32(S - f32(nx - S)), f32(-v), True
            elif nx < -S:
                nx, v, reflected[e] = f32(-S - f32(nx + S)), f32(-v), True
            m[off_row], m[vel_row] = nx, v
        oa, oc = f32(m[F.VTM_OFF_ALONG]), f32(m[F.VTM_OFF_ACROSS])
        if mode == F.TARGET_FREE:
            st[F.VF_TARGET_Y, e], st[F.VF_TARGET_Z, e] = f32(ay + oa), f32(az + oc)
        elif mode == F.TARGET_SHELF:
            st[F.VF_TARGET_Y, e], st[F.VF_OBJ_DEPTH, e] = f32(ay - oa), f32(d0 + oa)
        else:
            st[F.VF_TARGET_Y, e], st[F.VF_TARGET_Z, e] = f32(ay - f32(oa * c)), f32(az - f32(oa * s))
            st[F.VF_OBJ_DEPTH, e] = f32(d0 + oa)
    episode = prev["episode_index"].copy()
    if spec["PER_EPISODE"]:
        for e in np.flatnonzero(resets):
            episode[e] += 1
            table[:, e] = env_target.draw_target(spec, SEED, [e], episode[e]).astype(f32)[:, 0]
    return {"state": st, "obs": ob, "table": table, "motion": motion, "fresh": np.zeros(n, np.uint8), "episode_index": episode,
            "first": first, "moving": moving, "reflected": reflected}


def same(a, b, what=""):
    for key in ("state", "obs", "table", "motion"):
        assert np.array_equal(bits(a[key]), bits(b[key])), (what, key)
    for key in ("fresh", "episode_index", "first", "moving", "reflected"):
        assert np.array_equal(a[key], b[key]), (what, key)


def test_the_array_replay_equals_the_scalar_statement_of_the_header_in_the_three_modes():
    """40 launches over hand-made flags (episodes of 5 + e % 7 steps), value lists with zero and both signs, per episode; the
    array code of ``target_replay`` against ``_continue``, which walks the header's five steps env by env."""
    n, steps = 23, 40
    t, e = np.meshgrid(np.arange(steps + 1), np.arange(n), indexing="ij")
    prog = (t + e) % (5 + e % 7)
    progress, resets = prog[:steps].astype(np.int64), (prog[1:] == 0).astype(np.int64)
    rng = np.random.default_rng(5)
    for mode_name, mode, col, keys in (
            ("free", F.TARGET_FREE, 22, dict(VEL_ALONG={"values": [0.0, 0.4, -0.4]}, VEL_ACROSS={"values": [0.0, 0.25, -0.3]}, SPAN_ALONG=0.03,
                                             SPAN_ACROSS=[0.02, 0.03])),
            ("shelf", F.TARGET_SHELF, 12, dict(VEL_ALONG={"values": [0.0, 0.4, -0.4]}, SPAN_ALONG=[0.02, 0.03])),
            ("pipe", F.TARGET_PIPE, 22, dict(VEL_ALONG=[-0.5, 0.5], SPAN_ALONG={"values": [0.03, 0.012]})),
            ("pos-only", F.TARGET_FREE, -1, dict(VEL_ALONG=0.4, SPAN_ALONG=0.03))):
        spec = config(mode_name if mode_name != "pos-only" else "free", PER_EPISODE=True, **keys)
        lay = layout(mode, col)
        num_obs = 14 if col < 0 else 28
        states = np.stack([hand_state(n)[0] for _ in range(steps)])
        states[:, F.VF_TARGET_Y] = rng.uniform(-0.3, -0.1, (steps, n))
        states[:, F.VF_TARGET_Z] = rng.uniform(0.5, 0.7, (steps, n))
        states[:, F.VF_OBJ_DEPTH] = rng.uniform(0.0, 0.1, (steps, n))
        states[:, F.VF_OBJ_ANGLE] = rng.uniform(-0.5, 0.5, (steps, n))
        obs = rng.uniform(-1, 1, (steps, n, num_obs)).astype(f32)
        external = [[] for _ in range(steps)]
        external[7], external[19] = [3, 4], [0, 22]
        got = env_target.target_replay(spec, SEED, np.arange(n) + 100, lay, states, obs, progress, resets, external_resets=external)
        prev = {"motion": np.zeros((F.VTM_COUNT, n), f32), "table": env_target.draw_target(spec, SEED, np.arange(n) + 100, 0).astype(f32),
                "episode_index": np.zeros(n, np.int64)}
        fresh = np.ones(n, bool)
        reflections = 0
        for k in range(steps):
            fresh[external[k]] = True
            first = (progress[k] == 0) | fresh
            want = _continue(spec, lay, states[k], obs[k], progress[k], resets[k], prev, first)
            # (the scalar statement draws by local index: shift it to the global ids the array code was given)
            for x in np.flatnonzero(resets[k]):
                want["table"][:, x] = env_target.draw_target(spec, SEED, [x + 100], want["episode_index"][x]).astype(f32)[:, 0]
            same(got[k], want, (mode_name, k))
            reflections += int(want["reflected"].sum())
            fresh[:] = False
            prev = want
            rest = [f for f in range(F.VF_COUNT) if f not in ((F.VF_TARGET_Y, F.VF_TARGET_Z), (F.VF_TARGET_Y, F.VF_OBJ_DEPTH),
                                                              (F.VF_TARGET_Y, F.VF_TARGET_Z, F.VF_OBJ_DEPTH))[mode]]
            assert np.array_equal(bits(got[k]["state"][rest]), bits(states[k][rest])), (mode_name, k)      # nothing else of the block
            quiet = ~got[k]["moving"]
            assert np.array_equal(bits(got[k]["state"][:, quiet]), bits(states[k][:, quiet]))
            assert np.array_equal(bits(got[k]["obs"][quiet]), bits(obs[k][quiet]))
            if col >= 0:
                others = [j for j in range(num_obs) if j not in (col, col + 1)]
                assert np.array_equal(bits(got[k]["obs"][:, others]), bits(obs[k][:, others]))
            else:
                assert np.array_equal(bits(got[k]["obs"]), bits(obs[k]))                                  # POS_ONLY: no column written
            if mode != F.TARGET_FREE:
                assert not got[k]["motion"][[F.VTM_OFF_ACROSS, F.VTM_VEL_ACROSS]].any()
        assert reflections > 5 and got[-1]["episode_index"].max() >= 3, mode_name
        assert np.array_equal(got[-1]["episode_index"], resets.sum(axis=0))


def test_first_frames_by_progress_and_by_fresh_leave_the_resets_own_target():
    spec = config(VEL_ALONG=0.4, VEL_ACROSS=-0.25, SPAN_ALONG=0.03, SPAN_ACROSS=0.02)
    n = 4
    table = np.repeat(np.asarray([[0.4], [-0.25], [0.03], [0.02]], f32), n, axis=1)
    lay = layout(F.TARGET_FREE)
    st = hand_state(n, 3)
    st[1, F.VF_TARGET_Y], st[2, F.VF_TARGET_Y] = -0.21, -0.19        # the step reset env 1 before launch 1; reset_idx env 2 before launch 2
    obs = np.zeros((3, n, 28), f32)
    progress = np.asarray([[0, 0, 0, 0], [1, 0, 1, 1], [2, 1, 2, 2]])
    out = run(spec, lay, st, obs, progress, np.zeros((3, n)), table, external_resets=[[], [], [2]])
    assert out[0]["first"].all() and list(out[1]["first"]) == [False, True, False, False] and list(out[2]["first"]) == [False, False, True, False]
    # launch 0: anchors are the state's words, offsets are one step from zero, the velocity columns hold the velocity scaled
    step_y, step_z = f32(0.4) * CDT, f32(-0.25) * CDT
    assert np.array_equal(bits(out[0]["motion"][F.VTM_ANCHOR_Y]), bits(st[0, F.VF_TARGET_Y]))
    assert np.array_equal(bits(out[0]["motion"][F.VTM_OFF_ALONG]), bits(np.full(n, step_y))) and (out[0]["fresh"] == 0).all()
    assert np.array_equal(bits(out[0]["state"][F.VF_TARGET_Y]), bits(st[0, F.VF_TARGET_Y] + step_y))
    assert np.array_equal(bits(out[0]["state"][F.VF_TARGET_Z]), bits(st[0, F.VF_TARGET_Z] + step_z))
    assert np.array_equal(bits(out[0]["obs"][:, 22]), bits(np.full(n, f32(0.4) * f32(0.5))))
    assert np.array_equal(bits(out[0]["obs"][:, 23]), bits(np.full(n, f32(-0.25) * f32(1.25))))
    # launch 1: env 1 starts anew from the state's target, the others go on from their anchor
    assert bits(out[1]["motion"][F.VTM_ANCHOR_Y, 1]) == bits(f32(-0.21)) and bits(out[1]["motion"][F.VTM_OFF_ALONG, 1]) == bits(step_y)
    assert bits(out[1]["state"][F.VF_TARGET_Y, 1]) == bits(f32(-0.21) + step_y)
    assert bits(out[1]["motion"][F.VTM_OFF_ALONG, 0]) == bits(f32(step_y + step_y))
    assert bits(out[1]["state"][F.VF_TARGET_Y, 0]) == bits(f32(-0.25) + f32(step_y + step_y))
    # launch 2: env 2 by fresh, though its progress is 2
    assert bits(out[2]["motion"][F.VTM_ANCHOR_Y, 2]) == bits(f32(-0.19)) and bits(out[2]["motion"][F.VTM_OFF_ALONG, 2]) == bits(step_y)


def test_reflection_at_both_ends_and_a_landing_exactly_on_the_span():
    spec = config(VEL_ALONG={"values": [0.5, -0.5, 0.25]}, SPAN_ALONG={"values": [0.03, 0.03125]}, cdt=f32(0.03125))
    lay = layout(F.TARGET_FREE, cdt=0.03125)
    # env 0: +0.5 over 0.03; env 1: -0.5 over 0.03; env 2: +0.25 * 2^-5 = 2^-7 per step over 2^-5: lands exactly on S at step 4
    table = np.asarray([[0.5, -0.5, 0.25], [0, 0, 0], [0.03, 0.03, 0.03125], [0, 0, 0]], f32)
    n, steps = 3, 9
    st = hand_state(n, steps)
    progress = np.arange(steps)[:, None].repeat(n, 1)
    out = run(spec, lay, st, np.zeros((steps, n, 28), f32), progress, np.zeros((steps, n)), table)
    off = np.stack([w["motion"][F.VTM_OFF_ALONG] for w in out])
    vel = np.stack([w["motion"][F.VTM_VEL_ALONG] for w in out])
    step = f32(0.5) * f32(0.03125)
    # env 0: 0.015625, then 0.03125 > 0.03 -> 0.03 - (0.03125 - 0.03), velocity flipped
    assert bits(off[0, 0]) == bits(step) and bits(off[1, 0]) == bits(f32(0.03) - f32(f32(step + step) - f32(0.03))) and vel[1, 0] == f32(-0.5)
    assert out[1]["reflected"][0] and not out[0]["reflected"][0] and off[2, 0] < off[1, 0]
    assert bits(off[1, 1]) == bits(f32(-0.03) - f32(f32(-step - step) + f32(0.03))) and vel[1, 1] == f32(0.5) and out[1]["reflected"][1]
    assert (np.abs(off[:, :2]) <= f32(0.03)).all()
    # the observation's velocity column follows the flip one launch later: launch 1 still adds the velocity it arrived with
    assert out[1]["obs"][0, 22] == f32(0.5) * f32(0.5) and out[2]["obs"][0, 22] == f32(-0.5) * f32(0.5)
    # env 2: exactly S after four steps is not a reflection; the fifth step is
    assert list(off[:5, 2]) == [2.0 ** -7, 2.0 ** -6, 3 * 2.0 ** -7, 2.0 ** -5, 3 * 2.0 ** -7]
    assert not out[3]["reflected"][2] and vel[3, 2] == f32(0.25) and out[4]["reflected"][2] and vel[4, 2] == f32(-0.25)
    # the state follows: anchor + offset, one add
    for k in range(steps):
        assert np.array_equal(bits(out[k]["state"][F.VF_TARGET_Y]), bits(f32(-0.25) + off[k]))


def test_an_env_at_rest_stores_nothing_and_keeps_a_negative_zero():
    spec = config(VEL_ALONG={"values": [0.0, 0.4]}, SPAN_ALONG=0.03)
    table = np.asarray([[0.0, 0.4, -0.0], [-0.0, 0, 0], [0.03] * 3, [0] * 3], f32)
    lay = layout(F.TARGET_FREE)
    st = hand_state(3, 2, ty=-0.0, tz=-0.0)
    obs = np.full((2, 3, 28), -0.0, f32)
    out = run(spec, lay, st, obs, np.asarray([[0] * 3, [1] * 3]), np.zeros((2, 3)), table)
    for k in range(2):
        assert list(out[k]["moving"]) == [False, True, False]
        for e in (0, 2):                              # +0 and -0 velocities alike: every bit kept, the -0 of target and column too
            assert np.array_equal(bits(out[k]["state"][:, e]), bits(st[k][:, e])) and np.array_equal(bits(out[k]["obs"][e]), bits(obs[k][e]))
            assert bits(out[k]["state"][F.VF_TARGET_Y, e]) == 0x80000000 and bits(out[k]["obs"][e, 22]) == 0x80000000
        assert bits(out[k]["state"][F.VF_TARGET_Z, 1]) == 0 and bits(out[k]["obs"][1, 23]) == 0      # the moving env: -0 + 0 is +0
    assert bits(out[0]["motion"][F.VTM_ANCHOR_Y, 0]) == 0x80000000 and bits(out[0]["motion"][F.VTM_VEL_ALONG, 2]) == 0x80000000


def test_per_episode_rewrites_flagged_envs_only_and_after_the_move():
    spec = config(VEL_ALONG=[-0.5, 0.5], SPAN_ALONG=0.03, PER_EPISODE=True)
    n = 6
    table = np.repeat(np.asarray([[0.3], [0.0], [0.03], [0.0]], f32), n, axis=1)        # hand-made entries
    st = hand_state(n, 3)
    resets = np.asarray([[0, 1, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0]])
    progress = np.asarray([[3] * n, [4, 0, 4, 4, 0, 4], [5, 1, 5, 5, 1, 5]])
    out = run(spec, layout(F.TARGET_FREE), st, np.zeros((3, n, 28), f32), progress, resets, table)
    assert list(out[0]["episode_index"]) == [0, 1, 0, 0, 1, 0] and list(out[2]["episode_index"]) == [0, 2, 1, 0, 1, 0]
    drawn = env_target.draw_target(spec, SEED, np.arange(n), 1).astype(f32)
    for e in range(n):
        want = drawn[:, e] if e in (1, 4) else table[:, e]
        assert np.array_equal(bits(out[0]["table"][:, e]), bits(want)), e
    # the flagged step itself still moved with the old velocity; the new one is taken at the next first frame
    assert (out[0]["motion"][F.VTM_VEL_ALONG] == f32(0.3)).all()
    assert bits(out[1]["motion"][F.VTM_VEL_ALONG, 1]) == bits(drawn[0, 1]) and bits(out[1]["motion"][F.VTM_VEL_ALONG, 0]) == bits(f32(0.3))
    assert np.array_equal(bits(out[2]["table"][:, 1]), bits(env_target.draw_target(spec, SEED, [1], 2).astype(f32)[:, 0]))
    held = run(dict(spec, PER_EPISODE=False), layout(F.TARGET_FREE), st, np.zeros((3, n, 28), f32), progress, resets, table)
    assert not held[2]["episode_index"].any() and np.array_equal(bits(held[2]["table"]), bits(table))


def test_shelf_and_pipe_move_along_the_depth_axis_and_keep_the_obstacle_where_it_is():
    """The pose a reset would derive from the moved target, the moved depth and the stored angle (vine_hip.hip
    task_obstacle_poses) is the pose the anchor gave, to float32 round-off; the observation gets the world velocity."""
    n, steps = 5, 12
    R = 0.0735
    for mode_name, mode in (("shelf", F.TARGET_SHELF), ("pipe", F.TARGET_PIPE)):
        spec = config(mode_name, VEL_ALONG={"values": [0.4, -0.4]}, SPAN_ALONG=0.03)
        table = np.asarray([[0.4, -0.4, 0.4, -0.4, 0.4], [0] * n, [0.03] * n, [0] * n], f32)
        lay = layout(mode)
        st0 = hand_state(n, 1, ty=-0.25, tz=0.62, depth=0.05, angle=0.3)[0]
        st0[F.VF_OBJ_ANGLE] = np.linspace(-0.6, 0.6, n).astype(f32)
        state, outs = st0, []
        for k in range(steps):
            prev = outs[-1] if outs else None
            if prev is None:
                w = run(spec, lay, state[None], np.zeros((1, n, 28), f32), np.zeros((1, n)), np.zeros((1, n)), table)[0]
            else:
                w = _continue(spec, lay, state, np.zeros((n, 28), f32), np.full(n, k), np.zeros(n), prev, np.zeros(n, bool))
            outs.append(w)
            state = w["state"]
            c, s = w["motion"][F.VTM_AXIS_C].astype(np.float64), w["motion"][F.VTM_AXIS_S].astype(np.float64)
            ty, tz, depth = (state[f].astype(np.float64) for f in (F.VF_TARGET_Y, F.VF_TARGET_Z, F.VF_OBJ_DEPTH))
            ay, az, d0 = np.float64(f32(-0.25)), np.float64(f32(0.62)), np.float64(f32(0.05))
            assert np.array_equal(bits(state[F.VF_OBJ_DEPTH]), bits(f32(0.05) + w["motion"][F.VTM_OFF_ALONG]))
            if mode == F.TARGET_SHELF:
                assert np.abs((ty + (depth - 0.2)) - (ay + (d0 - 0.2))).max() < 4 * np.spacing(f32(0.5))
                assert np.array_equal(bits(state[F.VF_TARGET_Z]), bits(st0[F.VF_TARGET_Z])) and (c == 1).all() and (s == 0).all()
                arrived = table[0] if k == 0 else outs[-2]["motion"][F.VTM_VEL_ALONG]       # the velocity the launch found
                assert np.array_equal(bits(w["obs"][:, 22]), bits(-arrived * f32(0.5)))
                assert not w["obs"][:, 23].any()
            else:
                assert np.abs((ty + depth * c + R * s) - (ay + d0 * c + R * s)).max() < 4 * np.spacing(f32(0.5))
                assert np.abs((tz + depth * s - R * c) - (az + d0 * s - R * c)).max() < 4 * np.spacing(f32(1.0))
                assert np.allclose(c, np.cos(st0[F.VF_OBJ_ANGLE].astype(np.float64)), atol=1e-7)
        offs = np.stack([w["motion"][F.VTM_OFF_ALONG] for w in outs])
        assert (np.abs(offs) <= f32(0.03)).all() and any(w["reflected"].any() for w in outs)
        # a positive offset is deeper, and the target went against the axis
        deeper = offs[0] > 0
        assert (outs[0]["state"][F.VF_OBJ_DEPTH][deeper] > f32(0.05)).all() and (outs[0]["state"][F.VF_TARGET_Y][deeper] < f32(-0.25)).all()


def test_a_column_is_clamped_at_clip_observations_and_noise_already_there_is_kept():
    spec = config(VEL_ALONG={"values": [0.4, -0.4]}, VEL_ACROSS={"values": [0.3]}, SPAN_ALONG=0.03, SPAN_ACROSS=0.03)
    table = np.asarray([[0.4, -0.4, 0.4], [0.3, 0.3, 0.3], [0.03] * 3, [0.03] * 3], f32)
    lay = layout(F.TARGET_FREE, inv=(20.0, 1.0), clip=5.0)
    obs = np.zeros((1, 3, 28), f32)
    obs[0, :, 22], obs[0, :, 23] = [0.0, 0.0, 0.0123], [0.25, -0.125, 4.9]
    out = run(spec, lay, hand_state(3), obs, np.zeros((1, 3)), np.zeros((1, 3)), table)[0]
    assert list(out["obs"][:, 22]) == [5.0, -5.0, 5.0]                               # 0.4 * 20 = 8 -> clip
    assert np.array_equal(bits(out["obs"][:, 23]), bits(np.asarray([f32(0.25) + f32(0.3), f32(-0.125) + f32(0.3), 5.0], f32)))


# ------------------------------------------------------------------------------------------------ the episode log's join
def test_the_episode_log_joins_and_stores_the_target_columns(tmp_path):
    spec = config(VEL_ALONG={"values": [0.0, 0.05, -0.05]}, SPAN_ALONG=[0.02, 0.03], PER_EPISODE=True)
    rows = episodes.concat_rows([])
    n = 9
    rows = {k: np.zeros(n, dtype=v.dtype) for k, v in rows.items()}
    rows["env"], rows["episode"] = np.arange(n) % 5, np.arange(n) // 5
    rows["end_step"] = np.arange(n) + 3

    def params(envs, eps):
        return env_target.episode_params(spec, SEED, np.asarray(envs) + 1000, eps)
    joined = episodes.with_target_params(rows, params)
    want = env_target.draw_target(spec, SEED, rows["env"] + 1000, rows["episode"]).astype(f32)
    assert np.array_equal(bits(joined["param_TARGET_VEL_ALONG"]), bits(want[0])) and np.array_equal(bits(joined["param_TARGET_SPAN_ALONG"]), bits(want[2]))
    assert "param_TARGET_VEL_ACROSS" not in joined and "param_TARGET_SPAN_ACROSS" not in joined
    path = episodes.save(str(tmp_path / "log.npz"), rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {},
                         target={"spec": spec, "seed": SEED, "env_id_offset": 1000})
    back_spec, episode, back_params = episodes.load_env_target(path)
    assert back_spec == spec and np.array_equal(episode, rows["episode"])
    back = episodes.load_rows_with_params(path)
    assert np.array_equal(bits(back["param_TARGET_VEL_ALONG"]), bits(want[0]))
    plain = episodes.save(str(tmp_path / "plain.npz"), rows, np.zeros(abi.EVAL_NUM_TOTALS), 0, {})
    assert episodes.load_env_target(plain) == (None, None, None)
