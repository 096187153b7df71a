"""MPC_TRACK without a GPU: include/vine_mpc_track.h against its ctypes mirror and the build plumbing of the seventeenth unit,
every ``ConfigError`` of ``track_config`` and of ``play``'s refused combinations, every refusal of ``vine_mpc_track_spec`` by name
through the library and through the stand-alone scripts/mpc_track_host_check.cpp (built with the host's sanitizers), and
utils/mpc_track.py plan_replay and node_replay: against a scalar walk on hand-made rows, and ``exact`` against k more launches
of ``env_target.target_replay``."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_target, mpc, mpc_track
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError, parse_scalar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = abi
f32 = np.float32
CDT = env_target.control_period(0.00833, 4)
MODES = (abi.TARGET_FREE, abi.TARGET_SHELF, abi.TARGET_PIPE)


@pytest.fixture(scope="module")
def lib():
    native.build()
    return native.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_header_equals_the_mirror_the_struct_size_and_the_build_wiring(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vine_mpc_track.h")).read(), flags=re.S)
    for macro, value in (("VINE_MPC_TRACK_ABI_VERSION", abi.MPC_TRACK_ABI_VERSION), ("VINE_MPC_TRACK_THREADS", abi.MPC_TRACK_THREADS),
                         ("VINE_MPC_TRACK_WORDS", abi.MPC_TRACK_WORDS)):
        assert int(re.search(r"#define %s (\d+)\s" % macro, text).group(1)) == value, macro
    assert abi.MPC_TRACK_THREADS == 256 and abi.MPC_TRACK_WORDS == 3
    body = re.search(r"typedef enum VineMpcTrackPath \{(.*?)\}", text, flags=re.S).group(1)
    assert [w.split("=")[0].strip() for w in body.split(",")] == ["VINE_TRACK_" + n.upper() for n in abi.MPC_TRACK_PATHS]
    assert [int(w.split("=")[1]) for w in body.split(",")] == [abi.TRACK_EXACT, abi.TRACK_LINEAR, abi.TRACK_HELD] == [0, 1, 2]
    assert mpc_track.PATHS == ("exact", "linear", "held")
    body = re.search(r"typedef struct VineMpcTrackSpec \{(.*?)\} VineMpcTrackSpec;", text, flags=re.S).group(1)
    fields = [re.sub(r"\[.*?\]", "", decl.strip()).replace("*", " ").split()[-1] for decl in body.split(";") if decl.strip()]
    assert fields == [f[0] for f in abi.VineMpcTrackSpec._fields_]
    assert fields == ["abi_version", "num_plants", "samples", "horizon", "mode", "path", "cdt", "checked", "reserved"]
    assert lib.vine_mpc_track_spec_size() == C.sizeof(abi.VineMpcTrackSpec) == 64
    functions = sorted(set(re.findall(r"\b(vine_mpc_track[a-z_0-9]*)\s*\(", text)))
    assert functions == sorted(abi.MPC_TRACK_PROTOTYPES) and len(functions) == 4
    for name in functions:
        assert hasattr(lib, name), name
    for name, count in (("vine_mpc_track_spec", 4), ("vine_mpc_track_plan", 9), ("vine_mpc_track_scheduled", 7)):
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert len(decl.split(",")) == len(abi.MPC_TRACK_PROTOTYPES[name][1]) == count, name
    assert "declare_mpc_track" in inspect.getsource(abi.declare_all)
    # nothing of it went into the target's own header, whose functions an existing test counts
    assert "mpc_track" not in open(os.path.join(REPO, "include", "vine_env_target.h")).read()
    # the seventeenth translation unit: compiled by the loop's body behind the loop, whose pinned line stands
    build = inspect.getsource(native.build)
    assert "for src in POLICY_UNITS + (SRC_MPC_OBSERVE,) + (SRC_MPC_FILTER,) + (SRC_TARGET,):" in build
    assert build.count("compile_unit(") == 3 and "compile_unit(SRC_MPC_TRACK)" in build
    assert build.index("compile_unit(SRC_MPC_TRACK)") < build.index("proc.wait()")      # side by side with the others
    assert "seventeen translation units" in native.build.__doc__
    assert os.path.basename(native.SRC_MPC_TRACK) == "vine_mpc_track.hip" and os.path.exists(native.SRC_MPC_TRACK)
    assert native.SRC_MPC_TRACK in native.DEPS and any(d.endswith("vine_mpc_track.h") for d in native.DEPS)
    assert any(d.endswith("vine_target_path.h") for d in native.DEPS)
    headers = [os.path.basename(h) for h in native._SOURCE_HEADERS[native.SRC_MPC_TRACK]]
    assert {"vine_mpc_track.h", "vine_env_target.h", "vine_env_redraw.h", "vine_mpc.h", "vine_target_path.h"} <= set(headers)
    assert "vine_target_path.h" in [os.path.basename(h) for h in native._SOURCE_HEADERS[native.SRC_TARGET]]
    assert native._SOURCE_FLAGS[native.SRC_MPC_TRACK] == ["-ffp-contract=fast-honor-pragmas"]
    flags = native._flags(native.SRC_MPC_TRACK)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast") and "-ffp-contract=off" not in flags
    source = open(native.SRC_MPC_TRACK).read()
    assert source.index("#pragma clang fp contract(off)") < source.index("#include")
    assert "__shared__" not in source and "atomic" not in source.replace("no atomics", "")
    # the path step and the words are stated once, and both units include the statement
    shared = open(os.path.join(os.path.dirname(native.SRC_TARGET), "vine_target_path.h")).read()
    assert "target_path_advance" in shared and "target_path_words" in shared
    for unit in (native.SRC_TARGET, native.SRC_MPC_TRACK):
        text = open(unit).read()
        assert '#include "vine_target_path.h"' in text and "target_path_advance(" in text and "target_path_words<MODE>(" in text
        assert "nx = S - (nx - S)" not in text, unit
    # the step kernels, the PPO kernels and the controller's own unit know nothing of it
    for other in (native.SRC, native.SRC_PPO, native.SRC_MPC):
        assert "mpc_track" not in open(other).read().lower(), other
    assert mpc.FORCED[-1] == ("env", "ENV_TARGET", {})


# ------------------------------------------------------------------------------------------------------ the configuration
def test_every_config_error_of_track_config_and_of_play():
    for path in mpc_track.PATHS:
        assert mpc_track.track_config({"PATH": path}) == {"PATH": path}
        assert mpc_track.path_kind(path) == mpc_track.PATHS.index(path)
    assert mpc_track.track_config(parse_scalar("{PATH: exact}")) == {"PATH": "exact"}
    with pytest.raises(ConfigError, match="track=.*must be a mapping, not 'exact'"):
        mpc_track.track_config("exact")
    with pytest.raises(ConfigError, match=r"track: unknown key\(s\) KIND, path"):
        mpc_track.track_config({"PATH": "exact", "path": "exact", "KIND": 1})
    with pytest.raises(ConfigError, match="track.PATH is missing"):
        mpc_track.track_config({})
    for bad in ("Exact", "quadratic", 0, None, True):
        with pytest.raises(ConfigError, match="track.PATH must be one of exact, linear, held, not"):
            mpc_track.track_config({"PATH": bad})
    with pytest.raises(ConfigError, match="track.PATH must be one of"):
        mpc_track.path_kind("nearest")
    # play: refused before any task is created (no device needed)
    moving = {"env": {"numEnvs": 2, "ENV_TARGET": {"VEL_ALONG": 0.1, "SPAN_ALONG": 0.05}}, "seed": 0}
    resting = {"env": {"numEnvs": 2, "ENV_TARGET": {}}, "seed": 0}
    track = {"PATH": "exact"}
    with pytest.raises(ConfigError, match="track= needs a plant with task.env.ENV_TARGET"):
        mpc.play(resting, samples=16, track=track)
    with pytest.raises(ConfigError, match="track= needs a plant with task.env.ENV_TARGET"):
        mpc.play({"env": {"numEnvs": 2}, "seed": 0}, samples=16, track=track)
    with pytest.raises(ConfigError, match="track= together with policy= is refused"):
        mpc.play(moving, samples=256, track=track, policy="x.pth", policy_params={})
    with pytest.raises(ConfigError, match="track= together with adapt= is refused"):
        mpc.play(moving, samples=16, track=track, adapt={"params": {"DAMPING": [0.005, 0.1]}})
    with pytest.raises(ConfigError, match="track= together with observe= or filter= is refused"):
        mpc.play(moving, samples=16, track=track, observe={"DELAY": 1})
    with pytest.raises(ConfigError, match="track= together with observe= or filter= is refused"):
        mpc.play(moving, samples=16, track=track, observe={"DELAY": 1}, filter={})
    with pytest.raises(ConfigError, match="track.PATH must be one of"):
        mpc.play(moving, samples=16, track={"PATH": "spline"})
    with pytest.raises(ConfigError, match="track=.*must be a mapping"):
        mpc.play(moving, samples=16, track="exact")
    assert inspect.signature(mpc.play).parameters["track"].default is None
    import mpc as tool
    assert tool.OWN["track"] is None and '"track"' in inspect.getsource(tool.main) and "track=own[\"track\"]" in inspect.getsource(tool.main)
    with pytest.raises(ConfigError, match="mpc: track=.*must be a mapping, not 'exact'"):
        tool.main(["track=exact"])


# ------------------------------------------------------------------------------------------- refusals of the entry point
def plant_spec(mode=abi.TARGET_FREE, cdt=CDT):
    t = abi.VineEnvTargetSpec()
    t.abi_version, t.mode, t.cdt, t.checked = abi.ENV_TARGET_ABI_VERSION, mode, cdt, 1
    return t


def test_spec_entry_point_fills_and_refuses_by_name(lib):
    for mode in MODES:
        for kind, name in enumerate(mpc_track.PATHS):
            s = mpc_track.track_spec(lib, plant_spec(mode), mpc.mpc_config(5, 14, 12), name)
            assert (s.abi_version, s.num_plants, s.samples, s.horizon, s.mode, s.path, s.checked) == (1, 5, 14, 12, mode, kind, 1)
            assert bits(s.cdt) == bits(CDT) and list(s.reserved) == [0] * 8
    assert mpc_track.track_spec(lib, plant_spec(), mpc.mpc_config(1, 2, 1), "exact").horizon == 1
    assert mpc_track.track_spec(lib, plant_spec(), mpc.mpc_config(1, 2, abi.MPC_MAX_HORIZON), 1).horizon == 64

    def call(t, c, path):
        out = abi.VineMpcTrackSpec()
        rc = lib.vine_mpc_track_spec(C.byref(t) if t is not None else None, C.byref(c) if c is not None else None, path, C.byref(out))
        return rc, lib.vine_last_error().decode(), out

    def changed(obj, **fields):
        copy = type(obj).from_buffer_copy(obj)
        for k, v in fields.items():
            setattr(copy, k, v)
        return copy
    t, c = plant_spec(abi.TARGET_PIPE), mpc.mpc_config(5, 14, 12)
    refusals = [
        ((None, c, 0), "null argument to vine_mpc_track_spec"),
        ((t, None, 0), "null argument to vine_mpc_track_spec"),
        ((changed(t, checked=0), c, 0), "the plant's VineEnvTargetSpec was not filled by vine_env_target_spec"),
        ((changed(t, abi_version=9), c, 0), "VineEnvTargetSpec.abi_version mismatch"),
        ((changed(t, mode=3), c, 0), "VineEnvTargetSpec.mode is not a mode of this library"),
        ((t, changed(c, abi_version=9), 0), "VineMpcConfig.abi_version mismatch"),
        ((t, c, 3), "path 3 is not exact (0), linear (1) or held (2)"),
        ((t, c, -1), "path -1 is not exact (0), linear (1) or held (2)"),
        ((t, changed(c, horizon=0), 0), "needs 1 <= horizon <= VINE_MPC_MAX_HORIZON (64)"),
        ((t, changed(c, horizon=65), 0), "needs 1 <= horizon <= VINE_MPC_MAX_HORIZON (64)"),
        ((t, changed(c, num_plants=0), 0), "num_plants must be at least 1"),
        ((t, changed(c, samples=1), 0), "samples must be at least 2"),
    ]
    for args, match in refusals:
        rc, msg, out = call(*args)
        assert rc == abi.ERR_INVALID_ARG and match in msg and out.checked == 0, (match, msg)
    assert lib.vine_mpc_track_spec(C.byref(t), C.byref(c), 0, None) == abi.ERR_INVALID_ARG
    with pytest.raises(ValueError, match="MPC_TRACK: mpc track spec: the plant's VineEnvTargetSpec was not filled"):
        mpc_track.track_spec(lib, changed(t, checked=0), c, "exact")
    # the launches: null pointers and an unchecked spec, refused before anything touches a device
    good = call(t, c, 0)[2]
    assert lib.vine_mpc_track_plan(None, C.byref(good), *([16] * 6), None) == abi.ERR_INVALID_ARG
    assert "null argument to vine_mpc_track_plan" in lib.vine_last_error().decode()
    assert lib.vine_mpc_track_scheduled(None, C.byref(good), *([16] * 4), None) == abi.ERR_INVALID_ARG
    assert "null argument to vine_mpc_track_scheduled" in lib.vine_last_error().decode()


def test_the_refusals_through_the_stand_alone_host_check(tmp_path):
    """scripts/mpc_track_host_check.cpp, built as its head says -- the unit's HOST code under AddressSanitizer and UBSan, with a
    stand-in handle -- walks every refusal of the spec by name and those of the two launches, the ones that need a handle
    included.  A few seconds of hipcc.  Nothing is loaded into Python under a sanitizer."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "mpc_track_host_check")
    source = os.path.join(REPO, "scripts", "mpc_track_host_check.cpp")
    text = open(source).read()
    for word in ("null argument to vine_mpc_track_spec", "was not filled by vine_env_target_spec", "VineEnvTargetSpec.abi_version mismatch",
                 "VineMpcConfig.abi_version mismatch", "is not exact (0), linear (1) or held (2)", "needs 1 <= horizon <= VINE_MPC_MAX_HORIZON",
                 "was not filled by vine_mpc_track_spec", "the plant handle has 70 envs, not num_plants = 5",
                 "the model handle has 5 envs, not num_plants * samples = 5 * 14", "mode is not that of the handle's obstacle flags",
                 "null argument to vine_mpc_track_plan", "null argument to vine_mpc_track_scheduled"):
        assert word in text, word
    subprocess.check_call([hipcc, "--offload-arch=" + native.ARCH, "-O1", "-g", "-std=c++17", "-ffp-contract=fast-honor-pragmas",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-x", "hip",
                           source, native.SRC_MPC_TRACK, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "mpc track host check ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------------------ the replay
def scalar_plan(mode, kind, cdt, H, state, motion, table, fresh, reset):
    """The three steps of include/vine_mpc_track.h, plant by plant, on numpy float32 scalars."""
    M = state.shape[1]
    path, live, bounced = np.zeros((M, H, 3), dtype=f32), np.zeros(M, dtype=np.uint8), np.zeros((M, H), dtype=bool)
    for p in range(M):
        w0 = [f32(state[F.VF_TARGET_Y, p]), f32(state[F.VF_TARGET_Z, p]), f32(state[F.VF_OBJ_DEPTH, p])]
        path[p, 0] = w0
        ay, az, d0, c, s, oa, oc, va, vc = (f32(motion[r, p]) for r in range(F.VTM_COUNT))
        live[p] = kind != F.TRACK_HELD and reset[p] == 0 and fresh[p] == 0 and (va != 0 or vc != 0)
        for k in range(1, H):
            if not live[p]:
                path[p, k] = w0
                continue
            axes = [(oa, va, f32(table[F.VTG_SPAN_ALONG, p]))] + ([(oc, vc, f32(table[F.VTG_SPAN_ACROSS, p]))] if mode == F.TARGET_FREE else [])
            moved = []
            for off, vel, S in axes:
                n = f32(off + f32(vel * cdt))
                if kind == F.TRACK_EXACT:
                    if n > S:
                        n, vel, bounced[p, k] = f32(S - f32(n - S)), f32(-vel), True
                    elif n < -S:
                        n, vel, bounced[p, k] = f32(f32(-S) - f32(n + S)), f32(-vel), True
                moved.append((n, vel))
            oa, va = moved[0]
            if mode == F.TARGET_FREE:
                oc, vc = moved[1]
            w = list(w0)
            if mode == F.TARGET_FREE:
                w[0], w[1] = f32(ay + oa), f32(az + oc)
            elif mode == F.TARGET_SHELF:
                w[0], w[2] = f32(ay - oa), f32(d0 + oa)
            else:
                w[0], w[1], w[2] = f32(ay - f32(oa * c)), f32(az - f32(oa * s)), f32(d0 + oa)
            path[p, k] = w
    return path, live, bounced


def hand_made_rows(mode):
    """Eight plants: 0 reflects at +S, 1 at -S, 2 lands exactly on S, 3 rests with +0 and 4 with -0 velocities, 5 is flagged, 6 is
    fresh, 7 moves across only (free space; at rest along) or slowly along."""
    M = 8
    rng = np.random.default_rng(5 + mode)
    state = rng.normal(size=(F.VF_COUNT, M)).astype(f32)
    motion = np.zeros((F.VTM_COUNT, M), dtype=f32)
    motion[F.VTM_ANCHOR_Y], motion[F.VTM_ANCHOR_Z] = rng.normal(size=M), rng.normal(size=M)
    motion[F.VTM_DEPTH0] = 0.1 if mode != F.TARGET_FREE else 0.0
    angle = rng.uniform(-0.5, 0.5, size=M)
    motion[F.VTM_AXIS_C], motion[F.VTM_AXIS_S] = (np.cos(angle), np.sin(angle)) if mode == F.TARGET_PIPE else (1.0, 0.0)
    span = f32(0.025)
    motion[F.VTM_OFF_ALONG] = [0.02, -0.02, 0.0, 0.01, 0.01, 0.0, 0.0, 0.0]
    motion[F.VTM_VEL_ALONG] = [0.4, -0.4, 0.0, 0.0, -0.0, 0.4, 0.4, 0.05]
    motion[F.VTM_OFF_ALONG, 2], motion[F.VTM_VEL_ALONG, 2] = 0.005, 0.25
    if mode == F.TARGET_FREE:
        motion[F.VTM_VEL_ACROSS] = [0.1, 0.0, 0.0, 0.0, -0.0, 0.1, 0.1, -0.4]
        motion[F.VTM_VEL_ALONG, 7] = 0.0
    table = np.zeros((F.VTG_NAMES, M), dtype=f32)
    table[F.VTG_SPAN_ALONG] = span
    step = f32(0.25) * f32(CDT)
    table[F.VTG_SPAN_ALONG, 2] = f32(f32(f32(0.005) + step) + step)      # plant 2's second step lands exactly on its S
    table[F.VTG_SPAN_ACROSS] = 0.02 if mode == F.TARGET_FREE else 0.0
    fresh = np.uint8([0, 0, 0, 0, 0, 0, 1, 0])
    reset = np.int64([0, 0, 0, 0, 0, 1, 0, 0])
    return state, motion, table, fresh, reset


@pytest.mark.parametrize("mode", MODES)
def test_plan_replay_equals_a_scalar_walk_on_hand_made_rows(mode):
    state, motion, table, fresh, reset = hand_made_rows(mode)
    H = 12
    plans = {}
    for kind, name in enumerate(mpc_track.PATHS):
        got = mpc_track.plan_replay(mode, name, CDT, H, state, motion, table, fresh, reset)
        path, live, bounced = scalar_plan(mode, kind, f32(CDT), H, state, motion, table, fresh, reset)
        assert np.array_equal(bits(got["path"]), bits(path)) and np.array_equal(got["live"], live), name
        assert got["path"].dtype == np.float32 and got["live"].dtype == np.uint8 and got["path"].shape == (8, H, 3)
        if name == "exact":
            assert np.array_equal(got["reflected"], bounced)
        else:
            assert not got["reflected"].any()
        plans[name] = got
    exact, linear, held = plans["exact"], plans["linear"], plans["held"]
    assert list(exact["live"]) == list(linear["live"]) == [1, 1, 1, 0, 0, 0, 0, 1] and not held["live"].any()
    words0 = np.stack([state[F.VF_TARGET_Y], state[F.VF_TARGET_Z], state[F.VF_OBJ_DEPTH]], axis=1)
    for plan in plans.values():                       # entry 0 is the plant's column, the words themselves
        assert np.array_equal(bits(plan["path"][:, 0]), bits(words0))
    for p in (3, 4, 5, 6):                            # resting (+0 and -0), flagged, fresh: the table is defined, and holds entry 0
        for plan in plans.values():
            assert np.array_equal(bits(plan["path"][p]), bits(np.broadcast_to(words0[p], (H, 3))))
    assert np.array_equal(bits(held["path"]), bits(np.broadcast_to(words0[:, None], (8, H, 3))))
    # plant 0 turns at +S, plant 1 at -S, inside the horizon; plant 2 lands exactly on S and turns one step later
    first = [int(np.argmax(exact["reflected"][p])) for p in (0, 1, 2)]
    assert first[0] == first[1] == 1 and exact["reflected"][0].sum() >= 2
    assert first[2] == 3
    if mode == F.TARGET_FREE:
        assert bits(exact["path"][2, 2, 0]) == bits(motion[F.VTM_ANCHOR_Y, 2] + table[F.VTG_SPAN_ALONG, 2])
    # exact equals linear up to the first reflection and differs behind it
    for p in (0, 1, 2, 7):
        turn = int(np.argmax(exact["reflected"][p])) if exact["reflected"][p].any() else H
        assert np.array_equal(bits(exact["path"][p, :turn]), bits(linear["path"][p, :turn])), p
        if turn < H:
            assert not np.array_equal(bits(exact["path"][p, turn]), bits(linear["path"][p, turn])), p
    # a word the mode does not write repeats entry 0's
    live = np.flatnonzero(exact["live"])
    if mode == F.TARGET_FREE:
        assert np.array_equal(bits(exact["path"][live, :, 2]), bits(np.broadcast_to(words0[live, None, 2], (len(live), H))))
        assert len(np.unique(exact["path"][7, :, 1])) > 2 and len(np.unique(exact["path"][7, 1:, 0])) == 1    # across only
    elif mode == F.TARGET_SHELF:
        assert np.array_equal(bits(exact["path"][live, :, 1]), bits(np.broadcast_to(words0[live, None, 1], (len(live), H))))
    if mode != F.TARGET_FREE:                         # the across axis moves only in free space: its motion rows are not read
        moved = motion.copy()
        moved[F.VTM_OFF_ACROSS], moved[F.VTM_VEL_ACROSS, :3] = 0.7, 0.3
        again = mpc_track.plan_replay(mode, "exact", CDT, H, state, moved, table, fresh, reset)
        assert np.array_equal(bits(again["path"]), bits(exact["path"]))
    # H = 1: the column's words and the flags, nothing else
    one = mpc_track.plan_replay(mode, "exact", CDT, 1, state, motion, table, fresh, reset)
    assert one["path"].shape == (8, 1, 3) and np.array_equal(bits(one["path"][:, 0]), bits(words0)) and list(one["live"]) == list(exact["live"])


@pytest.mark.parametrize("mode,name", [(abi.TARGET_FREE, "free"), (abi.TARGET_SHELF, "shelf"), (abi.TARGET_PIPE, "pipe")])
def test_the_exact_plan_is_k_more_launches_of_the_target_replay(mode, name):
    """The property that ties the plan to existing code: from the motion block behind launch t0, ``env_target.target_replay``'s
    state words behind launch t0 + k equal ``plan_replay``'s ``exact`` entry k, bit for bit, for every plant (none resets, none is
    redrawn) -- through several reflections."""
    N, T0, H = 24, 5, 16
    keys = {"VEL_ALONG": {"values": [0.0, 0.4, -0.4, 0.13]}, "SPAN_ALONG": [0.02, 0.03]}
    if mode == abi.TARGET_FREE:
        keys.update(VEL_ACROSS=[-0.4, 0.4], SPAN_ACROSS=[0.02, 0.03])
    env = {"ENV_TARGET": keys, "CREATE_SHELF": name == "shelf", "CREATE_PIPE": name == "pipe"}
    spec = env_target.target_config(env, CDT)
    layout = {"mode": mode, "vel_column": 22, "inv_obs_scale": np.asarray((0.5, 1.25), dtype=f32), "clip": f32(5.0), "cdt": f32(CDT)}
    rng = np.random.default_rng(3)
    T = T0 + H
    block = rng.normal(size=(F.VF_COUNT, N)).astype(f32)
    block[F.VF_OBJ_ANGLE] = rng.uniform(-0.6, 0.6, size=N)
    state = np.broadcast_to(block, (T,) + block.shape)       # only the first frame reads the target's words: the anchor
    obs = np.zeros((T, N, 28), dtype=f32)
    progress = np.broadcast_to(np.arange(T)[:, None], (T, N))
    behind = env_target.target_replay(spec, 42, np.arange(N), layout, state, obs, progress, np.zeros((T, N), dtype=np.int64))
    at = behind[T0 - 1]
    plan = mpc_track.plan_replay(mode, "exact", CDT, H, at["state"], at["motion"], at["table"], at["fresh"], np.zeros(N, dtype=np.int64))
    moving = at["moving"]
    assert np.array_equal(plan["live"], moving.astype(np.uint8)) and 0 < moving.sum()
    assert mode == abi.TARGET_FREE or moving.sum() < N          # with an obstacle the plants that drew VEL_ALONG 0 rest
    reflections = 0
    for k in range(H):
        words = behind[T0 - 1 + k]["state"][[F.VF_TARGET_Y, F.VF_TARGET_Z, F.VF_OBJ_DEPTH]].T
        assert np.array_equal(bits(plan["path"][:, k]), bits(words)), k
        if k:
            assert np.array_equal(plan["reflected"][:, k], behind[T0 - 1 + k]["reflected"]), k
            reflections += int(behind[T0 - 1 + k]["reflected"].sum())
    assert reflections >= 2 * moving.sum()                   # |VEL| = 0.4 over a span of 0.02 .. 0.03 turns every few steps
    linear = mpc_track.plan_replay(mode, "linear", CDT, H, at["state"], at["motion"], at["table"], at["fresh"], np.zeros(N, dtype=np.int64))
    for p in range(N):
        turn = int(np.argmax(plan["reflected"][p])) if plan["reflected"][p].any() else H
        assert np.array_equal(bits(linear["path"][p, :turn]), bits(plan["path"][p, :turn])), p
        assert turn == H or not np.array_equal(bits(linear["path"][p, turn]), bits(plan["path"][p, turn])), p


def test_node_replay_on_hand_made_rows():
    M, K, H = 3, 4, 5
    N = M * K
    rng = np.random.default_rng(9)
    state = rng.normal(size=(F.VF_COUNT, N)).astype(f32)
    path = rng.normal(size=(M, H, 3)).astype(f32)
    live = np.uint8([1, 0, 1])
    alive = np.ones(N, dtype=np.uint8)
    alive[[1, 9]] = 0                                        # a dead sample of a live plant each
    written = {abi.TARGET_FREE: [F.VF_TARGET_Y, F.VF_TARGET_Z], abi.TARGET_SHELF: [F.VF_TARGET_Y, F.VF_OBJ_DEPTH],
               abi.TARGET_PIPE: [F.VF_TARGET_Y, F.VF_TARGET_Z, F.VF_OBJ_DEPTH]}
    word_of = {F.VF_TARGET_Y: 0, F.VF_TARGET_Z: 1, F.VF_OBJ_DEPTH: 2}
    for mode in MODES:
        for k in (-3, 0, H, H + 1, 1 << 40):                 # outside 1 .. H - 1: nothing
            assert np.array_equal(bits(mpc_track.node_replay(mode, K, k, state, alive, path, live)), bits(state)), (mode, k)
        for k in range(1, H):
            before = state.copy()
            out = mpc_track.node_replay(mode, K, k, state, alive, path, live)
            assert np.array_equal(bits(state), bits(before)) and out is not state
            for e in range(N):
                p = e // K
                for field in range(F.VF_COUNT):
                    if live[p] and alive[e] and field in written[mode]:
                        assert bits(out[field, e]) == bits(path[p, k, word_of[field]]), (mode, k, e, field)
                    else:
                        assert bits(out[field, e]) == bits(state[field, e]), (mode, k, e, field)
    assert np.array_equal(bits(mpc_track.node_replay(abi.TARGET_PIPE, K, 2, state, alive, path, np.zeros(M, dtype=np.uint8))), bits(state))
    assert np.array_equal(bits(mpc_track.node_replay(abi.TARGET_PIPE, K, 2, state, np.zeros(N, dtype=np.uint8), path, live)), bits(state))
    one = path[:, :1]                                        # H = 1: no k lies in 1 .. 0
    for k in (0, 1, 2):
        assert np.array_equal(bits(mpc_track.node_replay(abi.TARGET_FREE, K, k, state, alive, one, live)), bits(state))
