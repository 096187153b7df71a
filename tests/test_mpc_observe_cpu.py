"""MPC_OBSERVE without a GPU: the C ABI of include/vine_mpc_observe.h against its ctypes mirror, every refusal of the library
that comes before a launch and every ``ConfigError`` by name, the build plumbing of the fourteenth unit, the purpose words,
and the numpy statements (``catchup_schedule``, ``measure_replay``, ``pin_replay``) on hand-made rows."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_observe
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = abi
RING = slice(F.VF_FIFO0, F.VF_PIPE_Y)
NOT_RING = [f for f in range(F.VF_COUNT) if not F.VF_FIFO0 <= f < F.VF_PIPE_Y]


def _header():
    return open(os.path.join(REPO, "include", "vine_mpc_observe.h")).read()


@pytest.fixture(scope="module")
def hip_lib():
    native.build()
    return native.load()


# (name, handles, an int behind the configuration?, pointer arguments behind it, the stream included)
ENTRY_POINTS = (("vine_mpc_observe_measure", 1, 0, 8), ("vine_mpc_observe_pin", 2, 0, 12), ("vine_mpc_observe_catchup", 2, 1, 12))


def _calls(lib, c, step_index=1):
    return [(name, getattr(lib, name), [None] * handles + [c] + [step_index] * ints + [None] * rest)
            for name, handles, ints, rest in ENTRY_POINTS]


# --------------------------------------------------------------------------------------------------------------- ABI
def test_observe_header_and_ctypes_mirror_agree(hip_lib):
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(vine_mpc_observe_[a-z_0-9]+)\s*\(", code)))
    assert names == sorted(abi.MPC_OBSERVE_PROTOTYPES) and len(names) == 5
    for name in names:
        assert hasattr(hip_lib, name), name
    assert hip_lib.vine_mpc_observe_config_size() == C.sizeof(abi.VineMpcObserveConfig) == 4 * 4 + 8
    body = re.search(r"typedef struct VineMpcObserveConfig \{(.*?)\} VineMpcObserveConfig;", code, re.S).group(1)
    fields = re.findall(r"^\s+(?:int32_t|uint64_t)\s+([a-z_]+);", body, re.M)
    assert fields == [n for n, _ in abi.VineMpcObserveConfig._fields_]
    for macro, value in (("ABI_VERSION", abi.MPC_OBSERVE_ABI_VERSION), ("THREADS", abi.MPC_OBSERVE_THREADS),
                         ("RNG_NOISE", abi.MPC_OBSERVE_RNG_NOISE), ("RNG_HOLD", abi.MPC_OBSERVE_RNG_HOLD)):
        assert int(re.search(r"#define VINE_MPC_OBSERVE_%s (\d+)" % macro, text).group(1)) == value
    assert "#define VINE_MPC_OBSERVE_SLOTS (VINE_MAX_DELAY + 1)" in text and abi.MPC_OBSERVE_SLOTS == abi.MAX_DELAY + 1 == 9
    assert "#define VINE_MPC_OBSERVE_LOG (2 * VINE_MAX_DELAY)" in text and abi.MPC_OBSERVE_LOG == 2 * abi.MAX_DELAY == 16
    slots = re.search(r"typedef enum VineMpcObserveSlot \{(.*?)\}", code, re.S).group(1)
    assert [w.split("=")[0].strip() for w in slots.split(",")] == ["VMO_" + n for n in abi.MPC_OBSERVE_NAMES] + ["VMO_NAMES"]
    assert (abi.VMO_DELAY, abi.VMO_HOLD, abi.VMO_NOISE_Q, abi.VMO_NOISE_QD, abi.VMO_NAMES) == (0, 1, 2, 3, 4)
    for name, handles, ints, rest in ENTRY_POINTS:
        decl = re.search(r"int %s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(abi.MPC_OBSERVE_PROTOTYPES[name][1]) == handles + 1 + ints + rest, name
    for other in ("vine.h", "vine_mpc.h", "vine_mpc_adapt.h"):
        assert "vine_mpc_observe" not in open(os.path.join(REPO, "include", other)).read(), other
    assert not set(abi.MPC_OBSERVE_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.MPC_PROTOTYPES) | set(abi.MPC_ADAPT_PROTOTYPES)
                                                 | set(abi.MPC_POLICY_PROTOTYPES))


def test_observe_defaults(hip_lib):
    c = abi.VineMpcObserveConfig()
    c.catchup, c.seed = 5, 9
    assert hip_lib.vine_mpc_observe_config_default(c) == abi.OK
    assert (c.abi_version, c.num_plants, c.catchup, c.compensate, c.seed) == (1, 0, 0, 1, 0)
    assert hip_lib.vine_mpc_observe_config_default(None) == abi.ERR_INVALID_ARG
    assert b"config is NULL" in hip_lib.vine_last_error()


def test_purpose_words_are_the_next_free_ones():
    taken = (1, 2, 3, 4, abi.SENSOR_RNG_NOISE, abi.SENSOR_RNG_HOLD, 7, abi.MPC_RNG_NOISE, abi.MPC_ADAPT_RNG)
    assert sorted(taken) == list(range(1, 10))
    assert (abi.MPC_OBSERVE_RNG_NOISE, abi.MPC_OBSERVE_RNG_HOLD) == (10, 11)
    assert not {abi.MPC_OBSERVE_RNG_NOISE, abi.MPC_OBSERVE_RNG_HOLD} & set(taken)
    assert "Purpose words 10 and 11" in _header()
    csrc = os.path.join(REPO, "vine_robot_isaacgymenvs_amd", "csrc")
    for name in sorted(os.listdir(csrc)):                       # nobody else draws from these two streams
        if name != "vine_mpc_observe.hip":
            source = open(os.path.join(csrc, name)).read()
            assert "VINE_MPC_OBSERVE_RNG" not in source and not re.search(r"RNG\w*\s*=?\s*1[01]u?\b", source), name


def test_observe_build_plumbing():
    assert native.POLICY_UNITS == native.LIB_UNITS + (native.SRC_MPC_POLICY,) and len(native.POLICY_UNITS) == 13     # still pinned
    assert "for src in POLICY_UNITS" in inspect.getsource(native.build)                                              # ... and this
    assert "for src in POLICY_UNITS + (SRC_MPC_OBSERVE,)" in inspect.getsource(native.build)
    assert native.SRC_MPC_OBSERVE not in native.POLICY_UNITS
    assert os.path.basename(native.SRC_MPC_OBSERVE) == "vine_mpc_observe.hip" and os.path.exists(native.SRC_MPC_OBSERVE)
    deps = [os.path.basename(d) for d in native.DEPS]
    for name in ("vine_mpc_observe.hip", "vine_mpc_observe.h", "vine_mpc_shared.h", "vine_policy_head.h", "vine_task_shared.h"):
        assert name in deps, name
    headers = [os.path.basename(h) for h in native._SOURCE_HEADERS[native.SRC_MPC_OBSERVE]]
    assert headers == ["vine_mpc_observe.h", "vine_mpc_shared.h"]
    assert native._SOURCE_FLAGS[native.SRC_MPC_OBSERVE] == ["-ffp-contract=fast-honor-pragmas"]
    flags = native._flags(native.SRC_MPC_OBSERVE)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast")
    src = open(native.SRC_MPC_OBSERVE).read()
    assert src.index("#pragma clang fp contract(off)") < src.index("#include")
    # contraction is on again exactly around the command map and the tip's forward kinematics
    on = src.index("#pragma clang fp contract(fast)")
    off_again = src.index("#pragma clang fp contract(off)", on)
    assert [line for line in src[on:off_again].splitlines()[1:] if line.strip()] == ['#include "vine_task_shared.h"']
    assert src.index('#include "vine_mpc_shared.h"') > off_again
    for word in ("tip_fk_joint(", "MPC_COPY_COLUMN(", "mpc_rebuild_ring(", "mpc_deviate_int("):
        assert word in src, word
    assert "task_new_command<false>" in open(os.path.join(os.path.dirname(native.SRC_MPC_OBSERVE), "vine_mpc_shared.h")).read()
    assert "atomic" not in re.sub(r"//.*", "", src) and "__shared__" not in src


# ------------------------------------------------------------------------------------------------- the library's refusals
@pytest.mark.parametrize("over, word", [
    (dict(abi_version=7), b"VineMpcObserveConfig.abi_version"), (dict(num_plants=0), b"num_plants"),
    (dict(catchup=-1), b"catchup"), (dict(catchup=abi.MAX_DELAY + 1), b"catchup"), (dict(compensate=2), b"compensate"),
    (dict(compensate=-1), b"compensate")])
def test_observe_refuses_bad_configs(hip_lib, over, word):
    """Validation comes before the handles or any pointer is looked at, so no device is needed to see it."""
    c = mpc_observe.observe_cconfig(3, 2)
    for k, v in over.items():
        setattr(c, k, v)
    for name, fn, args in _calls(hip_lib, c):
        hip_lib.vine_set_step_count(None, -1)             # leaves another message behind
        assert fn(*args) == abi.ERR_INVALID_ARG, name
        assert word in hip_lib.vine_last_error(), hip_lib.vine_last_error()


def test_observe_refuses_null_pointers_null_configs_and_step_indices(hip_lib):
    c = mpc_observe.observe_cconfig(3, 2)
    for name, fn, args in _calls(hip_lib, c):
        assert fn(*args) == abi.ERR_INVALID_ARG
        assert b"null argument to " + name.encode() in hip_lib.vine_last_error(), hip_lib.vine_last_error()
    for name, fn, args in _calls(hip_lib, None):
        assert fn(*args) == abi.ERR_INVALID_ARG and b"mpc observe config is NULL" in hip_lib.vine_last_error()
    # past the null checks and still in front of the handles: host memory stands in for the buffers (nothing is read)
    buf = (C.c_char * 256)()
    base = (C.addressof(buf) + 15) // 16 * 16
    h1, h2, p, odd4 = base, base + 64, base + 16, base + 20
    lib = hip_lib

    def refused(fn, args, word):
        lib.vine_set_step_count(None, -1)
        assert fn(*args) == abi.ERR_INVALID_ARG
        assert word in lib.vine_last_error(), lib.vine_last_error()

    for i in (0, 3, -1):
        refused(lib.vine_mpc_observe_catchup, [h1, h2, c, i] + [p] * 11 + [None], b"1 <= step_index <= catchup")
    refused(lib.vine_mpc_observe_pin, [h1, h1, c] + [p] * 11 + [None], b"two handles")
    refused(lib.vine_mpc_observe_catchup, [h1, h1, c, 1] + [p] * 11 + [None], b"two handles")
    refused(lib.vine_mpc_observe_pin, [h1, h2, c, p, p, p, odd4, p, p, p, p, p, p, p, None], b"8-byte aligned")
    refused(lib.vine_mpc_observe_pin, [h1, h2, c, p, p, p, p, p, p, odd4, p, p, p, p, None], b"8-byte aligned")
    refused(lib.vine_mpc_observe_measure, [h1, c, p, p, odd4, p, p, p, p, None], b"8-byte aligned")
    refused(lib.vine_mpc_observe_measure, [h1, c, p, p, p, p, odd4, p, p, None], b"8-byte aligned")


# ------------------------------------------------------------------------------------------------------ the configuration
def test_observe_config_fills_the_defaults_and_the_mirror():
    spec = mpc_observe.observe_config({"DELAY": {"values": [0, 1, 3]}, "HOLD": 0.3, "NOISE_Q": [0.0, 0.01]})
    assert spec == {"DELAY": {"values": [0.0, 1.0, 3.0]}, "HOLD": 0.3, "NOISE_Q": [0.0, 0.01], "NOISE_QD": 0.0,
                    "COMPENSATE": True, "CATCHUP": 3}
    assert mpc_observe.observe_config({})["CATCHUP"] == 0
    assert mpc_observe.observe_config({"DELAY": 2, "CATCHUP": 5, "COMPENSATE": False})["CATCHUP"] == 5
    table = mpc_observe.draw_observe(spec, 7, np.arange(7))
    assert table.shape == (4, 7) and table.dtype == np.float64
    assert list(table[0]) == [0, 1, 3, 0, 1, 3, 0] and np.all(table[1] == 0.3) and not table[3].any()
    assert np.all((table[2] >= 0) & (table[2] <= 0.01)) and len(set(table[2])) == 7
    assert np.array_equal(table, mpc_observe.draw_observe(spec, 7, np.arange(7)))          # a pure function
    c = mpc_observe.observe_cconfig(7, 3, False, 2 ** 40 + 5, table)
    assert (c.abi_version, c.num_plants, c.catchup, c.compensate, c.seed) == (abi.MPC_OBSERVE_ABI_VERSION, 7, 3, 0, 2 ** 40 + 5)


@pytest.mark.parametrize("spec, word", [
    (5, "must be a mapping"), ({"LATENCY": 1}, "unknown key(s) LATENCY"), ({"DELAY": 1.5}, "observe.DELAY"),
    ({"DELAY": 9}, "observe.DELAY"), ({"DELAY": -1}, "observe.DELAY"), ({"DELAY": [3, 1]}, "observe.DELAY"),
    ({"DELAY": {"values": []}}, "observe.DELAY"), ({"DELAY": {"vals": [1]}}, "observe.DELAY"), ({"DELAY": "x"}, "observe.DELAY"),
    ({"HOLD": 1.0}, "observe.HOLD"), ({"HOLD": -0.1}, "observe.HOLD"), ({"HOLD": float("nan")}, "observe.HOLD"),
    ({"NOISE_Q": -1e-3}, "observe.NOISE_Q"), ({"NOISE_Q": float("inf")}, "observe.NOISE_Q"), ({"NOISE_QD": [0, -1]}, "observe.NOISE_QD"),
    ({"NOISE_QD": {"values": [0.1, -0.1]}}, "observe.NOISE_QD"), ({"COMPENSATE": 1}, "observe.COMPENSATE"),
    ({"CATCHUP": 9}, "observe.CATCHUP"), ({"CATCHUP": 2.0}, "observe.CATCHUP"), ({"CATCHUP": True}, "observe.CATCHUP"),
    ({"DELAY": [1, 4], "CATCHUP": 3}, "below the largest DELAY")])
def test_observe_config_errors_name_the_key(spec, word):
    with pytest.raises(ConfigError, match=re.escape(word)):
        mpc_observe.observe_config(spec)


@pytest.mark.parametrize("kw, word", [
    (dict(num_plants=0), "plants"), (dict(num_plants=2.0), "plants"), (dict(catchup=-1), "catchup"), (dict(catchup=9), "catchup"),
    (dict(catchup=True), "catchup"), (dict(compensate=1), "compensate"), (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"),
    (dict(catchup=2, table=np.float32([[0, 3, 1]] + [[0, 0, 0]] * 3)), "below the table's largest DELAY"),
    (dict(table=np.zeros((3, 3))), "the table must be")])
def test_observe_cconfig_errors_name_the_key(kw, word):
    args = dict(num_plants=3)
    args.update(kw)
    with pytest.raises(ConfigError, match=re.escape(word)):
        mpc_observe.observe_cconfig(**args)


def test_play_refuses_observe_with_adapt_and_with_policy():
    cfg = {"env": {"numEnvs": 2}, "seed": 0}
    # refused before any task is created (no device needed)
    with pytest.raises(ConfigError, match="observe= together with adapt= is refused"):
        mpc.play(cfg, samples=16, observe={"DELAY": 1}, adapt={"params": {"DAMPING": [0.005, 0.1]}})
    with pytest.raises(ConfigError, match="observe= together with policy= is refused"):
        mpc.play(cfg, samples=256, observe={"DELAY": 1}, policy="x.pth", policy_params={})
    with pytest.raises(ConfigError, match="mpc: observe.HOLD"):
        mpc.play(cfg, samples=16, observe={"HOLD": 2.0})
    assert "observe" in inspect.signature(mpc.play).parameters and inspect.signature(mpc.play).parameters["observe"].default is None


# ------------------------------------------------------------------------------------------------- the numpy statements
def test_catchup_schedule_on_hand_made_pairs():
    sched = mpc_observe.catchup_schedule
    # d = 0: every step is pinned again, every action is zero
    assert sched(3, 0) == [dict(i=0, pinned=True, real=False, action=None), dict(i=1, pinned=True, real=False, action=None),
                           dict(i=2, pinned=True, real=False, action=None), dict(i=3, pinned=True, real=False, action="none")]
    # d = C: only the pin pins; the actions run from the oldest, act_log[C - 1], to the newest, act_log[0]
    assert sched(3, 3) == [dict(i=0, pinned=True, real=False, action=2), dict(i=1, pinned=False, real=True, action=1),
                           dict(i=2, pinned=False, real=True, action=0), dict(i=3, pinned=False, real=True, action="none")]
    # in between: the real steps are the last d
    assert sched(3, 1) == [dict(i=0, pinned=True, real=False, action=None), dict(i=1, pinned=True, real=False, action=None),
                           dict(i=2, pinned=True, real=False, action=0), dict(i=3, pinned=False, real=True, action="none")]
    assert sched(0, 0) == [dict(i=0, pinned=True, real=False, action="none")]
    for C in range(abi.MAX_DELAY + 1):
        for d in range(C + 1):
            rows = sched(C, d)
            assert sum(r["real"] for r in rows) == d and rows[0]["pinned"]
            assert [r["action"] for r in rows if isinstance(r["action"], int)] == list(range(d - 1, -1, -1))
            assert [r["i"] for r in rows if r["pinned"]] == list(range(C - d + 1))      # the last pin stands in front of the real steps
    with pytest.raises(ValueError):
        sched(2, 3)


def _columns(T, M, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(T, F.VF_COUNT, M)).astype(np.float32)


def test_measure_replay_first_frame_fills_every_slot_a_held_frame_repeats_and_age_saturates():
    M, T = 2, 13
    cols = _columns(T, M)
    acts = np.arange(T * M * 2, dtype=np.float32).reshape(T, M, 2)
    progress = np.tile(np.arange(T)[:, None], (1, M))
    progress[:, 1] = [0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7, 8]           # plant 1 consumes a reset in step 4
    table = np.float32([[3, 3], [0.0, 0.0], [0, 0], [0, 0]])
    sentinel = np.full((abi.MPC_OBSERVE_SLOTS, F.VF_COUNT, M), -7777.0, dtype=np.float32)
    out = mpc_observe.measure_replay(table, 5, np.arange(T), cols, progress, acts, state={"snap": sentinel})
    assert len(out) == T
    first = out[0]
    assert first["first"].all() and not first["held"].any() and not first["fresh"].any() and not first["age"].any()
    for k in range(abi.MPC_OBSERVE_SLOTS):                              # the first frame fills every slot; the ring fields never
        assert np.array_equal(first["snap"][k][NOT_RING], cols[0][NOT_RING])
        assert np.all(first["snap"][k][RING] == -7777.0)
    for t in range(1, T):
        o = out[t]
        assert np.array_equal(o["snap"][t % 9][NOT_RING][:, 0], cols[t][NOT_RING][:, 0])
        assert np.array_equal(o["snap"][(t - 1) % 9][:, 0], out[t - 1]["snap"][(t - 1) % 9][:, 0])      # the others stand
        assert np.all(o["snap"][:, RING] == -7777.0)
        assert np.array_equal(o["act_log"][:, 0], acts[t]) and np.array_equal(o["act_log"][:, 1:], out[t - 1]["act_log"][:, :-1])
    assert [int(o["age"][0]) for o in out] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 8, 8, 8]          # saturates at MAX_DELAY
    assert [int(o["age"][1]) for o in out] == [0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert [bool(o["first"][1]) for o in out] == [True, False, False, False, True] + [False] * 8
    for k in range(abi.MPC_OBSERVE_SLOTS):                              # no frame of the earlier episode is left
        assert np.array_equal(out[4]["snap"][k][NOT_RING][:, 1], cols[4][NOT_RING][:, 1])
    assert np.array_equal(out[-1]["act_log"][0, :, :], acts[::-1][:, 0][:16][:13].tolist() + [[0, 0]] * 3)
    # HOLD close to 1: every frame but the first repeats the first; external resets start anew and clear the log
    held = mpc_observe.measure_replay(np.float32([[0, 0], [0.999999, 0.999999], [0, 0], [0, 0]]), 5, np.arange(T), cols, progress,
                                      acts, external_resets=[[]] * 7 + [[0]] + [[]] * 5)
    assert all(o["held"][0] for o in held[1:7]) and not held[7]["held"][0] and held[7]["first"][0]
    for t in range(1, 7):
        assert np.array_equal(held[t]["snap"][t % 9][NOT_RING][:, 0], cols[0][NOT_RING][:, 0])
    assert np.array_equal(held[8]["snap"][8][NOT_RING][:, 0], cols[7][NOT_RING][:, 0])
    assert np.array_equal(held[7]["act_log"][0, 0], acts[7, 0]) and not held[7]["act_log"][0, 1:].any()
    assert held[7]["act_log"][1, 1:].any()


def test_measure_replay_noise_is_one_multiply_one_add_and_the_derived_fields_follow():
    M = 3
    cols = _columns(1, M, seed=2)
    table = np.float32([[0, 0, 0], [0, 0, 0], [0.01, 0.0, 0.0], [0.0, 0.0, 0.05]])
    tip = lambda q, qd, plants: mpc_observe.fk64(q, qd, 0.0885, 0.965, 3.1415)          # noqa: E731
    o = mpc_observe.measure_replay(table, 11, [41], cols, np.ones((1, M)), np.zeros((1, M, 2)), tip=tip,
                                   state={"fresh": np.zeros(M)})[0]
    frame = o["frame"]
    assert np.array_equal(frame[:, 1], cols[0][:, 1])                   # a noise-free plant keeps the column's own bits
    z = mpc_observe.noise_deviate(11, [0, 2], 41, np.arange(12))
    assert z.dtype == np.float32 and np.all(z == np.round(z)) and np.abs(z).max() < 524281
    cq = np.float32(np.float64(np.float32(0.01)) * mpc_observe.NOISE_SCALE)
    cqd = np.float32(np.float64(np.float32(0.05)) * mpc_observe.NOISE_SCALE)
    assert np.array_equal(frame[F.VF_Q0:F.VF_Q0 + 6, 0], cols[0][F.VF_Q0:F.VF_Q0 + 6, 0] + z[0, :6] * cq)
    assert np.array_equal(frame[F.VF_QD0:F.VF_QD0 + 6, 0], cols[0][F.VF_QD0:F.VF_QD0 + 6, 0])          # NOISE_QD of plant 0 is zero
    assert np.array_equal(frame[F.VF_QD0:F.VF_QD0 + 6, 2], cols[0][F.VF_QD0:F.VF_QD0 + 6, 2] + z[1, 6:] * cqd)
    assert np.array_equal(frame[F.VF_Q0:F.VF_Q0 + 6, 2], cols[0][F.VF_Q0:F.VF_Q0 + 6, 2])
    for p in (0, 2):
        q, qd = frame[F.VF_Q0:F.VF_Q0 + 6, p], frame[F.VF_QD0:F.VF_QD0 + 6, p]
        t = np.float32(mpc_observe.fk64(q[None], qd[None], 0.0885, 0.965, 3.1415))[0]
        assert np.array_equal(frame[F.VF_TIP_Y:F.VF_TIP_VZ + 1, p], t)
        assert frame[F.VF_CART_Y, p] == q[0] and frame[F.VF_CART_VY, p] == qd[0] and frame[F.VF_PREV_CART_VEL, p] == qd[0]
        assert np.array_equal(frame[F.VF_PREV_Q0:F.VF_PREV_Q0 + 6, p], q)
        assert frame[F.VF_PREV_TIP_Y, p] == t[0] and frame[F.VF_PREV_TIP_Z, p] == t[1]
        untouched = [f for f in NOT_RING if f not in list(range(0, 18)) + [F.VF_PREV_CART_VEL] + list(range(F.VF_PREV_Q0, F.VF_FIFO0))]
        assert np.array_equal(frame[untouched, p], cols[0][untouched, p])      # the controller's own memories, the poses
    with pytest.raises(ValueError, match="needs tip"):
        mpc_observe.measure_replay(table, 11, [41], cols, np.ones((1, M)), np.zeros((1, M, 2)))
    # the two streams are the two purpose words: another word, other numbers
    u = mpc_observe.hold_uniform(11, np.arange(4), 41)
    assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1)) and len(set(u)) == 4


def test_pin_replay_on_hand_made_rows():
    M, C = 4, 3
    cols = _columns(6, M, seed=3)
    acts = (1 + np.arange(6 * M * 2, dtype=np.float32)).reshape(6, M, 2)
    progress = np.tile(np.arange(6)[:, None], (1, M))
    progress[:, 3] = [0, 1, 2, 3, 0, 1]                                  # plant 3 is one step into its episode
    table = np.float32([[0, 1, 3, 3], [0] * 4, [0] * 4, [0] * 4])
    state = mpc_observe.measure_replay(table, 1, np.arange(6), cols, progress, acts)[-1]
    assert list(state["age"]) == [5, 5, 5, 1]
    plant_now = cols[5]
    pin = mpc_observe.pin_replay(table, state, plant_now, progress[5], 6, C, True)
    assert list(pin["lag"]) == [0, 1, 3, 1] and list(pin["behind"]) == [0, 1, 3, 1] and pin["pinned"].all()
    for p, t in enumerate((5, 4, 2, 4)):                                 # the frame of step s - d
        assert np.array_equal(pin["column"][NOT_RING][:, p], cols[t][NOT_RING][:, p])
    assert list(pin["progress"]) == [5, 4, 2, 0]
    log = state["act_log"]
    assert np.array_equal(log[:, :6], acts[::-1].transpose(1, 0, 2))
    for p, d in enumerate((0, 1, 3, 1)):
        assert np.array_equal(pin["ring_history"][p], log[p, d:d + 8])
    assert np.array_equal(pin["actions"], [[0, 0], [0, 0], log[2, 2], [0, 0]]) and pin["writes_action"]
    node1 = mpc_observe.pin_replay(table, state, plant_now, progress[5], 6, C, True, step_index=1)
    assert list(node1["pinned"]) == [True, True, False, True] and np.array_equal(node1["actions"][2], log[2, 1])
    node2 = mpc_observe.pin_replay(table, state, plant_now, progress[5], 6, C, True, step_index=2)
    assert list(node2["pinned"]) == [True, True, False, True]
    assert np.array_equal(node2["actions"], [[0, 0], log[1, 0], log[2, 0], log[3, 0]])
    node3 = mpc_observe.pin_replay(table, state, plant_now, progress[5], 6, C, True, step_index=3)
    assert list(node3["pinned"]) == [True, False, False, False] and not node3["writes_action"]
    # not compensated: the stale frame is still what is delivered, and nothing is replayed
    off = mpc_observe.pin_replay(table, state, plant_now, progress[5], 6, C, False)
    assert not off["lag"].any() and list(off["behind"]) == [0, 1, 3, 1] and np.array_equal(off["column"], pin["column"])
    assert list(off["progress"]) == [5, 4, 2, 0] and not off["actions"].any()
    assert np.array_equal(off["ring_history"], log[:, :8])
    # nothing measured yet: the plant's own column, lag 0
    fresh = dict(state, fresh=np.uint8([0, 0, 1, 0]))
    known = mpc_observe.pin_replay(table, fresh, plant_now, progress[5], 6, C, True)
    assert list(known["lag"]) == [0, 1, 0, 1] and np.array_equal(known["column"][NOT_RING][:, 2], plant_now[NOT_RING][:, 2])
    assert not mpc_observe.pin_replay(table, state, plant_now, progress[5], 0, C, True)["lag"].any()
