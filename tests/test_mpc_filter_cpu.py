"""MPC_FILTER without a GPU: the C ABI of include/vine_mpc_filter.h against its ctypes mirror, every refusal of the library
that comes before a launch (those that need a handle through the stand-alone scripts/mpc_filter_host_check.cpp, built with
the host's sanitizers) and every ``ConfigError`` by name, the build plumbing of the fifteenth unit, and the two numpy
statements (``filter_pin_replay``, ``filter_correct_replay``) on hand-made rows, every case of the correction among them."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_filter, mpc_observe
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = abi
SLOTS, LOG = abi.MPC_OBSERVE_SLOTS, abi.MPC_OBSERVE_LOG
RING = slice(F.VF_FIFO0, F.VF_PIPE_Y)
NOT_RING = [f for f in range(F.VF_COUNT) if not F.VF_FIFO0 <= f < F.VF_PIPE_Y]
JOINTS = list(range(12))
DERIVED = ([F.VF_TIP_Y, F.VF_TIP_Z, F.VF_TIP_VY, F.VF_TIP_VZ, F.VF_CART_Y, F.VF_CART_VY] + list(range(F.VF_PREV_Q0, F.VF_PREV_Q0 + 6))
           + [F.VF_PREV_TIP_Y, F.VF_PREV_TIP_Z, F.VF_PREV_CART_VEL])
RECORDED = [f for f in NOT_RING if f not in JOINTS + DERIVED]      # the controller's memories, target and obstacle poses


def _header():
    return open(os.path.join(REPO, "include", "vine_mpc_filter.h")).read()


@pytest.fixture(scope="module")
def hip_lib():
    native.build()
    return native.load()


# (name, pointer arguments behind the two handles and the configuration, the stream included)
ENTRY_POINTS = (("vine_mpc_filter_pin", 12), ("vine_mpc_filter_correct", 9))


# --------------------------------------------------------------------------------------------------------------- ABI
def test_filter_header_and_ctypes_mirror_agree(hip_lib):
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(vine_mpc_filter_[a-z_0-9]+)\s*\(", code)))
    assert names == sorted(abi.MPC_FILTER_PROTOTYPES) and len(names) == 3
    for name in names:
        assert hasattr(hip_lib, name), name
    assert hip_lib.vine_mpc_filter_abi_version() == abi.MPC_FILTER_ABI_VERSION == 1
    for macro, value in (("ABI_VERSION", abi.MPC_FILTER_ABI_VERSION), ("THREADS", abi.MPC_FILTER_THREADS)):
        assert int(re.search(r"#define VINE_MPC_FILTER_%s (\d+)" % macro, text).group(1)) == value
    # the filter has no random stream of its own: it reads the measurement's hold draw again
    assert "#define VINE_MPC_FILTER_HOLD_PURPOSE VINE_MPC_OBSERVE_RNG_HOLD" in text
    slots = re.search(r"typedef enum VineMpcFilterSlot \{(.*?)\}", code, re.S).group(1)
    assert [w.split("=")[0].strip() for w in slots.split(",")] == ["VMF_" + n for n in abi.MPC_FILTER_NAMES] + ["VMF_NAMES"]
    assert (abi.VMF_GAIN_Q, abi.VMF_GAIN_QD, abi.VMF_NAMES) == (0, 1, 2) and abi.MPC_FILTER_NAMES == ("GAIN_Q", "GAIN_QD")
    for name, rest in ENTRY_POINTS:
        decl = re.search(r"int %s\((.*?)\);" % name, code, re.S).group(1)
        assert len(decl.split(",")) == len(abi.MPC_FILTER_PROTOTYPES[name][1]) == 3 + rest, name
    for other in ("vine.h", "vine_mpc.h", "vine_mpc_adapt.h", "vine_mpc_observe.h"):
        assert "vine_mpc_filter" not in open(os.path.join(REPO, "include", other)).read(), other
    assert not set(abi.MPC_FILTER_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.MPC_PROTOTYPES) | set(abi.MPC_OBSERVE_PROTOTYPES))
    assert "declare_mpc_filter" in inspect.getsource(abi.declare_all)


def test_filter_build_plumbing():
    assert "for src in POLICY_UNITS + (SRC_MPC_OBSERVE,) + (SRC_MPC_FILTER,)" in inspect.getsource(native.build)
    assert native.SRC_MPC_FILTER not in native.POLICY_UNITS
    assert os.path.basename(native.SRC_MPC_FILTER) == "vine_mpc_filter.hip" and os.path.exists(native.SRC_MPC_FILTER)
    deps = [os.path.basename(d) for d in native.DEPS]
    for name in ("vine_mpc_filter.hip", "vine_mpc_filter.h", "vine_mpc_observe.h", "vine_mpc_shared.h", "vine_task_shared.h"):
        assert name in deps, name
    headers = [os.path.basename(h) for h in native._SOURCE_HEADERS[native.SRC_MPC_FILTER]]
    assert headers == ["vine_mpc_observe.h", "vine_mpc_filter.h", "vine_mpc_shared.h"]
    assert native._SOURCE_FLAGS[native.SRC_MPC_FILTER] == ["-ffp-contract=fast-honor-pragmas"]
    flags = native._flags(native.SRC_MPC_FILTER)
    assert flags.index("-ffp-contract=fast-honor-pragmas") > flags.index("-ffp-contract=fast")
    src = open(native.SRC_MPC_FILTER).read()
    assert src.index("#pragma clang fp contract(off)") < src.index("#include")
    # contraction is on again exactly around the command map and the tip's forward kinematics
    on = src.index("#pragma clang fp contract(fast)")
    off_again = src.index("#pragma clang fp contract(off)", on)
    assert [line for line in src[on:off_again].splitlines()[1:] if line.strip()] == ['#include "vine_task_shared.h"']
    assert src.index('#include "vine_mpc_shared.h"') > off_again
    for word in ("tip_fk_joint(", "MPC_COPY_COLUMN(", "mpc_rebuild_ring(", "VINE_MPC_FILTER_HOLD_PURPOSE"):
        assert word in src, word
    code = re.sub(r"//.*", "", src)
    assert "task_new_command" not in code and "#define MPC_COPY_COLUMN" not in code and "sincosf" not in code      # used, not restated
    assert "atomic" not in code and "__shared__" not in src
    # nothing of the units the filter rides on was touched to make room for it
    assert "filter" not in open(native.SRC_MPC_OBSERVE).read().lower()


# ------------------------------------------------------------------------------------------------- the library's refusals
@pytest.mark.parametrize("over, word", [(dict(abi_version=7), b"mpc filter: VineMpcObserveConfig.abi_version"),
                                        (dict(num_plants=0), b"mpc filter: num_plants")])
def test_filter_refuses_bad_configs(hip_lib, over, word):
    """Validation comes before the handles or any pointer is looked at, so no device is needed to see it."""
    c = mpc_observe.observe_cconfig(3, 2)
    for k, v in over.items():
        setattr(c, k, v)
    for name, rest in ENTRY_POINTS:
        hip_lib.vine_set_step_count(None, -1)             # leaves another message behind
        assert getattr(hip_lib, name)(None, None, c, *[None] * rest) == abi.ERR_INVALID_ARG, name
        assert word in hip_lib.vine_last_error(), hip_lib.vine_last_error()


def test_filter_refuses_null_pointers_null_configs_and_misaligned_buffers(hip_lib):
    lib, c = hip_lib, mpc_observe.observe_cconfig(3, 2)
    for name, rest in ENTRY_POINTS:
        assert getattr(lib, name)(None, None, c, *[None] * rest) == abi.ERR_INVALID_ARG
        assert b"null argument to " + name.encode() in lib.vine_last_error(), lib.vine_last_error()
        assert getattr(lib, name)(None, None, None, *[None] * rest) == abi.ERR_INVALID_ARG
        assert b"mpc filter: the observe config is NULL" in lib.vine_last_error()
    # past the null checks and still in front of the handles: host memory stands in for the buffers (nothing is read)
    buf = (C.c_char * 256)()
    base = (C.addressof(buf) + 15) // 16 * 16
    h1, h2, p, odd4 = base, base + 64, base + 16, base + 20

    def refused(fn, args, word):
        lib.vine_set_step_count(None, -1)
        assert fn(*args) == abi.ERR_INVALID_ARG
        assert word in lib.vine_last_error(), lib.vine_last_error()

    refused(lib.vine_mpc_filter_pin, [h1, h2, c, p, p, p, p, odd4, p, p, p, p, p, p, None], b"8-byte aligned")      # act_log
    refused(lib.vine_mpc_filter_pin, [h1, h2, c, p, p, p, p, p, p, p, odd4, p, p, p, None], b"8-byte aligned")      # actions
    refused(lib.vine_mpc_filter_pin, [h1, h1, c] + [p] * 11 + [None], b"two handles")
    refused(lib.vine_mpc_filter_correct, [h1, h1, c] + [p] * 8 + [None], b"two handles")


def test_the_refusals_that_need_a_handle_through_the_stand_alone_host_check(tmp_path):
    """scripts/mpc_filter_host_check.cpp, built as its head says -- the unit's HOST code under AddressSanitizer and UBSan, with
    stand-in handles -- walks the plant-count, predictor and device mismatches by name.  A few seconds of hipcc."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "mpc_filter_host_check")
    source = os.path.join(REPO, "scripts", "mpc_filter_host_check.cpp")
    text = open(source).read()
    for word in ("the plant handle does not have num_plants envs", "the predictor handle has 4 envs, not num_plants = 3",
                 "the predictor handle sits on another device", "vine_randomize", "CREATE_SHELF / CREATE_PIPE", "max_episode_length"):
        assert word in text, word
    subprocess.check_call([hipcc, "--offload-arch=" + native.ARCH, "-O1", "-g", "-std=c++17", "-ffp-contract=fast-honor-pragmas",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-x", "hip",
                           source, native.SRC_MPC_FILTER, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "mpc filter host check ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------------ the configuration
def test_filter_config_fills_the_defaults_and_the_draw():
    assert mpc_filter.filter_config({}) == {"GAIN_Q": mpc_filter.DEFAULT_GAIN, "GAIN_QD": mpc_filter.DEFAULT_GAIN}
    spec = mpc_filter.filter_config({"GAIN_Q": {"values": [0, 0.3, 1]}, "GAIN_QD": [0.1, 0.2]})
    assert spec == {"GAIN_Q": {"values": [0.0, 0.3, 1.0]}, "GAIN_QD": [0.1, 0.2]}
    gain = mpc_filter.draw_gains(spec, 7, np.arange(7))
    assert gain.shape == (2, 7) and gain.dtype == np.float64
    assert list(gain[0]) == [0, 0.3, 1, 0, 0.3, 1, 0] and np.all((gain[1] >= 0.1) & (gain[1] <= 0.2)) and len(set(gain[1])) == 7
    assert np.array_equal(gain, mpc_filter.draw_gains(spec, 7, np.arange(7)))              # a pure function
    # keyed by FILTER_<NAME>: not the observe table's numbers under the same seed and ids
    other = mpc_observe.draw_observe(mpc_observe.observe_config({"NOISE_Q": [0.1, 0.2]}), 7, np.arange(7))[abi.VMO_NOISE_Q]
    assert not np.array_equal(gain[1], other)
    both = mpc_filter.draw_gains(mpc_filter.filter_config({"GAIN_Q": {"values": [0.1, 1]}, "GAIN_QD": {"values": [0, 0.5, 1]}}), 0, np.arange(6))
    assert list(both[0]) == [0.1, 1, 0.1, 1, 0.1, 1] and list(both[1]) == [0, 0, 0.5, 0.5, 1, 1]      # the mixed radix
    assert mpc_filter.DRAW_NAMES == ("FILTER_GAIN_Q", "FILTER_GAIN_QD")
    assert mpc_filter.check_gains(gain, 7).dtype == np.float32


@pytest.mark.parametrize("spec, word", [
    (5, "must be a mapping"), ({"GAIN": 1}, "unknown key(s) GAIN"), ({"GAIN_Q": 1.5}, "filter.GAIN_Q"), ({"GAIN_Q": -0.1}, "filter.GAIN_Q"),
    ({"GAIN_QD": [0.5, 1.2]}, "filter.GAIN_QD"), ({"GAIN_QD": [0.5, 0.2]}, "filter.GAIN_QD"), ({"GAIN_QD": {"values": []}}, "filter.GAIN_QD"),
    ({"GAIN_QD": {"values": [0.1, 2]}}, "filter.GAIN_QD"), ({"GAIN_Q": float("nan")}, "filter.GAIN_Q"), ({"GAIN_Q": "x"}, "filter.GAIN_Q"),
    ({"GAIN_Q": True}, "filter.GAIN_Q")])
def test_filter_config_errors_name_the_key(spec, word):
    with pytest.raises(ConfigError, match=re.escape(word)):
        mpc_filter.filter_config(spec)


def test_gain_table_and_reach_errors_name_the_reason():
    with pytest.raises(ConfigError, match=re.escape("the gain table must be [2, 3]")):
        mpc_filter.check_gains(np.zeros((2, 4)), 3)
    with pytest.raises(ConfigError, match="a gain lies outside"):
        mpc_filter.check_gains(np.float32([[0, 1, 1.5], [0, 0, 0]]), 3)
    observe = mpc_observe.observe_config({"DELAY": {"values": [0, 8]}})
    assert mpc_filter.largest_reach(observe, 7) == 15 == LOG - 1
    with pytest.raises(ConfigError, match="largest observe.DELAY, 8, plus the model's largest ACTION_DELAY, 8, exceeds 15"):
        mpc_filter.largest_reach(observe, 8)
    assert mpc_filter.model_action_delay({"ACTION_DELAY": 2}) == 2 and mpc_filter.model_action_delay({}) == 0
    assert mpc_filter.model_action_delay({"ACTION_DELAY": 2}, {"DAMPING": [0.01, 0.05]}) == 2
    assert mpc_filter.model_action_delay({"ACTION_DELAY": 2}, {"ACTION_DELAY": [0, 8]}) == 8
    assert mpc_filter.model_action_delay({"ACTION_DELAY": 2}, {"ACTION_DELAY": {"values": [1, 5, 3]}}) == 5
    assert mpc_filter.model_action_delay({"ACTION_DELAY": 2}, {"ACTION_DELAY": 4}) == 4


def test_play_refuses_filter_without_observe_with_adapt_with_policy_and_beyond_the_log():
    cfg = {"env": {"numEnvs": 2, "ACTION_DELAY": 1}, "seed": 0}
    # refused before any task is created (no device needed)
    with pytest.raises(ConfigError, match="filter= needs observe="):
        mpc.play(cfg, samples=16, filter={})
    with pytest.raises(ConfigError, match="filter= together with adapt= is refused"):
        mpc.play(cfg, samples=16, observe={"DELAY": 1}, filter={}, adapt={"params": {"DAMPING": [0.005, 0.1]}})
    with pytest.raises(ConfigError, match="filter= together with policy= is refused"):
        mpc.play(cfg, samples=256, observe={"DELAY": 1}, filter={}, policy="x.pth", policy_params={})
    with pytest.raises(ConfigError, match="mpc: filter.GAIN_Q"):
        mpc.play(cfg, samples=16, observe={"DELAY": 1}, filter={"GAIN_Q": 2.0})
    with pytest.raises(ConfigError, match="plus the model's largest ACTION_DELAY, 8, exceeds 15"):
        mpc.play(cfg, samples=16, observe={"DELAY": 8}, filter={}, model_params={"ACTION_DELAY": [0, 8]})
    deep = {"env": {"numEnvs": 2, "ACTION_DELAY": 8}, "seed": 0}
    with pytest.raises(ConfigError, match="largest observe.DELAY, 8, plus the model's largest ACTION_DELAY, 8"):
        mpc.play(deep, samples=16, observe={"DELAY": [0, 8]}, filter={"GAIN_Q": 0.5})
    assert inspect.signature(mpc.play).parameters["filter"].default is None


# ------------------------------------------------------------------------------------------------- the numpy statements
def _columns(T, M, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(T, F.VF_COUNT, M)).astype(np.float32)


def _tip(q, qd, plants):
    return mpc_observe.fk64(q, qd, 0.0885, 0.965, 3.1415)


def test_filter_pin_replay_on_hand_made_rows():
    M = 6
    cols = _columns(3, M, seed=1)
    est = _columns(SLOTS, M, seed=2)
    log = (1 + np.arange(M * LOG * 2, dtype=np.float32)).reshape(M, LOG, 2)
    table = np.float32([[0, 1, 3, 3, 8, 0], [0] * M, [0] * M, [0] * M])
    # plant steps completed 20: s = 19.  plant 0: DELAY 0, e = 19; 1: e = 18; 2: e = 16; 3: age 1, dd = 1, e = 18; 4: DELAY 8,
    # e = 11; 5: fresh -- known
    state = {"act_log": log, "age": np.int32([8, 8, 8, 1, 8, 8]), "fresh": np.uint8([0, 0, 0, 0, 0, 1])}
    index = np.int64([18, 18, 15, 17, 10, 18])
    pin = mpc_filter.filter_pin_replay(table, state, est, index, cols[0], 100 + np.arange(M), 20)
    assert list(pin["behind"]) == [0, 1, 3, 1, 8, 0] and list(pin["e"]) == [19, 18, 16, 18, 11, 19]
    assert list(pin["advancing"]) == [True, False, True, True, True, False]
    for p, slot in ((0, 18 % SLOTS), (2, 15 % SLOTS), (3, 17 % SLOTS), (4, 10 % SLOTS)):            # xhat(e - 1)
        assert np.array_equal(pin["column"][NOT_RING][:, p], est[slot][NOT_RING][:, p])
    assert np.array_equal(pin["column"][NOT_RING][:, 1], est[18 % SLOTS][NOT_RING][:, 1])            # est_index == e: xhat(e)
    assert np.array_equal(pin["column"][NOT_RING][:, 5], cols[0][NOT_RING][:, 5])                    # known: the plant's own
    assert not pin["column"][RING].any()
    assert list(pin["progress"]) == [99, 99, 98, 101, 95, 104]                                        # progress - dd - 1
    assert np.array_equal(pin["actions"], [log[0, 0], [0, 0], log[2, 3], log[3, 1], log[4, 8], [0, 0]])
    for p, dd in enumerate((0, 1, 3, 1)):
        assert np.array_equal(pin["ring_history"][p], log[p, dd + 1:dd + 9])
    # the log's out-of-range entries: with dd = 8 the eighth entry of the history is act_log[p][16], which reads (0, 0)
    assert np.array_equal(pin["ring_history"][4][:7], log[4, 9:16]) and not pin["ring_history"][4][7].any()
    assert pin["ring_history"].shape == (M, F.MAX_DELAY, 2)
    # age 0, no estimate, an estimate of another step, no plant step yet: nobody advances, the plant's own column
    for change, idx in ((dict(age=np.zeros(M, np.int32)), index), ({}, np.full(M, -1)), ({}, index - 7)):
        quiet = mpc_filter.filter_pin_replay(table, dict(state, **change), est, idx, cols[0], np.arange(M), 20)
        assert not quiet["advancing"].any() and not quiet["actions"].any()
        if "age" not in change:
            assert np.array_equal(quiet["column"][NOT_RING], cols[0][NOT_RING])
    zero = mpc_filter.filter_pin_replay(table, state, est, np.full(M, -1), cols[0], np.arange(M), 0)
    assert not zero["advancing"].any() and np.array_equal(zero["column"][NOT_RING], cols[0][NOT_RING])   # e = -1 matches no -1
    # age 0 and est_index == e - 1 (DELAY 0 at an episode's first frame): not advancing
    young = mpc_filter.filter_pin_replay(table, dict(state, age=np.zeros(M, np.int32)), est, np.full(M, 18), cols[0], np.arange(M), 20)
    assert not young["advancing"].any()


def test_filter_correct_replay_takes_every_case():
    M, seed, steps = 9, 5, 20                                            # s = 19
    snap, est, xminus = _columns(SLOTS, M, seed=3), _columns(SLOTS, M, seed=4), _columns(1, M, seed=5)[0]
    u = mpc_observe.hold_uniform(seed, np.arange(M), 19)
    table = np.zeros((4, M), dtype=np.float32)
    table[abi.VMO_HOLD, 3] = np.nextafter(u[3], np.float32(1.0))         # plant 3's frame of step 19 was held
    table[abi.VMO_HOLD, 4] = u[4]                                        # ... plant 4's just was not: u < HOLD is strict
    gain = np.float32([[0.3] * M, [0.25] * M])
    gain[:, 5] = 1.0                                                     # unit
    gain[:, 8] = [1.0, 0.5]                                              # one gain 1 alone is no unit
    snap[19 % SLOTS][JOINTS, 6] = xminus[JOINTS, 6]                      # still: every innovation zero
    xminus[F.VF_QD0 + 2, 6] = snap[19 % SLOTS][F.VF_QD0 + 2, 6] = np.float32(-0.0)
    snap[19 % SLOTS][F.VF_QD0 + 2, 6] = np.float32(0.0)                  # (equal as numbers, other words)
    state = {"snap": snap, "age": np.int32([8, 0, 8, 8, 8, 8, 8, 8, 8]), "fresh": np.uint8([1, 0, 0, 0, 0, 0, 0, 0, 0])}
    index = np.int64([18, 18, 19, 18, 18, 18, 18, 12, 18])
    innov0 = np.full((2, M), -3.0, dtype=np.float32)
    out = mpc_filter.filter_correct_replay(table, gain, seed, state, est, index, innov0, xminus, steps, tip=_tip)
    assert list(out["case"]) == ["known", "first", "same", "held", "blend", "unit", "still", "other", "blend"]
    assert set(out["case"]) == set(mpc_filter.CASES)
    assert list(out["est_index"]) == [-1, 19, 19, 19, 19, 19, 19, 19, 19]
    got, y, slot = out["est"], snap[19 % SLOTS], 19 % SLOTS
    assert np.array_equal(got[:, RING], est[:, RING])                   # the ring fields of a slot are never written
    assert np.array_equal(got[:, :, 0], est[:, :, 0]) and np.array_equal(got[:, :, 2], est[:, :, 2])      # known, same: nothing
    for k in range(SLOTS):                                              # first: the frame into every slot
        assert np.array_equal(got[k][NOT_RING][:, 1], y[NOT_RING][:, 1])
    for p in (3, 4, 5, 6, 7, 8):                                        # the others write slot e mod S alone
        others = [k for k in range(SLOTS) if k != slot]
        assert np.array_equal(got[others][:, :, p], est[others][:, :, p])
    assert np.array_equal(got[slot][NOT_RING][:, 3], xminus[NOT_RING][:, 3])              # held: predicted through, whole
    assert np.array_equal(got[slot][NOT_RING][:, 5], y[NOT_RING][:, 5])                   # unit: the frame, its own bits
    assert np.array_equal(got[slot][NOT_RING][:, 7], y[NOT_RING][:, 7])                   # other: the frame
    # still: the frame's recorded fields, the prediction's own words for the joints and what they determine
    assert np.array_equal(got[slot][RECORDED][:, 6], y[RECORDED][:, 6])
    assert np.array_equal(got[slot][JOINTS + DERIVED][:, 6].view(np.uint32), xminus[JOINTS + DERIVED][:, 6].view(np.uint32))
    assert np.signbit(got[slot][F.VF_QD0 + 2, 6]) and not np.signbit(y[F.VF_QD0 + 2, 6])
    for p, (gq, gqd) in ((4, (0.3, 0.25)), (8, (1.0, 0.5))):           # blend: one subtract, one multiply, one add
        x = xminus[:, p]
        v = y[JOINTS, p] - x[JOINTS]
        g = np.float32([gq] * 6 + [gqd] * 6)
        joint = x[JOINTS] + g * v
        assert joint.dtype == np.float32 and np.array_equal(got[slot][JOINTS, p], joint)
        t = np.float32(mpc_observe.fk64(joint[None, :6], joint[None, 6:], 0.0885, 0.965, 3.1415))[0]
        assert np.array_equal(got[slot][F.VF_TIP_Y:F.VF_TIP_VZ + 1, p], t)
        assert got[slot][F.VF_CART_Y, p] == joint[0] and got[slot][F.VF_CART_VY, p] == joint[6] == got[slot][F.VF_PREV_CART_VEL, p]
        assert np.array_equal(got[slot][F.VF_PREV_Q0:F.VF_PREV_Q0 + 6, p], joint[:6])
        assert got[slot][F.VF_PREV_TIP_Y, p] == t[0] and got[slot][F.VF_PREV_TIP_Z, p] == t[1]
        assert np.array_equal(got[slot][RECORDED][:, p], y[RECORDED][:, p])               # recorded exactly
        sums = [np.float32(0), np.float32(0)]
        for i in range(12):
            sums[i // 6] = np.float32(sums[i // 6] + np.float32(v[i] * v[i]))
        assert np.array_equal(out["innov"][:, p], sums) and np.all(out["innov"][:, p] > 0)
    assert np.array_equal(got[slot][JOINTS[:6], 8], y[JOINTS[:6], 8] - xminus[JOINTS[:6], 8] + xminus[JOINTS[:6], 8])
    innov = out["innov"]
    assert list(innov[:, 0]) == [-3, -3] and list(innov[:, 2]) == [-3, -3] and list(innov[:, 7]) == [-3, -3]      # not written
    assert not innov[:, 1].any() and not innov[:, 3].any() and not innov[:, 6].any()      # first, held, still: zero
    assert np.all(innov[:, 5] > 0)                                      # unit: the innovation is still reported
    # a blended estimate needs the tip; the inputs are left as they were
    with pytest.raises(ValueError, match="needs tip"):
        mpc_filter.filter_correct_replay(table, gain, seed, state, est, index, innov0, xminus, steps)
    assert list(index) == [18, 18, 19, 18, 18, 18, 18, 12, 18] and np.all(innov0 == -3.0)
    # no plant step yet: everybody is known
    none = mpc_filter.filter_correct_replay(table, gain, seed, state, est, index, innov0, xminus, 0)
    assert list(none["case"]) == ["known"] * M and np.all(none["est_index"] == -1) and np.array_equal(none["est"], est)
