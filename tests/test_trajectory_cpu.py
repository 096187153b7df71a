"""RECORD_TRAJECTORIES without a GPU: the C ABI of include/vine_record.h against its ctypes mirror, the refusal of bad
configurations, the MAT file writer on a synthetic ring, and the window arithmetic against a literal loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils.trajectory import write_trajectory_mat
from vine_robot_isaacgymenvs_amd.utils.video import capture_schedule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(REPO, "include", "vine_record.h")).read()


def _header_functions():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(vine_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def hip_lib():
    native.build()
    return native.load()


def _rcfg(lib, **over):
    c = abi.VineRecordConfig()
    assert lib.vine_record_config_default(c) == abi.OK
    for k, v in over.items():
        setattr(c, k, v)
    return c


# --------------------------------------------------------------------------------------------------------------- ABI
def test_record_header_and_ctypes_mirror_agree(hip_lib):
    names = _header_functions()
    assert names == sorted(abi.RECORD_PROTOTYPES) and len(names) == 5
    for name in names:
        assert hasattr(hip_lib, name), name
    assert hip_lib.vine_record_config_size() == C.sizeof(abi.VineRecordConfig)
    text = _header()
    fields = re.findall(r"^\s+int32_t\s+([a-z_]+);", re.search(r"typedef struct VineRecordConfig \{(.*?)\}", text, re.S).group(1),
                        re.M)
    assert fields == [n for n, _ in abi.VineRecordConfig._fields_]
    for macro, value in (("ABI_VERSION", abi.RECORD_ABI_VERSION), ("FIELDS", abi.RECORD_FIELDS), ("MAX_ENVS", abi.RECORD_MAX_ENVS)):
        assert int(re.search(r"#define VINE_RECORD_%s (\d+)" % macro, text).group(1)) == value
    enum = re.findall(r"\b(VRF_[A-Z_0-9]+) = (\d+)", text)
    assert [(k, int(v)) for k, v in enum] == [(k, getattr(abi, k)) for k, _ in enum] and len(enum) == 18
    # the recorder's declarations stay out of vine.h: the CPU oracle exports every symbol of that header
    assert "vine_record" not in open(os.path.join(REPO, "include", "vine.h")).read()
    assert not set(abi.RECORD_PROTOTYPES) & set(abi.PROTOTYPES)


def test_record_defaults_and_ring_size(hip_lib):
    c = _rcfg(hip_lib)
    assert (c.abi_version, c.record_every, c.num_steps, c.num_envs) == (1, 1000, 500, 1)
    assert hip_lib.vine_record_ring_bytes(c) == 500 * 1 * 32 * 4
    c = _rcfg(hip_lib, record_every=9, num_steps=6, num_envs=5)
    assert hip_lib.vine_record_ring_bytes(c) == 6 * 5 * abi.RECORD_FIELDS * 4
    c = _rcfg(hip_lib, record_every=6, num_steps=6, num_envs=abi.RECORD_MAX_ENVS)
    assert hip_lib.vine_record_ring_bytes(c) == 6 * 64 * 128


@pytest.mark.parametrize("over, word", [(dict(num_envs=0), b"num_envs"), (dict(num_envs=abi.RECORD_MAX_ENVS + 1), b"num_envs"),
                                        (dict(record_every=10, num_steps=11), b"num_steps"), (dict(num_steps=0), b"num_steps"),
                                        (dict(abi_version=7), b"abi_version")])
def test_record_refuses_bad_configs(hip_lib, over, word):
    """Validation comes before the handle or any pointer is looked at, so no device is needed to see it."""
    bad = _rcfg(hip_lib, **over)
    assert hip_lib.vine_record_ring_bytes(bad) == abi.ERR_INVALID_ARG
    assert word in hip_lib.vine_last_error()
    for fn, lead in ((hip_lib.vine_record, (None, bad, 0)), (hip_lib.vine_record_scheduled, (None, bad))):
        hip_lib.vine_set_step_count(None, -1)             # leaves another message behind
        assert fn(*lead, *([None] * 9)) == abi.ERR_INVALID_ARG
        assert word in hip_lib.vine_last_error()


def test_record_refuses_null_pointers(hip_lib):
    good = _rcfg(hip_lib)
    for fn, lead in ((hip_lib.vine_record, (None, good, 0)), (hip_lib.vine_record_scheduled, (None, good))):
        assert fn(*lead, *([None] * 9)) == abi.ERR_INVALID_ARG
        assert b"null argument to vine_record" in hip_lib.vine_last_error()
    assert hip_lib.vine_record_config_default(None) == abi.ERR_INVALID_ARG
    assert hip_lib.vine_record_ring_bytes(None) == abi.ERR_INVALID_ARG and b"NULL" in hip_lib.vine_last_error()


# ---------------------------------------------------------------------------------------------------------- MAT file
def test_write_trajectory_mat_round_trip(tmp_path):
    import scipy.io
    T, F = 7, abi.RECORD_FIELDS
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((T, F)).astype(np.float32)
    rows[:, abi.VRF_RESET] = [0, 0, 1, 0, 0, 0, 1]
    rows[:, abi.VRF_TIMEOUT] = [0, 0, 0, 0, 0, 0, 1]
    rows[:, abi.VRF_PROGRESS] = [1, 2, 3, 0, 1, 2, 3]
    steps = np.arange(18, 18 + T)
    path = write_trajectory_mat(str(tmp_path / "t.mat"), rows, steps, 0.03332, env=409)
    assert path.endswith("t.mat") and os.listdir(str(tmp_path)) == ["t.mat"]
    m = scipy.io.loadmat(path)
    keys = {k for k in m if not k.startswith("__")}
    assert keys == {"cart_pos", "Q", "moving_target_pos", "target_vel", "tip_pos", "tip_vel", "cart_vel", "Qd", "action",
                    "smoothed_u_fpam", "reward", "reset", "time_out", "progress", "obj_info", "contact", "step", "dt", "env"}
    shapes = dict(cart_pos=(1, T), Q=(5, T), moving_target_pos=(3, T), target_vel=(3, 1), tip_pos=(3, T), tip_vel=(3, T),
                  cart_vel=(1, T), Qd=(5, T), action=(2, T), smoothed_u_fpam=(1, T), reward=(1, T), reset=(1, T),
                  time_out=(1, T), progress=(1, T), obj_info=(2, T), contact=(1, T), step=(1, T), dt=(1, 1), env=(1, 1))
    for k, shape in shapes.items():
        assert m[k].shape == shape, k
        assert m[k].dtype == (np.int64 if k in ("step", "env") else np.float64), k
    r = rows.astype(np.float64)              # exact
    assert np.array_equal(m["cart_pos"][0], r[:, 0]) and np.array_equal(m["Q"], r[:, 1:6].T)
    assert np.array_equal(m["cart_vel"][0], r[:, 6]) and np.array_equal(m["Qd"], r[:, 7:12].T)
    assert np.array_equal(m["tip_pos"][1:], r[:, 12:14].T) and np.array_equal(m["tip_vel"][1:], r[:, 14:16].T)
    assert np.array_equal(m["moving_target_pos"][1:], r[:, 16:18].T)
    for k in ("tip_pos", "tip_vel", "moving_target_pos"):
        assert not m[k][0].any(), k                                   # the x rows
    assert not m["target_vel"].any()
    assert np.array_equal(m["action"], r[:, 18:20].T) and np.array_equal(m["smoothed_u_fpam"][0], r[:, 20])
    assert np.array_equal(m["reward"][0], r[:, 21]) and np.array_equal(m["reset"][0], r[:, 22])
    assert np.array_equal(m["time_out"][0], r[:, 23]) and np.array_equal(m["progress"][0], r[:, 24])
    assert np.array_equal(m["obj_info"], r[:, 25:27].T) and np.array_equal(m["contact"][0], r[:, 27])
    assert np.array_equal(m["step"][0], steps) and m["dt"][0, 0] == 0.03332 and m["env"][0, 0] == 409
    with pytest.raises(AssertionError):
        write_trajectory_mat(str(tmp_path / "bad.mat"), rows[:, :31], steps, 0.03332)


# ---------------------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("every, steps", [(9, 6), (6, 6), (1000, 500)])
def test_window_arithmetic_matches_a_literal_loop(every, steps):
    """vine_record_scheduled's rule, step by step: step s goes to slot s % every iff that is < steps; a window is complete
    with its last slot, and the file carries that step's index."""
    total = 4 * every + 3
    draws, files = [], []
    for s in range(total):
        slot = s % every
        if slot < steps:
            draws.append((s, slot))
            if slot == steps - 1:
                files.append((s - slot, s))
    for chunk in (1, 16, 7):
        got_draws, got_done, done = [], [], 0
        while done < total:
            n = min(chunk, total - done)
            d, completed, opens = capture_schedule(done, n, every, steps)
            assert opens == any(slot == 0 for _, slot in d)
            got_draws += d
            got_done += completed
            done += n
        assert got_draws == draws and got_done == files
    assert [last for _, last in files] == [w * every + steps - 1 for w in range(4)]
