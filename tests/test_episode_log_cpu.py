"""EPISODE_LOG without a GPU: the C ABI of include/vine_episodes.h against its ctypes mirror, the refusals that need no
device, and the host side (utils/episodes.py) on synthetic rows: sort, report, binned rates, the dropped-row arithmetic
and the file.  (The refusal of a handle without a bound reward matrix needs a handle, hence a device: it is in
tests/test_episode_log_gpu.py.)"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.learning.player import REPORT_KEYS, eval_report
from vine_robot_isaacgymenvs_amd.utils import episodes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(REPO, "include", "vine_episodes.h")).read()


@pytest.fixture(scope="module")
def hip_lib():
    native.build()
    return native.load()


def _ecfg(lib, **over):
    c = abi.VineEpisodesConfig()
    assert lib.vine_episodes_config_default(c) == abi.OK
    for k, v in over.items():
        setattr(c, k, v)
    return c


# --------------------------------------------------------------------------------------------------------------- ABI
def test_episodes_header_and_ctypes_mirror_agree(hip_lib):
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(vine_[a-z_0-9]+)\s*\(", code)))
    assert names == sorted(abi.EPISODES_PROTOTYPES) and len(names) == 5
    for name in names:
        assert hasattr(hip_lib, name), name
    assert hip_lib.vine_episodes_config_size() == C.sizeof(abi.VineEpisodesConfig) == 16
    fields = re.findall(r"^\s+int(?:32|64)_t\s+([a-z_]+);",
                        re.search(r"typedef struct VineEpisodesConfig \{(.*?)\}", code, re.S).group(1), re.M)
    assert fields == [n for n, _ in abi.VineEpisodesConfig._fields_]
    for macro, value in (("ABI_VERSION", abi.EPISODES_ABI_VERSION), ("WORDS", abi.EPISODES_WORDS),
                         ("THREADS", abi.EPISODES_THREADS)):
        assert int(re.search(r"#define VINE_EPISODES_%s (\d+)" % macro, code).group(1)) == value
    # the sixteen words of a row: fourteen named ones in the order of episodes.COLUMNS, two reserved
    enum = [(k, int(v)) for k, v in re.findall(r"\b(VEW_[A-Z_0-9]+) = (\d+)", code)]
    assert enum == [(k, getattr(abi, k)) for k, _ in enum] and len(enum) == 15
    assert [v for _, v in enum] == list(range(15)) and abi.VEW_RESERVED0 == len(episodes.COLUMNS) == 14
    assert [k[4:].lower() for k, _ in enum[:14]] == list(episodes.COLUMNS)
    assert abi.EPISODES_WORDS == 16
    bits = [(k, int(v)) for k, v in re.findall(r"\bVINE_EPISODES_(END_[A-Z_]+) = (\d+)", code)]
    assert bits == [("END_TIMEOUT", 1), ("END_RAIL_LIMIT", 2), ("END_TIP_LIMIT", 4), ("END_CONTACT", 8)]
    assert all(getattr(abi, "EPISODES_" + k) == v for k, v in bits)
    # the totals and the accumulators are vine_step_eval's
    ppo = open(os.path.join(REPO, "include", "vine_ppo.h")).read()
    assert int(re.search(r"#define VINE_EVAL_NUM_TOTALS (\d+)", ppo).group(1)) == abi.EVAL_NUM_TOTALS == len(REPORT_KEYS)
    assert int(re.search(r"#define VINE_EVAL_EPISODE_FIELDS (\d+)", ppo).group(1)) == abi.EVAL_EPISODE_FIELDS == 4
    # out of vine.h: the CPU oracle exports every symbol of that header
    assert "vine_episodes" not in open(os.path.join(REPO, "include", "vine.h")).read()
    assert not set(abi.EPISODES_PROTOTYPES) & set(abi.PROTOTYPES)
    # the fingerprint of the library covers the new source and header
    deps = [os.path.basename(d) for d in native.DEPS]
    assert "vine_episodes.hip" in deps and "vine_episodes.h" in deps


def test_episodes_defaults_and_table_size(hip_lib):
    c = _ecfg(hip_lib)
    assert (c.abi_version, c.reserved, c.capacity) == (1, 0, 1048576)
    assert hip_lib.vine_episodes_table_bytes(c) == 1048576 * 64
    assert hip_lib.vine_episodes_table_bytes(_ecfg(hip_lib, capacity=64)) == 64 * 16 * 4
    assert hip_lib.vine_episodes_table_bytes(_ecfg(hip_lib, capacity=1)) == 64


@pytest.mark.parametrize("over, word", [(dict(capacity=0), b"capacity"), (dict(capacity=-5), b"capacity"),
                                        (dict(capacity=(1 << 40) + 1), b"capacity"), (dict(reserved=1), b"reserved"),
                                        (dict(abi_version=7), b"abi_version")])
def test_episodes_refuses_bad_configs(hip_lib, over, word):
    """Validation comes before the handle or any pointer is looked at, so no device is needed to see it."""
    bad = _ecfg(hip_lib, **over)
    assert hip_lib.vine_episodes_table_bytes(bad) == abi.ERR_INVALID_ARG
    assert word in hip_lib.vine_last_error()
    hip_lib.vine_set_step_count(None, -1)                 # leaves another message behind
    assert hip_lib.vine_episodes_scheduled(None, bad, *([None] * 9)) == abi.ERR_INVALID_ARG
    assert word in hip_lib.vine_last_error()


def test_episodes_refuses_null_pointers(hip_lib):
    good = _ecfg(hip_lib)
    assert hip_lib.vine_episodes_scheduled(None, good, *([None] * 9)) == abi.ERR_INVALID_ARG
    assert b"null argument to vine_episodes_scheduled" in hip_lib.vine_last_error()
    assert hip_lib.vine_episodes_scheduled(None, None, *([None] * 9)) == abi.ERR_INVALID_ARG
    assert b"NULL" in hip_lib.vine_last_error()
    assert hip_lib.vine_episodes_config_default(None) == abi.ERR_INVALID_ARG
    assert hip_lib.vine_episodes_table_bytes(None) == abi.ERR_INVALID_ARG and b"NULL" in hip_lib.vine_last_error()
    assert hip_lib.vine_episodes_rows(None) == abi.ERR_INVALID_ARG
    assert b"null argument to vine_episodes_rows" in hip_lib.vine_last_error()


# --------------------------------------------------------------------------------------------------------- host side
def _synthetic_words(rng, count, n_envs=37):
    """``count`` rows as the device writes them, in a shuffled order; returns (words, the same rows as float64 lists)."""
    w = np.zeros((count, abi.EPISODES_WORDS), dtype=np.uint32)
    f = w.view(np.float32)
    i = w.view(np.int32)
    keys = rng.permutation(n_envs * 50)[:count]            # distinct (end step, env) pairs
    i[:, abi.VEW_ENV] = keys % n_envs
    i[:, abi.VEW_END_STEP] = keys // n_envs
    f[:, abi.VEW_LENGTH] = rng.integers(1, 13, count)
    f[:, abi.VEW_RETURN] = rng.standard_normal(count) * 30
    ever = rng.random(count) < 0.4
    f[:, abi.VEW_REACHED_EVER] = ever
    f[:, abi.VEW_REACHED_AT_END] = ever & (rng.random(count) < 0.7)
    f[:, abi.VEW_FIRST_REACH] = np.where(ever, np.minimum(rng.integers(1, 13, count), f[:, abi.VEW_LENGTH]), 0)
    f[:, abi.VEW_MIN_DIST] = rng.random(count) * 0.3
    f[:, abi.VEW_FINAL_DIST] = f[:, abi.VEW_MIN_DIST] + rng.random(count) * 0.1
    i[:, abi.VEW_END_REASON] = rng.integers(0, 16, count)
    f[:, abi.VEW_TARGET_Y] = -0.48 + 0.08 * rng.random(count)
    f[:, abi.VEW_TARGET_Z] = 0.58 + 0.09 * rng.random(count)
    f[:, abi.VEW_OBJ_DEPTH] = rng.random(count) * 0.2
    f[:, abi.VEW_OBJ_ANGLE] = rng.standard_normal(count) * 0.1
    return w


def test_decode_sorts_by_end_step_then_env_and_keeps_bits():
    rng = np.random.default_rng(3)
    w = _synthetic_words(rng, 300)
    rows = episodes.decode_rows(w)
    assert tuple(rows) == episodes.COLUMNS
    key = rows["end_step"] * 1000 + rows["env"]
    assert np.all(np.diff(key) > 0)
    order = np.argsort(w.view(np.int32)[:, abi.VEW_END_STEP].astype(np.int64) * 1000 + w.view(np.int32)[:, abi.VEW_ENV])
    for k, name in enumerate(episodes.COLUMNS):
        col = w[order, k]
        if name in episodes.INT_COLUMNS:
            assert rows[name].dtype == np.int64 and np.array_equal(rows[name], col.view(np.int32))
        else:
            assert rows[name].dtype == np.float32 and np.array_equal(rows[name].view(np.uint32), col)
    # harvested in pieces and put together: the same table
    parts = [episodes.decode_rows(w[a:b]) for a, b in ((0, 110), (110, 110), (110, 300))]
    whole = episodes.concat_rows(parts)
    assert all(np.array_equal(whole[name], rows[name]) for name in episodes.COLUMNS)
    empty = episodes.concat_rows([])
    assert all(len(empty[name]) == 0 for name in episodes.COLUMNS)


def test_report_of_rows_equals_eval_report_of_their_totals():
    rng = np.random.default_rng(4)
    w = _synthetic_words(rng, 257)
    rows = episodes.decode_rows(w)
    f, i = w.view(np.float32).astype(np.float64), w.view(np.int32)
    t = np.zeros(abi.EVAL_NUM_TOTALS)
    for r in range(len(w)):                               # a literal loop over the words
        t[abi.EVAL_EPISODES] += 1
        t[abi.EVAL_RETURN_SUM] += f[r, abi.VEW_RETURN]
        t[abi.EVAL_LENGTH_SUM] += f[r, abi.VEW_LENGTH]
        t[abi.EVAL_REACHED_EVER] += f[r, abi.VEW_REACHED_EVER]
        t[abi.EVAL_REACHED_AT_END] += f[r, abi.VEW_REACHED_AT_END]
        t[abi.EVAL_FIRST_REACH_SUM] += f[r, abi.VEW_FIRST_REACH]
        t[abi.EVAL_FINAL_DIST_SUM] += f[r, abi.VEW_FINAL_DIST]
        t[abi.EVAL_MIN_DIST_SUM] += f[r, abi.VEW_MIN_DIST]
        t[abi.EVAL_END_TIMEOUT] += bool(i[r, abi.VEW_END_REASON] & 1)
        t[abi.EVAL_END_RAIL_LIMIT] += bool(i[r, abi.VEW_END_REASON] & 2)
        t[abi.EVAL_END_TIP_LIMIT] += bool(i[r, abi.VEW_END_REASON] & 4)
        t[abi.EVAL_END_CONTACT] += bool(i[r, abi.VEW_END_REASON] & 8)
    got, want = episodes.report(rows), eval_report(t)
    assert tuple(got) == REPORT_KEYS
    for k in REPORT_KEYS:
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    for k in ("episodes", "reached_ever_rate", "reached_at_end_rate", "length_mean", "steps_to_reach_mean",
              "end_timeout_rate", "end_rail_limit_rate", "end_tip_limit_rate", "end_contact_rate"):
        assert got[k] == want[k], k                       # sums of small integers: exact in any order
    none = episodes.report(episodes.concat_rows([]))
    assert none["episodes"] == 0 and math.isnan(none["reached_ever_rate"]) and math.isnan(none["steps_to_reach_mean"])


def test_binned_rate():
    rows = {"obj_depth": np.array([0.01, 0.02, 0.06, 0.07, 0.08, 0.19, 0.195], dtype=np.float32),
            "reached_ever": np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.float32),
            "reached_at_end": np.array([0, 0, 1, 0, 0, 0, 1], dtype=np.float32)}
    rate, count, edges = episodes.binned_rate(rows, "obj_depth", [0.0, 0.05, 0.1, 0.15, 0.2])
    assert np.array_equal(count, [2, 3, 0, 2]) and np.array_equal(edges, [0.0, 0.05, 0.1, 0.15, 0.2])
    assert rate[0] == 0.5 and rate[1] == pytest.approx(2 / 3) and math.isnan(rate[2]) and rate[3] == 0.5
    rate, count, _ = episodes.binned_rate(rows, "obj_depth", [0.0, 0.1, 0.2], of="reached_at_end")
    assert np.array_equal(count, [5, 2]) and rate[0] == 0.2 and rate[1] == 0.5
    rate, count, edges = episodes.binned_rate(rows, "obj_depth", 2)
    assert len(rate) == 2 and count.sum() == 7 and len(edges) == 3


@pytest.mark.parametrize("cursor, harvested, capacity, want", [(0, 0, 64, 0), (64, 0, 64, 0), (65, 0, 64, 1), (500, 100, 64, 336),
                                                               (163, 100, 64, 0), (164, 100, 64, 0), (165, 100, 64, 1)])
def test_dropped_arithmetic_matches_a_literal_ring(cursor, harvested, capacity, want):
    assert episodes.dropped_rows(cursor, harvested, capacity) == want
    ring = [None] * capacity                              # row k lives in slot k % capacity
    for k in range(cursor):
        ring[k % capacity] = k
    alive = [k for k in ring if k is not None and k >= harvested]
    assert (cursor - harvested) - len(alive) == want


def test_npz_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    rows = episodes.decode_rows(_synthetic_words(rng, 40))
    totals = rng.random((3, abi.EVAL_NUM_TOTALS))
    task = {"SUCCESS_DIST": 0.08, "MIN_TARGET_Z": 0.58, "CREATE_SHELF": True, "maxEpisodeLength": 12}
    path = episodes.save(str(tmp_path / "sub" / "x_episodes.npz"), rows, totals, 7, task)
    assert os.listdir(str(tmp_path / "sub")) == ["x_episodes.npz"]
    got, t, dropped, tk = episodes.load(path)
    assert tuple(got) == episodes.COLUMNS and dropped == 7
    for name in episodes.COLUMNS:
        assert got[name].dtype == rows[name].dtype and np.array_equal(got[name], rows[name]), name
    assert np.array_equal(t, totals.sum(axis=0))
    assert tk == {"SUCCESS_DIST": 0.08, "MIN_TARGET_Z": 0.58, "CREATE_SHELF": True, "maxEpisodeLength": 12}
    assert episodes.report(got) == pytest.approx(episodes.report(rows), nan_ok=True)


def test_config_keys_are_off_by_default():
    from vine_robot_isaacgymenvs_amd.cfg import defaults
    env = defaults.TASK["Vine5LinkMovingBase"]["env"]
    assert env["EPISODE_LOG"] is False and env["EPISODE_LOG_TABLE"] is True
    assert env["EPISODE_LOG_CAPACITY"] == 1048576 and env["EPISODE_LOG_DIR"] == ""
