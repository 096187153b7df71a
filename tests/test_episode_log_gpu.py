"""EPISODE_LOG on the GPU: the episode kernel behind both step kernels against a NumPy restatement of the accounting (bit
for bit), against vine_step_eval's own totals in the player, as an observer of a training (nothing perturbed, graphs
replay it, the scalars are written), a ring that laps, and resets from outside the step.

WHAT SURVIVES A LAP (include/vine_episodes.h).  The ring keeps the newest ``capacity`` rows in append order.  With
capacity >= num_envs the waves of one step append in an unspecified order: every row of the steps after the lapped one
survives, and of the lapped step a subset of the right size.  With capacity < num_envs the launch is one workgroup that
appends in env order and does not write what the same step would lap: the survivors are exactly the newest ``capacity``
rows by (end step, env), row k in slot k % capacity."""
import glob
import math
import os

import numpy as np
import pytest
import torch

from tests.helpers import base_cfg
from tests.hip_env import HipEnv
from vine_robot_isaacgymenvs_amd import abi, load_config, load_task_config
from vine_robot_isaacgymenvs_amd.learning.player import REPORT_KEYS, eval_report
from vine_robot_isaacgymenvs_amd.utils import episodes, tfevents

pytestmark = pytest.mark.gpu

N, STEPS, MAX_LEN = 192, 60, 12
COUNT_COLS = [abi.EVAL_EPISODES, abi.EVAL_LENGTH_SUM, abi.EVAL_REACHED_EVER, abi.EVAL_REACHED_AT_END, abi.EVAL_END_TIMEOUT,
              abi.EVAL_END_RAIL_LIMIT, abi.EVAL_END_TIP_LIMIT, abi.EVAL_END_CONTACT]
REAL_COLS = [abi.EVAL_RETURN_SUM, abi.EVAL_FIRST_REACH_SUM, abi.EVAL_FINAL_DIST_SUM, abi.EVAL_MIN_DIST_SUM]
STATE_FIELDS = [abi.VF_TARGET_Y, abi.VF_TARGET_Z, abi.VF_OBJ_DEPTH, abi.VF_OBJ_ANGLE]


# ------------------------------------------------------------------------------------------- the NumPy restatement
class Accounting:
    """include/vine_episodes.h in NumPy: per-env accumulators in float32 (``ret`` by sequential fp32 adds), one 16-word row
    per finished episode in (end step, env) order, totals in float64."""

    def __init__(self, n, flags):
        self.n = n
        self.tip_armed = bool(flags & abi.FLAG_USE_TIP_LIMIT_HIT_RESET)
        self.contact_armed = bool(flags & abi.FLAG_USE_NONZERO_CONTACT_FORCE_RESET)
        self.ret, self.len = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.min, self.first = np.full(n, np.inf, np.float32), np.zeros(n, np.float32)
        self.words = []
        self.per_step = []           # rows appended by each step

    def clear(self, ids):
        self.ret[ids], self.len[ids], self.min[ids], self.first[ids] = 0.0, 0.0, np.inf, 0.0

    def step(self, s, rew, reset, timeouts, rm, fields):
        """``fields``: [4, n] float32 = VF_TARGET_Y, VF_TARGET_Z, VF_OBJ_DEPTH, VF_OBJ_ANGLE after the step."""
        rew, rm = np.asarray(rew, np.float32), np.asarray(rm, np.float32)
        dist, reached = -rm[:, 0], rm[:, 2] != 0
        self.ret = (self.ret + rew).astype(np.float32)
        self.len = self.len + np.float32(1)
        self.min = np.minimum(self.min, dist)
        self.first = np.where((self.first == 0) & reached, self.len, self.first).astype(np.float32)
        done = np.flatnonzero(np.asarray(reset) != 0)
        w = np.zeros((len(done), abi.EPISODES_WORDS), np.uint32)
        f, i = w.view(np.float32), w.view(np.int32)
        i[:, abi.VEW_ENV], i[:, abi.VEW_END_STEP] = done, s
        f[:, abi.VEW_LENGTH], f[:, abi.VEW_RETURN] = self.len[done], self.ret[done]
        f[:, abi.VEW_REACHED_EVER], f[:, abi.VEW_REACHED_AT_END] = self.first[done] != 0, reached[done]
        f[:, abi.VEW_FIRST_REACH], f[:, abi.VEW_FINAL_DIST], f[:, abi.VEW_MIN_DIST] = self.first[done], dist[done], self.min[done]
        i[:, abi.VEW_END_REASON] = ((np.asarray(timeouts)[done] != 0) * abi.EPISODES_END_TIMEOUT
                                    + (rm[done, 9] != 0) * abi.EPISODES_END_RAIL_LIMIT
                                    + ((rm[done, 11] != 0) & self.tip_armed) * abi.EPISODES_END_TIP_LIMIT
                                    + ((rm[done, 12] < 0) & self.contact_armed) * abi.EPISODES_END_CONTACT)
        f[:, abi.VEW_TARGET_Y:abi.VEW_OBJ_ANGLE + 1] = np.asarray(fields, np.float32)[:, done].T
        self.words.append(w)
        self.per_step.append(len(done))
        self.clear(done)

    def table(self):
        return np.concatenate(self.words) if self.words else np.zeros((0, abi.EPISODES_WORDS), np.uint32)

    def totals(self):
        return episodes.totals_of(episodes.decode_rows(self.table()))


def _sorted_words(words):
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, abi.EPISODES_WORDS)
    i = w.view(np.int32)
    return w[np.lexsort((i[:, abi.VEW_ENV], i[:, abi.VEW_END_STEP]))]


def _check_totals(got, want):
    """Integer-valued totals exact; real-valued ones within 1e-10 relative (float64 summation, at most 1e6 terms)."""
    got, want = np.asarray(got, np.float64).reshape(-1, abi.EVAL_NUM_TOTALS).sum(axis=0), np.asarray(want, np.float64)
    assert np.array_equal(got[COUNT_COLS], want[COUNT_COLS]), (got, want)
    assert np.array_equal(got[[abi.EVAL_FIRST_REACH_SUM]], want[[abi.EVAL_FIRST_REACH_SUM]])        # integer-valued too
    for c in REAL_COLS:
        assert abs(got[c] - want[c]) <= 1e-10 * abs(want[c]), (c, got[c], want[c])


# ------------------------------------------------------------------------------------- straight through the C ABI
class Lane(HipEnv):
    kernel = "lane"


class Quad(HipEnv):
    kernel = "quad"


def case_cfg(kind, n=N):
    """The four configurations of the kernel test.  ``lane``: an unscaled observation layout, which only the one-lane step
    kernel serves; ``shelf``: the F6 shelf placements with the contact reset armed.  Rail limit 0.2 m with carts started up
    to it, success distance 0.12 m with targets the tip passes, 12-step episodes: a random policy ends episodes by every
    reason within 60 steps (the counts were checked on the CPU oracle before these seeds were fixed)."""
    obs = abi.OBS_POS_ONLY if kind.startswith("lane") else abi.OBS_POS_AND_FD_VEL_AND_OBJ_INFO
    cfg = base_cfg(n, obs)
    cfg.max_episode_length = MAX_LEN
    cfg.success_dist = 0.12
    cfg.rail_soft_limit = 0.2
    cfg.min_target_y, cfg.max_target_y = -0.3, -0.1
    cfg.min_target_z, cfg.max_target_z = 0.53, 0.6
    cfg.random_init_cart_min_y, cfg.random_init_cart_max_y = -0.02, 0.2
    cfg.seed = {"quad-free": 11, "quad-shelf": 12, "lane-free": 13, "lane-shelf": 14}[kind]
    if kind.endswith("shelf"):
        cfg.set_flag(abi.FLAG_CREATE_SHELF, True)
        cfg.set_flag(abi.FLAG_USE_NONZERO_CONTACT_FORCE_RESET, True)
        cfg.min_target_y, cfg.max_target_y = -0.12, -0.02
        cfg.min_target_z, cfg.max_target_z = 0.56, 0.66
        cfg.min_target_depth, cfg.max_target_depth = 0.0, 0.1
    return cfg


def case_actions(kind, steps=STEPS, n=N):
    rng = np.random.default_rng(sum(map(ord, kind)))
    return (rng.random((steps, n, 2)) * 2.4 - 1.2).astype(np.float32)


class Logged:
    """A HipEnv with a bound reward matrix and the episode log's buffers, driven step by step."""

    def __init__(self, kind, capacity, n=N):
        self.cfg = case_cfg(kind, n)
        self.env = (Lane if kind.startswith("lane") else Quad)(self.cfg)
        self.lib, self.n, self.capacity = self.env.lib, n, capacity
        dev = self.env.dev
        self.ecfg = episodes.episodes_config(self.lib, capacity)
        self.rows = self.lib.vine_episodes_rows(self.env.h)
        self.episode = torch.zeros((4, n), device=dev)
        self.episode[abi.EVAL_EP_MIN_DIST] = math.inf
        # sentinel tails behind every buffer the kernel writes
        self.totals_all = torch.zeros((self.rows + 2, abi.EVAL_NUM_TOTALS), device=dev, dtype=torch.float64)
        self.totals_all[self.rows:] = -7.0
        self.table_all = torch.zeros((capacity + 8, abi.EPISODES_WORDS), device=dev, dtype=torch.int32)
        self.table_all[capacity:] = -7
        self.cursor_all = torch.tensor([0, -7], device=dev, dtype=torch.int64)

    totals = property(lambda self: self.totals_all[:self.rows])
    table = property(lambda self: self.table_all[:self.capacity])

    def log(self, table=True):
        e = self.env
        return self.lib.vine_episodes_scheduled(
            e.h, self.ecfg, e.rew_t.data_ptr(), e.reset_t.data_ptr(), e.progress_t.data_ptr(), e.timeouts_t.data_ptr(),
            self.episode.data_ptr(), self.totals_all.data_ptr(), self.table_all.data_ptr() if table else None,
            self.cursor_all.data_ptr() if table else None, torch.cuda.current_stream(e.dev).cuda_stream)

    def run(self, actions, acc, start=0):
        e = self.env
        for s in range(start, start + len(actions)):
            e.step(actions[s - start], sync=False)
            assert self.log() == abi.OK, self.lib.vine_last_error()
            torch.cuda.synchronize()
            acc.step(s, e.rew_t.cpu().numpy(), e.reset_t.cpu().numpy(), e.timeouts_t.cpu().numpy(),
                     e.reward_matrix_t.cpu().numpy(), e.state_t[STATE_FIELDS].cpu().numpy())

    def tails_intact(self):
        return (bool((self.totals_all[self.rows:] == -7.0).all()) and bool((self.table_all[self.capacity:] == -7).all())
                and int(self.cursor_all[1]) == -7)

    def close(self):
        self.env.close()


def coverage(words):
    """How many episodes ended by time-out, rail limit, contact, with the target reached, and after a single step."""
    w = np.asarray(words).view(np.uint32).reshape(-1, abi.EPISODES_WORDS)
    reason, f = w.view(np.int32)[:, abi.VEW_END_REASON], w.view(np.float32)
    return {"timeout": int(np.count_nonzero(reason & abi.EPISODES_END_TIMEOUT)),
            "rail": int(np.count_nonzero(reason & abi.EPISODES_END_RAIL_LIMIT)),
            "contact": int(np.count_nonzero(reason & abi.EPISODES_END_CONTACT)),
            "reached": int(np.count_nonzero(f[:, abi.VEW_REACHED_AT_END])),
            "length1": int(np.count_nonzero(f[:, abi.VEW_LENGTH] == 1))}


@pytest.mark.parametrize("kind", ["quad-free", "quad-shelf", "lane-free", "lane-shelf"])
def test_rows_and_totals_equal_the_numpy_accounting(kind):
    """192 envs (three workgroups of the four-lane step kernel in a grid of four; one workgroup of the episode kernel with
    64 idle lanes), 12-step episodes, 60 vine_step calls with seeded actions, the episode launch behind each.  After every
    step the host copies rew, reset, timeouts, the reward matrix and the four state fields and accounts in NumPy.  The
    sorted table equals the NumPy rows in all sixteen words, the accumulators equal NumPy's, integer totals are exact and
    real ones within 1e-10 relative.  Fails before the feature: the library has no vine_episodes_* symbols."""
    log = Logged(kind, capacity=8192)
    try:
        name = log.lib.vine_step_kernel_name(log.env.h).decode()
        assert name == ("vine_step_kernel" if kind.startswith("lane") else "vine_step_quad_kernel")
        log.env.bind_reward_matrix()
        acc = Accounting(N, log.cfg.flags)
        log.run(case_actions(kind), acc)
        want = acc.table()
        cursor = int(log.cursor_all[0])
        assert cursor == len(want) and cursor < log.capacity
        got = log.table.cpu().numpy()
        assert np.array_equal(_sorted_words(got[:cursor]), want)
        assert not got[cursor:].any()
        ep = log.episode.cpu().numpy()
        for k, a in enumerate((acc.ret, acc.len, acc.min, acc.first)):
            assert np.array_equal(ep[k].view(np.uint32), a.view(np.uint32)), k
        _check_totals(log.totals.cpu().numpy(), acc.totals())
        assert log.rows == 1 and log.tails_intact()
        cov = coverage(want)
        print(kind, len(want), "episodes", cov)
        assert cov["timeout"] >= 1 and cov["rail"] >= 1 and cov["reached"] >= 1 and cov["length1"] >= 1, cov
        assert (cov["contact"] >= 1) == kind.endswith("shelf"), cov
        # totals only: the same sums, no ring touched
        before = log.table_all.clone(), log.cursor_all.clone()
        log.env.step(case_actions(kind)[0], sync=False)
        assert log.log(table=False) == abi.OK
        torch.cuda.synchronize()
        assert torch.equal(log.table_all, before[0]) and torch.equal(log.cursor_all, before[1])
    finally:
        log.close()


def test_several_workgroups_of_the_episode_kernel():
    """600 envs: three workgroups of the episode kernel, the last with 88 lanes; each adds to its own row of the totals."""
    n = 600
    log = Logged("quad-free", capacity=4096, n=n)
    try:
        log.env.bind_reward_matrix()
        acc = Accounting(n, log.cfg.flags)
        log.run(case_actions("quad-free", steps=26, n=n), acc)
        want = acc.table()
        assert int(log.cursor_all[0]) == len(want) > n
        assert np.array_equal(_sorted_words(log.table.cpu().numpy()[:len(want)]), want)
        totals = log.totals.cpu().numpy()
        assert log.rows == 3 and log.tails_intact()
        for r in range(3):
            mine = want[(want.view(np.int32)[:, abi.VEW_ENV] // abi.EPISODES_THREADS) == r]
            _check_totals(totals[r], episodes.totals_of(episodes.decode_rows(mine)))
    finally:
        log.close()


def test_refuses_a_handle_without_a_reward_matrix():
    log = Logged("quad-free", capacity=64)
    try:
        log.env.step(case_actions("quad-free")[0], sync=False)
        assert log.log() == abi.ERR_INVALID_ARG
        assert b"needs a reward matrix bound to the handle" in log.lib.vine_last_error()
        e = log.env
        assert log.lib.vine_episodes_scheduled(e.h, log.ecfg, e.rew_t.data_ptr(), e.reset_t.data_ptr(), e.progress_t.data_ptr(),
                                               e.timeouts_t.data_ptr(), log.episode.data_ptr(), log.totals_all.data_ptr(),
                                               log.table_all.data_ptr(), None, None) == abi.ERR_INVALID_ARG
        assert b"both or neither" in log.lib.vine_last_error()
        torch.cuda.synchronize()
        assert int(log.cursor_all[0]) == 0 and not log.table.any() and log.tails_intact()
    finally:
        log.close()


@pytest.mark.parametrize("capacity", [64, 256])
def test_a_ring_that_laps_counts_what_it_loses(capacity):
    """No harvest for 60 steps at 192 envs.  The cursor equals the NumPy count of finished episodes and dropped is exact,
    also against a harvest point in mid-run.  capacity = 64 < 192 envs (one workgroup, env order): row k sits in slot
    k % 64 and the 64 survivors are exactly the newest by (end step, env) -- although the first time-out ends well over 64
    episodes in one step.  capacity = 256: the survivors are every row of the steps after the lapped one and, of that step,
    a subset of the right size."""
    log = Logged("quad-free", capacity=capacity)
    try:
        log.env.bind_reward_matrix()
        acc = Accounting(N, log.cfg.flags)
        actions = case_actions("quad-free")
        log.run(actions[:20], acc)
        harvested = int(log.cursor_all[0])
        assert harvested == sum(acc.per_step)
        log.run(actions[20:], acc, start=20)
        want = acc.table()
        cursor = int(log.cursor_all[0])
        assert cursor == len(want) and max(acc.per_step) > 64
        assert episodes.dropped_rows(cursor, 0, capacity) == cursor - capacity > 0
        assert episodes.dropped_rows(cursor, harvested, capacity) == cursor - harvested - capacity > 0
        got = log.table.cpu().numpy().view(np.uint32)
        assert log.tails_intact()
        if capacity < N:
            slots = np.arange(cursor - capacity, cursor) % capacity
            assert np.array_equal(got[slots], want[-capacity:])
        else:
            ends = np.cumsum(acc.per_step)
            first_whole = int(np.searchsorted(ends - np.asarray(acc.per_step), cursor - capacity, side="left"))
            whole = want[ends[first_whole - 1] if first_whole else 0:]
            got = _sorted_words(got)
            assert np.array_equal(got[capacity - len(whole):], whole)
            part = got[:capacity - len(whole)]
            lapped = want[(ends[first_whole - 2] if first_whole > 1 else 0):ends[first_whole - 1]] if first_whole else want[:0]
            keys = {r.tobytes() for r in lapped}
            assert len({r.tobytes() for r in part}) == len(part) and all(r.tobytes() in keys for r in part)
        _check_totals(log.totals.cpu().numpy(), acc.totals())
    finally:
        log.close()


# ------------------------------------------------------------------------------------------------- the task class
def _task(n, seed=42, **env_over):
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % n])
    cfg["seed"] = seed
    cfg["env"].update(env_over)
    return isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg, rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                    headless=True)


def test_a_reset_from_outside_the_step_leaves_no_row(tmp_path):
    """VecTask.step at 192 envs with the log on; after step 4 three envs in mid-episode are reset through reset_idx.  They
    leave no row for the abandoned episode, their next row's length counts from the reset, and the whole table still
    equals the NumPy accounting told of the same reset.  The file holds the same rows."""
    env = _task(N, seed=6, maxEpisodeLength=MAX_LEN, CREATE_PIPE=False, RAIL_SOFT_LIMIT=0.2, SUCCESS_DIST=0.12,
                EPISODE_LOG=True, EPISODE_LOG_CAPACITY=4096, EPISODE_LOG_DIR=str(tmp_path))
    try:
        log = env.episode_log
        assert log is not None and env._observers == [log] and log.table.shape == (4096, abi.EPISODES_WORDS)
        acc = Accounting(N, env._vcfg.flags)
        actions = torch.as_tensor(case_actions("quad-free", steps=30), device=env.device)
        picked, reset_after, next_end = None, 4, {}
        for s in range(30):
            env.step(actions[s])
            torch.cuda.synchronize()
            acc.step(s, env.rew_buf.cpu().numpy(), env.reset_buf.cpu().numpy(), env.timeout_buf.cpu().numpy(),
                     env._reward_matrix.cpu().numpy(), env.state[STATE_FIELDS].cpu().numpy())
            if s == reset_after:
                running = np.flatnonzero((env.reset_buf.cpu().numpy() == 0) & (acc.len >= 3))
                picked = running[[0, len(running) // 2, -1]]
                env.reset_idx(torch.as_tensor(picked, device=env.device))
                acc.clear(picked)
        assert picked is not None and len(set(picked.tolist())) == 3
        log.harvest()
        rows = log.rows()
        want = episodes.decode_rows(acc.table())
        for name in episodes.COLUMNS:
            assert np.array_equal(rows[name], want[name]), name
        for e in picked:
            mine = np.flatnonzero((rows["env"] == e) & (rows["end_step"] > reset_after))
            first = mine[0]
            assert rows["length"][first] == rows["end_step"][first] - reset_after <= MAX_LEN
            assert not np.any((rows["env"] == e) & (rows["end_step"] == reset_after))
        _check_totals(log.folded_totals(), acc.totals())
        assert log.dropped == 0
        env.close()
        (path,) = glob.glob(str(tmp_path / "*_episodes.npz"))
        got, totals, dropped, task = episodes.load(path)
        assert all(np.array_equal(got[name], rows[name]) for name in episodes.COLUMNS) and dropped == 0
        assert task["SUCCESS_DIST"] == 0.12 and task["maxEpisodeLength"] == MAX_LEN and not task["CREATE_PIPE"]
        assert episodes.report(got) == pytest.approx(eval_report(totals), rel=1e-12, nan_ok=True)
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------- the player
def test_player_log_equals_vine_step_eval(tmp_path, capsys):
    """The device player at 512 envs, 12-step episodes, 200 steps (twelve replays of a 16-step graph holding the episode
    launch, eight eager steps), the log on.  Its totals and report(rows) against the player's own eval_report from
    vine_step_eval: the eight count columns exact, the four real-valued sums within 1e-5 relative (the evaluation mode sums
    up to 64 episodes per workgroup in fp32 first: 64 x 2^-24 = 4e-6)."""
    from vine_robot_isaacgymenvs_amd.learning.player import PpoPlayerContinuous
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_config(overrides=["num_envs=512", "task.env.maxEpisodeLength=%d" % MAX_LEN])
    cfg["task"]["seed"] = 42
    cfg["task"]["env"].update(EPISODE_LOG=True, EPISODE_LOG_CAPACITY=16384, EPISODE_LOG_DIR=str(tmp_path))
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0",
                                                  graphics_device_id=0, headless=True)
    try:
        params = cfg["train"]["params"]
        params["config"]["player"] = {"graph_steps": 16}
        torch.manual_seed(0)
        player = PpoPlayerContinuous(params, vec_env=env)
        player.run(n_steps=200)
        torch.cuda.synchronize()
        assert player.device_path is True and player._eval_graph is not None
        theirs = player._dev["totals"].cpu().numpy().sum(axis=0)
        log = env.episode_log
        mine = log.folded_totals()
        rows = log.rows()
        from_rows = episodes.totals_of(rows)
        assert theirs[abi.EVAL_EPISODES] >= 512 * (200 // MAX_LEN) and log.dropped == 0
        for t in (mine, from_rows):
            assert np.array_equal(t[COUNT_COLS], theirs[COUNT_COLS]), (t, theirs)
            for c in REAL_COLS:
                assert abs(t[c] - theirs[c]) <= 1e-5 * abs(theirs[c]), (c, t[c], theirs[c])
        _check_totals(mine, from_rows)
        rep = episodes.report(rows)
        assert tuple(rep) == REPORT_KEYS and rep["episodes"] == player.report["episodes"]
        for k in REPORT_KEYS[1:]:
            assert rep[k] == pytest.approx(player.report[k], rel=1e-5, nan_ok=True), k
        assert torch.equal(log.episode, player._dev["episode"])      # and the running episodes, bit for bit
        out = capsys.readouterr().out
        assert "reached_ever_rate by obj_depth:" in out              # the default task has the pipe
        assert len(glob.glob(str(tmp_path / "*_episodes.npz"))) == 1
    finally:
        env.close()


# -------------------------------------------------------------------------------------------------------- training
def _train(tmp_path, monkeypatch, name, log, graphs=True):
    from vine_robot_isaacgymenvs_amd import train
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    run = tmp_path / name
    run.mkdir()
    monkeypatch.chdir(run)
    seen = {}
    play = A2CAgent.play_steps_rnn

    def play_and_keep(self):
        seen["agent"] = self
        return play(self)
    monkeypatch.setattr(A2CAgent, "play_steps_rnn", play_and_keep)
    argv = ["num_envs=512", "minibatch_size=2048", "seed=5", "max_iterations=3", "headless=True",
            "task.env.maxEpisodeLength=%d" % MAX_LEN, "+train.params.config.print_stats=False"]
    if not graphs:
        argv.append("train.params.config.use_graphs=False")
    if log:
        argv += ["task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_CAPACITY=32768"]
    train.main(argv)
    torch.cuda.synchronize()
    monkeypatch.setattr(A2CAgent, "play_steps_rnn", play)
    root = run / "runs" / "Vine5LinkMovingBase"
    ckpt = sorted(glob.glob(str(root / "nn" / "last_*ep3*.pth")))
    assert ckpt, os.listdir(str(root / "nn"))
    return torch.load(ckpt[-1], map_location="cpu", weights_only=False), seen["agent"], root


def test_training_is_not_perturbed_and_graphs_replay_the_log(tmp_path, monkeypatch):
    """Three iterations of 16 steps at 512 envs through train.py's entry, 12-step episodes.  Log on against off: every model
    parameter is bit-equal.  Log on, use_graphs on against off: the sorted tables and the totals are bit-equal.  The event
    file holds episodes/reached_ever_rate and episodes/episodes at the frame of every iteration that finished an episode
    (all three: 16 steps outlast a 12-step episode), and the episodes add up to the table."""
    off, off_agent, _ = _train(tmp_path, monkeypatch, "off", False)
    on, agent, root = _train(tmp_path, monkeypatch, "on", True)
    eager, eager_agent, eager_root = _train(tmp_path, monkeypatch, "eager", True, graphs=False)
    assert getattr(off_agent.vec_env, "env", off_agent.vec_env).episode_log is None
    assert agent.use_graphs and agent._rollout_graph is not None and not eager_agent.use_graphs
    assert on["model"].keys() == off["model"].keys()
    for k in on["model"]:
        assert torch.equal(on["model"][k], off["model"][k]), k
    tables = []
    for r in (root, eager_root):
        (path,) = glob.glob(str(r / "*_episodes.npz"))
        tables.append(episodes.load(path))
    (rows, totals, dropped, _), (erows, etotals, edropped, _) = tables
    assert dropped == edropped == 0 and len(rows["env"]) >= 3 * 512
    for name in episodes.COLUMNS:
        assert np.array_equal(rows[name].view(np.uint32 if rows[name].dtype == np.float32 else np.int64),
                              erows[name].view(np.uint32 if erows[name].dtype == np.float32 else np.int64)), name
    assert np.array_equal(totals, etotals)
    _check_totals(totals, episodes.totals_of(rows))
    assert rows["end_step"].max() < 48
    (events,) = glob.glob(str(root / "summaries" / "events.out.tfevents.*"))
    scalars = tfevents.read_scalars(events)
    frames = [512 * 16 * (i + 1) for i in range(3)]
    for tag in ("episodes/episodes", "episodes/reached_ever_rate"):
        assert [step for t, _, step, _ in scalars if t == tag] == frames, tag
    counts = [v for t, v, _, _ in scalars if t == "episodes/episodes"]
    per_iter = [int(np.count_nonzero(rows["end_step"] // 16 == i)) for i in range(3)]
    assert [int(c) for c in counts] == per_iter and min(per_iter) > 0
    rates = [v for t, v, _, _ in scalars if t == "episodes/reached_ever_rate"]
    for i in range(3):
        sel = rows["end_step"] // 16 == i
        assert rates[i] == pytest.approx(float(rows["reached_ever"][sel].mean()), rel=1e-6)
    tags = {t for t, _, _, _ in scalars if t.startswith("episodes/")}
    assert tags <= {"episodes/" + k for k in REPORT_KEYS} and len(tags) >= 11
