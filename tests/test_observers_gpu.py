"""The three step observers on one task (needs an MI355X): what they harvest from 24 eager steps equals, bit for bit, what
they harvest from three replays of a graph of 8 steps captured by ``graph_capture.capture_rolled_back``.  And the three
observers with a table of named draws on one task, one env past a workgroup: every table against the one Python draw."""
import glob
import os

import numpy as np
import pytest
import scipy.io
import torch

from vine_robot_isaacgymenvs_amd import abi, load_task_config
from vine_robot_isaacgymenvs_amd.learning import graph_capture
from vine_robot_isaacgymenvs_amd.utils import episodes, named_draw

pytestmark = pytest.mark.gpu

N, GRAPH_STEPS, REPLAYS = 256, 8, 3


def _task(directory):
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % N])
    cfg["seed"] = 42
    d = str(directory)
    cfg["env"].update(maxEpisodeLength=8, CREATE_SHELF=False, CREATE_PIPE=False,
                      CAPTURE_VIDEO=True, CAPTURE_VIDEO_EVERY=8, CAPTURE_VIDEO_FRAMES=4, CAPTURE_VIDEO_VIEWS=1,
                      CAPTURE_VIDEO_WIDTH=64, CAPTURE_VIDEO_HEIGHT=48, CAPTURE_VIDEO_DIR=d,
                      RECORD_TRAJECTORIES=True, RECORD_TRAJECTORIES_EVERY=8, RECORD_TRAJECTORIES_STEPS=4,
                      RECORD_TRAJECTORIES_ENVS=2, RECORD_TRAJECTORIES_DIR=d,
                      EPISODE_LOG=True, EPISODE_LOG_CAPACITY=4096, EPISODE_LOG_DIR=d)
    return isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg, rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                    headless=True)


def _run(directory, actions, graphed):
    env = _task(directory)
    try:
        video, rec, log = env.video, env.trajectory, env.episode_log
        assert env._observers == [video, rec, log] == env.observers
        frames = {}
        video.on_frames = lambda f, last: frames.__setitem__(last, f)
        obs = [torch.zeros_like(env.obs_buf) for _ in range(2)]

        def drain():                     # pace the loop to the writers: a window that finds the host buffer taken is skipped
            video.drain()
            rec.drain()

        if graphed:
            def body():
                for t in range(GRAPH_STEPS):
                    env.step_into(actions[t], obs[t & 1])

            graph = graph_capture.capture_rolled_back(env.device, body, obs + env.live_tensors(), env)
            assert video.steps_done == rec.steps_done == env.step_count == 0
            for _ in range(REPLAYS):
                graph_capture.replay_observed(graph, env, GRAPH_STEPS)
                drain()
        else:
            for t in range(REPLAYS * GRAPH_STEPS):
                env.step_into(actions[t % GRAPH_STEPS], obs[t & 1])
                if t % GRAPH_STEPS == 3:
                    drain()
        torch.cuda.synchronize()
        drain()
        for o in (video, rec):
            assert list(o.skipped) == [] and o.windows_skipped == 0 and o.windows_written == REPLAYS
            assert o.steps_done == 24 == env.step_count
        log.harvest()
        assert log.dropped == 0
        mats = {os.path.basename(p).split("_trajectory_")[1]: scipy.io.loadmat(p) for p in glob.glob(os.path.join(str(directory), "*.mat"))}
        return {"frames": frames, "mats": mats, "rows": log.rows(), "totals": log.folded_totals(),
                "state": env.state.cpu().numpy(), "ring": rec.ring.cpu().numpy(), "steps": rec.steps.cpu().numpy()}
    finally:
        env.close()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_three_observers_eager_equals_graph_replay(tmp_path):
    g = torch.Generator(device="cuda:0").manual_seed(5)
    actions = torch.rand((GRAPH_STEPS, N, 2), device="cuda:0", generator=g) * 2 - 1
    a = _run(tmp_path / "eager", actions, graphed=False)
    b = _run(tmp_path / "graph", actions, graphed=True)
    for out in (a, b):
        assert sorted(out["frames"]) == [3, 11, 19]
        assert sorted(out["mats"]) == sorted("%d_env%d.mat" % (last, e) for last in (3, 11, 19) for e in (25, 26))
        assert len(out["rows"]["env"]) >= 2 * N              # 8-step episodes: every env finished at least twice in 24 steps
    for last in (3, 11, 19):
        assert a["frames"][last].shape == (4, 48, 64) and _same(a["frames"][last], b["frames"][last]), last
    for name, mat in a["mats"].items():
        keys = sorted(k for k in mat if not k.startswith("__"))
        assert keys == sorted(k for k in b["mats"][name] if not k.startswith("__")) and "Q" in keys
        for k in keys:
            assert _same(mat[k], b["mats"][name][k]), (name, k)
    for k in episodes.COLUMNS:
        assert _same(a["rows"][k], b["rows"][k]), k
    for k in ("totals", "state", "ring", "steps"):
        assert _same(a[k], b[k]), k
    assert a["steps"].tolist() == [16, 17, 18, 19]


class _Flags:
    """A step observer, last in the order, that keeps the step's reset flags as the launches in front of it saw them."""
    paused, copy_done = 0, None

    def __init__(self, env):
        self.env, self.reset = env, []

    def enqueue(self, stream, actions=None):
        self.reset.append(self.env.reset_buf.clone())

    def before(self, n):
        pass

    advance = set_steps = before

    def live_tensors(self):
        return []

    def drain(self):
        pass

    close = drain


def test_three_redraw_tails_one_env_past_a_workgroup():
    """ENV_SENSOR, ENV_PUSH and ENV_TARGET, all redrawn per episode, on one handle of N = the largest workgroup of the three
    units + 1 envs: the last env is alone in the second workgroup.  Six steps; the step itself resets envs 0, 1, N - 2 and
    N - 1 at steps 2 and 4 (their progress is put at the episode's last step in front of it).  Every observer's ``table`` and
    ``episode_index`` then equal, bit for bit, ``named_draw.draw`` at the episodes counted from the flags the launches saw:
    a wrong stride, a wrong id offset or a missed last lane in the shared tail shows here."""
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    n = max(abi.ENV_SENSOR_THREADS, abi.ENV_PUSH_THREADS, abi.ENV_TARGET_THREADS) + 1
    max_len, forced = 400, [0, 1, n - 2, n - 1]
    cfg = load_config(overrides=["num_envs=%d" % n, "task.env.CREATE_PIPE=False", "task.env.CREATE_SHELF=False",
                                 "task.env.maxEpisodeLength=%d" % max_len])
    cfg["task"]["seed"] = 42
    cfg["task"]["env"]["ENV_SENSOR"] = {"DELAY": {"values": [0, 2]}, "HOLD": [0.0, 0.3], "NOISE_STD": 0.01, "PER_EPISODE": True}
    cfg["task"]["env"]["ENV_PUSH"] = {"RATE": [0.1, 0.5], "IMPULSE": {"values": [0.002, 0.01]}, "PER_EPISODE": True}
    cfg["task"]["env"]["ENV_TARGET"] = {"VEL_ALONG": [-0.2, 0.2], "SPAN_ALONG": {"values": [0.03, 0.05]}, "PER_EPISODE": True}
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                  headless=True)
    try:
        flags = _Flags(env)
        env._observers.append(flags)
        observers = (env.env_sensor, env.env_push, env.env_target)
        assert all(o is not None and o.spec["PER_EPISODE"] and o.num_envs == n for o in observers)
        g = torch.Generator(device="cuda:0").manual_seed(9)
        actions = torch.rand((6, n, 2), device="cuda:0", generator=g) * 2 - 1
        obs = torch.zeros_like(env.obs_buf)
        for t in range(6):
            if t in (2, 4):
                env.progress_buf[forced] = max_len - 1
            env.step_into(actions[t], obs)
        torch.cuda.synchronize()
        seen = torch.stack(flags.reset).cpu().numpy() != 0
        assert seen.shape == (6, n) and seen[2, forced].all() and seen[4, forced].all()
        counted = seen.sum(axis=0).astype(np.int64)
        never = np.flatnonzero(counted == 0)
        assert counted[forced].min() >= 2 and len(never) >= n // 2
        gids = np.arange(n, dtype=np.int64) + int(env.env_sensor.env_id_offset)
        for o in observers:
            named = named_draw.named(o.NAMES, o.DRAW_NAMES, o.spec)
            assert len(named_draw.varying(o.NAMES, o.spec)) == 2, type(o).__name__
            want = named_draw.draw(named, o.seed, gids, counted, o.INTEGER).astype(np.float32)
            first = named_draw.draw(named, o.seed, gids, 0, o.INTEGER).astype(np.float32)
            assert np.array_equal(o.episodes_now(), counted), type(o).__name__
            assert _same(o.episode_index.cpu().numpy(), counted.astype(np.int32)), type(o).__name__
            table = o.table.cpu().numpy()
            assert _same(table, want), type(o).__name__
            assert _same(table[:, never], first[:, never]), type(o).__name__
            assert not _same(table[:, forced], first[:, forced]), type(o).__name__      # (the forced envs did get new values)
    finally:
        env.close()
