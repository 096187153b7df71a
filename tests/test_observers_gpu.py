"""The three step observers on one task (needs an MI355X): what they harvest from 24 eager steps equals, bit for bit, what
they harvest from three replays of a graph of 8 steps captured by ``graph_capture.capture_rolled_back``."""
import glob
import os

import numpy as np
import pytest
import scipy.io
import torch

from vine_robot_isaacgymenvs_amd import load_task_config
from vine_robot_isaacgymenvs_amd.learning import graph_capture
from vine_robot_isaacgymenvs_amd.utils import episodes

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
