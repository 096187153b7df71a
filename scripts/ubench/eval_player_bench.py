"""The player's two paths at 16384 envs, free space and the task default (pipe): env-steps/s of ``run(2048)`` by the host clock
(``run`` ends in the device->host copy of the totals, a synchronise follows), stock and device path alternated three times
after one warm-up run each (the device path's warm-up also captures its graph).  Raw lines go to
profiles/eval_player/player_paths.txt.

  python scripts/ubench/eval_player_bench.py                       # both configurations, both paths
  python scripts/ubench/eval_player_bench.py --trace-device pipe   # device path only, short: a workload for a kernel trace
  python scripts/ubench/eval_player_bench.py --record 64 --out profiles/record_trajectories/player_paths.txt
                                                                   # + the device path with RECORD_TRAJECTORIES of 64 envs
  python scripts/ubench/eval_player_bench.py --episode-log --out profiles/episode_log/player_paths.txt
                                                                   # + the device path with EPISODE_LOG, with and without the table
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from vine_robot_isaacgymenvs_amd import load_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.learning.player import PpoPlayerContinuous  # noqa: E402
from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map  # noqa: E402

CONFIGS = {"free": ["task.env.CREATE_PIPE=False"], "pipe": []}


def make(name, n, device_rollout, record=0, episode_log=None):
    cfg = load_config(overrides=["num_envs=%d" % n] + CONFIGS[name])
    cfg["task"]["seed"] = 42
    if record:      # the task's default window: maxEpisodeLength (500) steps every 1000, files into a scratch directory
        import tempfile
        cfg["task"]["env"].update(RECORD_TRAJECTORIES=True, RECORD_TRAJECTORIES_ENVS=record,
                                  RECORD_TRAJECTORIES_DIR=tempfile.mkdtemp(prefix="vine_trajectories_"))
    if episode_log:  # "table" or "totals"; the file goes into a scratch directory
        import tempfile
        cfg["task"]["env"].update(EPISODE_LOG=True, EPISODE_LOG_TABLE=episode_log == "table",
                                  EPISODE_LOG_DIR=tempfile.mkdtemp(prefix="vine_episodes_"))
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0",
                                                  graphics_device_id=0, headless=True)
    params = cfg["train"]["params"]
    params["config"]["player"] = {"device_rollout": device_rollout}
    torch.manual_seed(0)
    return PpoPlayerContinuous(params, vec_env=env), env


def timed_run(player, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        player.run(n_steps=steps)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-device", choices=sorted(CONFIGS), default=None)
    ap.add_argument("--record", type=int, default=0, help="also time the device path with RECORD_TRAJECTORIES of this many envs")
    ap.add_argument("--episode-log", action="store_true", help="also time the device path with EPISODE_LOG (table / totals only)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_player", "player_paths.txt"))
    args = ap.parse_args()
    if args.trace_device:
        player, env = make(args.trace_device, args.envs, True, args.record)
        timed_run(player, 64)
        dt = timed_run(player, 512)
        assert player.device_path is True
        print(json.dumps({"config": args.trace_device, "envs": args.envs, "steps": 512, "env_steps_per_s": args.envs * 512 / dt}))
        env.close()
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    lines = []
    for name in CONFIGS:
        players = {path: make(name, args.envs, path == "device") for path in ("stock", "device")}
        if args.record:
            players["device+record"] = make(name, args.envs, True, args.record)
        if args.episode_log:
            players["device+episodes"] = make(name, args.envs, True, episode_log="table")
            players["device+episodes(totals only)"] = make(name, args.envs, True, episode_log="totals")
        for path, (player, _) in players.items():
            timed_run(player, 64 if path != "stock" else 16)            # warm-up (device: the graph capture too)
            assert player.device_path is (path != "stock")
        for rnd in range(args.rounds):
            for path, (player, _) in players.items():
                dt = timed_run(player, args.steps)
                rec = {"config": name, "path": path, "round": rnd, "envs": args.envs, "steps": args.steps, "seconds": round(dt, 6),
                       "env_steps_per_s": round(args.envs * args.steps / dt, 1), "report": player.report}
                trajectory = getattr(players[path][1], "trajectory", None)
                if trajectory is not None:
                    rec.update(files=len(trajectory.written), skipped=len(trajectory.skipped),
                               harvest_ms=[round(1e3 * t, 3) for t in trajectory.harvest_seconds],
                               write_ms=[round(1e3 * t, 3) for t in trajectory.write_seconds])
                log = getattr(players[path][1], "episode_log", None)
                if log is not None:
                    rec.update(rows=int(len(log.rows()["env"])), dropped=log.dropped)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
        for _, env in players.values():
            scratch = getattr(getattr(env, "trajectory", None), "directory", None)
            if getattr(env, "episode_log", None) is not None:
                scratch = os.path.dirname(env.episode_log.path)
            env.close()
            if scratch:                       # the MAT files of the timed runs are not the result
                import shutil
                shutil.rmtree(scratch, ignore_errors=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
