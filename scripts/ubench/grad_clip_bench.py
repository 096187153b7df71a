"""What ``truncate_grads: True`` costs per PPO iteration at 16384 envs: whole iterations timed by
``learning.bench_support.ppo_iteration_rate`` (the bench line's method) with the switch off and on, alternated, on the
default train config otherwise.  ``grad_norm`` defaults to the YAML's value; the arithmetic is not looked at here
(tests/test_grad_clip_device.py does that).  Raw lines go to profiles/grad_clip_device/.

  python scripts/ubench/grad_clip_bench.py                         # off / on, three rounds
  python scripts/ubench/grad_clip_bench.py --only on --rounds 1    # a workload for a kernel trace
"""
import argparse
import copy
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from vine_robot_isaacgymenvs_amd import load_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.learning.bench_support import ppo_iteration_rate  # noqa: E402
from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grad-norm", type=float, default=None)
    ap.add_argument("--only", choices=["off", "on"], default=None)
    args = ap.parse_args()
    cfg = load_config(overrides=["num_envs=%d" % args.envs])
    cfg["task"]["seed"] = 42
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0",
                                                  graphics_device_id=0, headless=True)
    for rnd in range(args.rounds):
        for name in ("off", "on"):
            if args.only not in (None, name):
                continue
            c = copy.deepcopy(cfg)
            conf = c["train"]["params"]["config"]
            conf["truncate_grads"] = name == "on"
            if args.grad_norm is not None:
                conf["grad_norm"] = args.grad_norm
            torch.manual_seed(0)
            r = ppo_iteration_rate(env, c, steps=args.steps, warmup=args.warmup)
            print(json.dumps({"truncate_grads": name, "round": rnd, "grad_norm": conf["grad_norm"],
                              "ms_per_iteration": round(r["ms_per_iteration"], 4), "rollout_ms": round(r["rollout_ms"], 4),
                              "update_ms": round(r["update_ms"], 4), "env_steps_per_sec": round(r["env_steps_per_sec"]),
                              "update": r["hipgraphs_active"]["update"]}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
