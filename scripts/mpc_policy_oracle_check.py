#!/usr/bin/env python3
"""MPC_POLICY on the CPU: the numpy statements of utils/mpc.py and utils/mpc_policy.py (sample_actions, act, keep, cost_sums,
mpc_replay, compose) around float64 oracle envs and the stock PyTorch network in float64, for the two runs of
tests/test_mpc_policy_gpu.py::test_it_plans.  No GPU is needed.

  python scripts/mpc_policy_oracle_check.py                     # the test's values: 4 plants, K = 128, H = 12, 60 control steps
  python scripts/mpc_policy_oracle_check.py --samples 256

The configuration is DESIGN.md section 24's "it controls": free space, the Position and Rail Limit reward weights 1 and every
other weight 0 on both handles, no target-reached reset, ACTION_DELAY 1, sigma 0.5, lambda 0.05, 60 control steps behind one
plant step on action zero.  The policy is a freshly initialised network (``torch.manual_seed(--net-seed)``).  The plants are
one oracle env of M envs, the samples one of M * K; a fork copies the plant's whole state column (both stand at the same step
count, so the delay ring goes with it).  Run A is the policy alone (sigma = 0: every sample is the policy, K = 2 suffices);
run B plans around it.  Prints the summed plant reward of both and their ratio per plant; profiles/mpc_policy/it_plans.txt
records them beside the device's."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import vine_oracle as vo  # noqa: E402
from vine_robot_isaacgymenvs_amd import abi, load_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.learning.network import ModelA2CContinuousLogStd  # noqa: E402
from vine_robot_isaacgymenvs_amd.tasks.vine5link_moving_base import vine_config_from_cfg  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_policy  # noqa: E402


def configs(M, K, seed=9):
    """``(plant task config, model task config, train.params)`` of the test."""
    cfg = load_config(overrides=["num_envs=%d" % M])
    task = cfg["task"]
    task["seed"] = seed
    task["task"]["vine_randomize"] = False
    weights = {k: 0.0 for k in task["env"] if k.endswith("_REWARD_WEIGHT")}
    weights.update(POSITION_REWARD_WEIGHT=1.0, RAIL_LIMIT_REWARD_WEIGHT=1.0)
    task["env"].update(weights, CREATE_PIPE=False, CREATE_SHELF=False, USE_TARGET_REACHED_RESET=False, ACTION_DELAY=1)
    return task, mpc.model_config(task, M, K, weights), cfg["train"]["params"]


def network(params, width, net_seed):
    torch.manual_seed(net_seed)
    model = ModelA2CContinuousLogStd(params["network"], abi.NUM_ACTIONS, (width,), params["config"].get("normalize_value", False),
                                     params["config"]["normalize_input"])
    return model.double().eval()


def run(M, K, H, steps, sigma, lam, seed, net_seed):
    """One run; returns the summed plant reward, float64 [M]."""
    lib = vo.load("f64")
    task, mtask, params = configs(M, K)
    plant = vo.OracleEnv(vine_config_from_cfg(task, lib, seed=task["seed"]), "f64")
    model = vo.OracleEnv(vine_config_from_cfg(mtask, lib, seed=task["seed"]), "f64")
    net = network(params, plant.num_obs, net_seed)
    clip = float(model.cfg.clip_actions)
    N, plant_of = M * K, np.arange(M * K) // K
    nominal = np.zeros((M, H, 2), np.float32)
    history = np.zeros((M, abi.MAX_DELAY, 2), np.float32)
    tick = np.zeros(M, np.int64)
    plant_h, plant_c = np.zeros((M, 256)), np.zeros((M, 256))
    plant.step(np.zeros((M, 2), np.float32))                  # one plant step on action zero consumes the reset
    total = np.zeros(M)
    for _ in range(steps):
        d = mpc.sample_actions(nominal, sigma, seed, K, tick, clip).reshape(N, H, 2)
        model.state[:] = plant.state[:, plant_of]
        model.progress[:], model.reset_buf[:] = plant.progress[plant_of], 0
        model.step_count = plant.step_count
        h, c = torch.from_numpy(plant_h[plant_of][None]), torch.from_numpy(plant_c[plant_of][None])
        obs = plant.obs[plant_of].copy()
        rews, resets = [], []
        for k in range(H):
            with torch.no_grad():
                res = net({"is_train": False, "prev_actions": None, "obs": torch.from_numpy(obs.astype(np.float64)),
                           "rnn_states": [h, c]})
            h, c = res["rnn_states"]
            mu = res["mus"].numpy().astype(np.float32)
            if k == 0:
                mu0, _, _ = mpc_policy.keep(mu, h[0].numpy(), c[0].numpy(), K, plant.reset_buf)
                plant_h, plant_c = h[0].numpy()[::K].copy(), c[0].numpy()[::K].copy()      # (float64 state; keep's is float32)
                plant_h[plant.reset_buf != 0], plant_c[plant.reset_buf != 0] = 0.0, 0.0
            model.step(mpc_policy.act(mu, d[:, k], clip))
            rews.append(model.rew.copy())
            resets.append(model.reset_buf.copy())
            obs = model.obs.copy()
        cost, _alive = mpc.cost_sums(np.stack(rews), np.stack(resets))
        r = mpc.mpc_replay(nominal, cost, sigma, lam, seed, tick, clip, plant.reset_buf, history)
        nominal, tick = r["nominal"], r["tick"]
        action, history = mpc_policy.compose(mu0, r["plant_actions"], r["history"], clip, plant.reset_buf)
        plant.step(action)
        total += plant.rew.astype(np.float64)
    plant.close()
    model.close()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plants", type=int, default=4)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--lam", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--net-seed", type=int, default=0)
    a = ap.parse_args()
    vo.build()
    alone = run(a.plants, 2, a.horizon, a.steps, 0.0, a.lam, a.seed, a.net_seed)
    planned = run(a.plants, a.samples, a.horizon, a.steps, a.sigma, a.lam, a.seed, a.net_seed)
    print("%d plants, K %d, H %d, %d control steps, sigma %g, lambda %g, seed %d, network seed %d" % (
        a.plants, a.samples, a.horizon, a.steps, a.sigma, a.lam, a.seed, a.net_seed))
    print("summed plant reward, policy alone (sigma 0): %s" % np.array2string(alone, precision=5))
    print("summed plant reward, policy + planning:      %s" % np.array2string(planned, precision=5))
    print("planned / alone (rewards are negative: below 1 is better): %s" % np.array2string(planned / alone, precision=4))
    ok = bool(np.all(planned > alone))
    print("condition (planning higher on every plant): %s" % ("met" if ok else "NOT met"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
