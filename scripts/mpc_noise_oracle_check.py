#!/usr/bin/env python3
"""MPC_NOISE on the CPU: do correlated samples and an adapted sigma pay?  The experiment an "it matters" GPU test would run, with
the float64 oracle for the plants and the samples and the numpy statements of utils/mpc.py (``cost_sums``) and
utils/mpc_noise.py (``colored_deviate``, ``colored_actions``, ``noise_replay``) for everything else.  No GPU is needed.

  python scripts/mpc_noise_oracle_check.py                       # (4, 64, 12), 60 control steps
  python scripts/mpc_noise_oracle_check.py --steps 80 --sigma 0.3

Section 24's "it controls" setting: free space, POSITION_REWARD_WEIGHT and RAIL_LIMIT_REWARD_WEIGHT 1 and every other weight 0
on both handles, no target-reached reset, ACTION_DELAY 1, sigma 0.5, lambda 0.05, one plant step on action zero first.  The
controller runs with BETA in {0, 0.5, 0.8, 0.95} without ADAPT and then with it, on the same plants and seed.  Prints the summed
plant reward per plant and setting, and the final sigma per plant with ADAPT.  profiles/mpc_noise/it_matters_oracle.txt records
what it gave."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import vine_oracle as vo  # noqa: E402
from vine_robot_isaacgymenvs_amd import abi, load_task_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.tasks.vine5link_moving_base import vine_config_from_cfg  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_noise  # noqa: E402

f32 = np.float32
BETAS = (0.0, 0.5, 0.8, 0.95)


def config(n, seed):
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % n])
    cfg["seed"] = seed
    cfg["task"]["vine_randomize"] = False
    weights = {k: 0.0 for k in cfg["env"] if k.endswith("_REWARD_WEIGHT")}
    weights.update(POSITION_REWARD_WEIGHT=1.0, RAIL_LIMIT_REWARD_WEIGHT=1.0)
    cfg["env"].update(weights, CREATE_PIPE=False, CREATE_SHELF=False, USE_TARGET_REACHED_RESET=False, ACTION_DELAY=1)
    return vine_config_from_cfg(cfg, vo.load("f64"), seed=seed)


def run(beta, adapt, a):
    """Returns the summed plant reward, float64 [M], and the final sigma_p [M, 2]."""
    M, K, H = a.plants, a.samples, a.horizon
    pcfg, mcfg = config(M, a.seed), config(M * K, a.seed)
    plant, model = vo.OracleEnv(pcfg, "f64"), vo.OracleEnv(mcfg, "f64")
    clip = float(mcfg.clip_actions)
    plant.step(np.zeros((M, 2), f32))                         # one plant step on action zero: consumes the first reset
    nominal = np.zeros((M, H, 2), f32)
    history = np.zeros((M, abi.MAX_DELAY, 2), f32)
    tick = np.zeros(M, np.int64)
    sigma_p = np.full((M, 2), a.sigma, f32)
    total = np.zeros(M)
    plant_of = np.arange(M * K) // K
    for _ in range(a.steps):
        model.state[:] = plant.state[:, plant_of]             # the fork (ACTION_DELAY 1 on both: one ring slot, copied with the rest)
        model.progress[:], model.reset_buf[:] = plant.progress[plant_of], 0
        model.step_count = plant.step_count
        eps = mpc_noise.colored_deviate(a.seed, M, K, tick, H, beta)
        u = mpc_noise.colored_actions(nominal, sigma_p, eps, clip)
        rews, raised = [], []
        for k in range(1, H + 1):
            model.step(u[:, :, k - 1].reshape(M * K, 2))
            rews.append(model.rew.copy())
            raised.append(model.reset_buf.copy())
        cost, _ = mpc.cost_sums(np.stack(rews), np.stack(raised))
        r = mpc_noise.noise_replay(nominal, cost, a.sigma, a.lam, a.seed, tick, clip, beta, sigma_p=sigma_p, adapt=adapt,
                                   plant_reset=plant.reset_buf, history=history, eps=eps)
        nominal, history, tick, sigma_p = r["nominal"], r["history"], r["tick"], r["sigma"]
        plant.step(r["plant_actions"])
        total += plant.rew
    plant.close()
    model.close()
    return total, sigma_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plants", type=int, default=4)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--lam", type=float, default=0.05)
    ap.add_argument("--rate", type=float, default=0.2)
    ap.add_argument("--sigma-min", dest="sigma_min", type=float, default=0.05)
    ap.add_argument("--sigma-max", dest="sigma_max", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    vo.build()
    adapt = mpc_noise.noise_config({"BETA": 0.0, "ADAPT": {"RATE": a.rate, "SIGMA_MIN": a.sigma_min, "SIGMA_MAX": a.sigma_max}})["ADAPT"]
    print("(%d, %d, %d), %d control steps, sigma %g, lambda %g, seed %d; ADAPT %s" % (
        a.plants, a.samples, a.horizon, a.steps, a.sigma, a.lam, a.seed, adapt))
    totals = {}
    for ad in (None, adapt):
        for beta in BETAS:
            total, sigma_p = totals[(beta, ad is not None)] = run(beta, ad, a)
            print("summed plant reward, BETA %-4g %s %s  sum %.4f%s" % (
                beta, "ADAPT" if ad else "fixed", np.array2string(total, precision=4), total.sum(),
                "  final sigma rail %s fpam %s" % (np.array2string(sigma_p[:, 0], precision=3), np.array2string(sigma_p[:, 1], precision=3))
                if ad else ""), flush=True)
    base = totals[(0.0, False)][0]
    for (beta, ad), (total, _) in totals.items():
        if (beta, ad) != (0.0, False):
            better = total > base
            print("BETA %-4g %s against BETA 0 fixed: better on %d of %d plants %s, sum ratio %.4f (the sums are negative: below 1 "
                  "is better)" % (beta, "ADAPT" if ad else "fixed", better.sum(), len(base), better.astype(int), total.sum() / base.sum()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
