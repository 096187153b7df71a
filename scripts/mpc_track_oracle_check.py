#!/usr/bin/env python3
"""MPC_TRACK on the CPU: does tracking pay?  The experiment an "it tracks" GPU test would run, with the float64 oracle for the
plants and the samples and the numpy statements of utils/mpc.py (``sample_actions``, ``mpc_replay``), utils/mpc_track.py
(``plan_replay``, ``node_replay``) and utils/env_target.py (``advance``) for everything else.  No GPU is needed.

  python scripts/mpc_track_oracle_check.py                       # (4, 64, 12), 60 control steps
  python scripts/mpc_track_oracle_check.py --vel 0.1 --span 0.05 --steps 80

Free space, POSITION_REWARD_WEIGHT 1 and every other weight 0 on both handles, no target-reached reset, ACTION_DELAY 1.  Every
plant's target moves along +-y at ``--vel`` m/s (the sign alternates over the plants) over ``--span``; the controller runs
without tracking, with the ``linear`` and with the ``exact`` path on the same plants, seed and noise.  Prints the summed plant
reward per plant and kind and their ratios.  profiles/mpc_track/it_tracks_oracle.txt records what it gave: no clear margin,
which is why tests/test_mpc_track_gpu.py has no such test."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import vine_oracle as vo  # noqa: E402
from vine_robot_isaacgymenvs_amd import abi, load_task_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.tasks.vine5link_moving_base import vine_config_from_cfg  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import env_target, mpc, mpc_track  # noqa: E402

F = abi
f32 = np.float32


def config(n, seed):
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % n])
    cfg["seed"] = seed
    cfg["task"]["vine_randomize"] = False
    weights = {k: 0.0 for k in cfg["env"] if k.endswith("_REWARD_WEIGHT")}
    weights["POSITION_REWARD_WEIGHT"] = 1.0
    cfg["env"].update(weights, CREATE_PIPE=False, CREATE_SHELF=False, USE_TARGET_REACHED_RESET=False, ACTION_DELAY=1)
    return vine_config_from_cfg(cfg, vo.load("f64"), seed=seed)


def run(kind, a):
    """``kind``: ``None`` (no tracking) or a name of ``mpc_track.PATHS``.  Returns the summed plant reward, float64 [M], and the
    number of resets the plants consumed in the run."""
    M, K, H = a.plants, a.samples, a.horizon
    pcfg, mcfg = config(M, a.seed), config(M * K, a.seed)
    plant, model = vo.OracleEnv(pcfg, "f64"), vo.OracleEnv(mcfg, "f64")
    cdt = env_target.control_period(pcfg.dt, pcfg.control_freq_inv)
    clip = float(mcfg.clip_actions)
    plant.step(np.zeros((M, 2), f32))                         # consumes the reset every env starts with: the anchor
    motion = np.zeros((F.VTM_COUNT, M), f32)
    motion[F.VTM_ANCHOR_Y], motion[F.VTM_ANCHOR_Z] = plant.state[F.VF_TARGET_Y], plant.state[F.VF_TARGET_Z]
    motion[F.VTM_AXIS_C] = 1.0
    table = np.zeros((F.VTG_NAMES, M), f32)
    table[F.VTG_VEL_ALONG] = f32(a.vel) * np.where(np.arange(M) % 2 == 0, 1, -1)
    table[F.VTG_VEL_ACROSS] = f32(a.vel_across) * np.where(np.arange(M) % 4 < 2, 1, -1)
    table[F.VTG_SPAN_ALONG], table[F.VTG_SPAN_ACROSS] = a.span, a.span
    motion[F.VTM_VEL_ALONG], motion[F.VTM_VEL_ACROSS] = table[F.VTG_VEL_ALONG], table[F.VTG_VEL_ACROSS]
    resets = [0]

    def move_target():                                        # the observer's launch behind a plant step (every plant moves)
        first = np.flatnonzero(plant.progress == 0)           # the step consumed a reset: the target is the reset's own
        if len(first):
            resets[0] += len(first)
            motion[F.VTM_ANCHOR_Y, first], motion[F.VTM_ANCHOR_Z, first] = plant.state[F.VF_TARGET_Y, first], plant.state[F.VF_TARGET_Z, first]
            motion[F.VTM_OFF_ALONG, first] = motion[F.VTM_OFF_ACROSS, first] = 0.0
            motion[F.VTM_VEL_ALONG, first], motion[F.VTM_VEL_ACROSS, first] = table[F.VTG_VEL_ALONG, first], table[F.VTG_VEL_ACROSS, first]
        oa, va, _ = env_target.advance(motion[F.VTM_OFF_ALONG], motion[F.VTM_VEL_ALONG], table[F.VTG_SPAN_ALONG], cdt)
        oc, vc, _ = env_target.advance(motion[F.VTM_OFF_ACROSS], motion[F.VTM_VEL_ACROSS], table[F.VTG_SPAN_ACROSS], cdt)
        motion[F.VTM_OFF_ALONG], motion[F.VTM_VEL_ALONG], motion[F.VTM_OFF_ACROSS], motion[F.VTM_VEL_ACROSS] = oa, va, oc, vc
        plant.state[F.VF_TARGET_Y] = motion[F.VTM_ANCHOR_Y] + oa
        plant.state[F.VF_TARGET_Z] = motion[F.VTM_ANCHOR_Z] + oc

    move_target()
    nominal = np.zeros((M, H, 2), f32)
    history = np.zeros((M, F.MAX_DELAY, 2), f32)
    tick = np.zeros(M, np.int64)
    total = np.zeros(M)
    plant_of = np.arange(M * K) // K
    for _ in range(a.steps):
        if kind is not None:
            plan = mpc_track.plan_replay(F.TARGET_FREE, kind, cdt, H, plant.state.astype(f32), motion, table, np.zeros(M, np.uint8),
                                         plant.reset_buf)
        model.state[:] = plant.state[:, plant_of]             # the fork (ACTION_DELAY 1 on both: one ring slot, copied with the rest)
        model.progress[:], model.reset_buf[:] = plant.progress[plant_of], 0
        model.step_count = plant.step_count
        u = mpc.sample_actions(nominal, a.sigma, a.seed, K, tick, clip)
        rews, raised = [], []
        alive = np.ones(M * K, np.uint8)
        for k in range(1, H + 1):
            model.step(u[:, :, k - 1].reshape(M * K, 2))
            rews.append(model.rew.copy())
            raised.append(model.reset_buf.copy())
            alive &= (model.reset_buf == 0).astype(np.uint8)
            if kind is not None:
                model.state[:] = mpc_track.node_replay(F.TARGET_FREE, K, k, model.state.astype(f32), alive, plan["path"], plan["live"])
        cost, _ = mpc.cost_sums(np.stack(rews), np.stack(raised))
        r = mpc.mpc_replay(nominal, cost, a.sigma, a.lam, a.seed, tick, clip, plant.reset_buf, history)
        nominal, history, tick = r["nominal"], r["history"], r["tick"]
        plant.step(r["plant_actions"])
        move_target()
        total += plant.rew
    plant.close()
    model.close()
    return total, resets[0] - M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plants", type=int, default=4)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--lam", type=float, default=0.05)
    ap.add_argument("--vel", type=float, default=0.2)
    ap.add_argument("--vel-across", dest="vel_across", type=float, default=0.0)
    ap.add_argument("--span", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    vo.build()
    totals = {kind: run(kind, a) for kind in (None, "linear", "exact")}
    print("(%d, %d, %d), %d control steps, sigma %g, lambda %g; VEL_ALONG +-%g, VEL_ACROSS +-%g, SPAN %g" % (
        a.plants, a.samples, a.horizon, a.steps, a.sigma, a.lam, a.vel, a.vel_across, a.span))
    for kind, (total, count) in totals.items():
        print("summed plant reward, %-11s %s  sum %.4f  (%d resets)" % (
            "no tracking" if kind is None else kind, np.array2string(total, precision=3), total.sum(), count))
    base = totals[None][0].sum()
    for kind in ("linear", "exact"):
        print("%s / no tracking: %.4f (both sums are negative: below 1 is better)" % (kind, totals[kind][0].sum() / base))
    return 0


if __name__ == "__main__":
    sys.exit(main())
