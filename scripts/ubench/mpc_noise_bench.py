#!/usr/bin/env python3
"""MPC_NOISE timings on one MI355X (profiles/mpc_noise/timings.txt):  python scripts/ubench/mpc_noise_bench.py [plants] [samples] [horizon] [free]

Per-launch durations from replayed hipGraphs of `horizon` launches each, device events around the replays (the method of
scripts/ubench/mpc_bench.py, whose helpers this imports): the draw; the base update and the update of
include/vine_mpc_noise.h without and with ADAPT; the noise node inside a window, as the difference of step + node + noise node
and step + node; then the whole control step from replayed graphs, the plain controller beside ``noise={BETA: 0.8}`` and
``noise={BETA: 0.8, ADAPT: {}}`` on the same tasks, each as the median, minimum and maximum over rounds of 50 replays."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_bench as base  # noqa: E402  (reads plants, samples, horizon, free from the command line)
from vine_robot_isaacgymenvs_amd import load_task_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_noise  # noqa: E402

M, K, H = base.M, base.K, base.H


def main():
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % M])
    cfg["seed"] = 42
    if base.FREE:
        cfg["env"].update(CREATE_PIPE=False, CREATE_SHELF=False)
    plant = mpc.make_task(cfg)
    model = mpc.make_task(mpc.model_config(cfg, M, K))
    print("%s, %d plants x %d samples = %d model envs, horizon %d, model step kernel %s" % (
        torch.cuda.get_device_name(0), M, K, M * K, H, model.step_kernel_name))
    fixed, adapt = {"BETA": 0.8}, {"BETA": 0.8, "ADAPT": {}}
    plain = mpc.Controller(plant, model, K, H, graph=False)
    ctl = mpc_noise.NoiseController(plant, model, K, fixed, H, graph=False)
    actl = mpc_noise.NoiseController(plant, model, K, adapt, H, graph=False)
    plant.step_into(ctl.plant_actions, ctl.plant_obs)
    for c in (plain, ctl, actl):
        c.control_step()                                 # (eager: every lazy initialisation done)
    line = "%-34s median %.2f us per launch (min %.2f, max %.2f) over %d replays of %d"
    print(line % ("draw", *base.per_launch_us(base.graph_of(ctl.draw)), base.REPLAYS, H))
    print(line % ("update, include/vine_mpc.h", *base.per_launch_us(base.graph_of(plain.update)), base.REPLAYS, H))
    print(line % ("update, noise", *base.per_launch_us(base.graph_of(ctl.update)), base.REPLAYS, H))
    print(line % ("update, noise with ADAPT", *base.per_launch_us(base.graph_of(actl.update)), base.REPLAYS, H))
    print(line % ("noise node outside a window", *base.per_launch_us(base.graph_of(ctl.noise_node)), base.REPLAYS, H))
    s = base.per_launch_us(base.graph_of(lambda: mpc.Controller.model_step(ctl)), ctl.fork)
    b = base.per_launch_us(base.graph_of(ctl.model_step), ctl.fork)
    print("step + node %.2f us, step + node + noise node %.2f us inside a window: noise node = %.2f us" % (s[0], b[0], b[0] - s[0]))
    rounds, n, med = 9, 50, {}
    for name, make in (("without noise=", lambda: mpc.Controller(plant, model, K, H)),
                       ("noise={BETA: 0.8}", lambda: mpc_noise.NoiseController(plant, model, K, fixed, H)),
                       ("noise={BETA: 0.8, ADAPT: {}}", lambda: mpc_noise.NoiseController(plant, model, K, adapt, H))):
        c = make()
        c.run(4)
        us = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.run(n)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / n * 1e6)
        med[name] = np.median(us)
        print("%-30s %d rounds of %d replayed control steps: median %.1f us per control step (min %.1f, max %.1f); launches per "
              "control step %d" % (name, rounds, n, med[name], min(us), max(us), sum(c.graph_launches.values())))
    for name in list(med)[1:]:
        print("%s / without noise= : %.4f (+%.1f us)" % (name, med[name] / med["without noise="], med[name] - med["without noise="]))
    model.close()
    plant.close()


if __name__ == "__main__":
    main()
