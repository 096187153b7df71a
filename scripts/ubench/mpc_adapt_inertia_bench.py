#!/usr/bin/env python3
"""MPC_ADAPT masses timings on one MI355X (profiles/mpc_adapt_inertia/timings.txt):
python scripts/ubench/mpc_adapt_inertia_bench.py [plants] [samples] [horizon] [free]

Per-launch durations from replayed hipGraphs of `horizon` launches each, device events around the replays (the method of
scripts/ubench/mpc_bench.py, whose helpers this imports): the base pin and estimate beside the two launches of
include/vine_mpc_adapt_inertia.h; then one cycle (W = E = 8) from replayed graphs, ``AdaptiveController`` beside
``AdaptiveInertiaController`` with one and with three mass dimensions, both tables bound to the model on every side, each as the
median, minimum and maximum over rounds of 10 cycles."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_bench as base  # noqa: E402  (reads plants, samples, horizon, free from the command line)
from vine_robot_isaacgymenvs_amd import load_task_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_adapt, mpc_adapt_inertia  # noqa: E402

M, K, H = base.M, base.K, base.H
W = E = 8


def main():
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % M])
    cfg["seed"] = 42
    if base.FREE:
        cfg["env"].update(CREATE_PIPE=False, CREATE_SHELF=False)
    cfg["env"]["ENV_PARAMS"] = {"DAMPING": [0.005, 0.1], "LINK_MASS": [0.7, 1.4]}
    plant = mpc.make_task(cfg)
    mcfg = mpc.model_config(cfg, M, K)
    mcfg["env"]["ENV_PARAMS"] = {"FPAM_K": 1.0, "LINK_MASS": 1.0}              # both tables, the configuration's own rows
    model = mpc.make_task(mcfg)
    print("%s, %d plants x %d samples = %d model envs, horizon %d, window %d, every %d; model step kernel %s" % (
        torch.cuda.get_device_name(0), M, K, M * K, H, W, E, model.step_kernel_name))
    params = {"params": {"DAMPING": [0.005, 0.1]}, "window": W, "every": E}
    one = dict(params, masses={"LINK_MASS": [0.7, 1.4]})
    three = dict(params, masses={"CART_MASS": [0.2, 0.8], "LINK_MASS": [0.7, 1.4], "TIP_LINK_MASS": [0.7, 1.6]})
    line = "%-44s median %.2f us per launch (min %.2f, max %.2f) over %d replays of %d"
    for name, spec in (("one mass dimension", one), ("three mass dimensions", three)):
        ctl = mpc_adapt_inertia.AdaptiveInertiaController(plant, model, K, spec, H)
        plant.step_into(ctl.plant_actions, ctl.plant_obs)
        ctl.run(2 * E)                                   # (two captured cycles: every lazy initialisation done)
        ctl.graph = None
        print(line % ("pin, include/vine_mpc_adapt.h", *base.per_launch_us(base.graph_of(lambda: mpc_adapt.AdaptiveController.pin(ctl))),
                      base.REPLAYS, H))
        print(line % ("inertia pin, " + name, *base.per_launch_us(base.graph_of(ctl.inertia_pin)), base.REPLAYS, H))
        print(line % ("estimate, include/vine_mpc_adapt.h",
                      *base.per_launch_us(base.graph_of(lambda: mpc_adapt.AdaptiveController.estimate(ctl))), base.REPLAYS, H))
        print(line % ("inertia estimate, " + name, *base.per_launch_us(base.graph_of(ctl.inertia_estimate)), base.REPLAYS, H))
    rounds, n, med = 9, 10 * E, {}
    for name, make in (("AdaptiveController", lambda: mpc_adapt.AdaptiveController(plant, model, K, params, H)),
                       ("masses: LINK_MASS", lambda: mpc_adapt_inertia.AdaptiveInertiaController(plant, model, K, one, H)),
                       ("masses: all three", lambda: mpc_adapt_inertia.AdaptiveInertiaController(plant, model, K, three, H))):
        c = make()
        c.run(2 * E)
        us = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.run(n)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / n * 1e6 * E)
        med[name] = np.median(us)
        print("%-22s %d rounds of %d replayed cycles: median %.1f us per cycle of %d control steps (min %.1f, max %.1f); launches "
              "per cycle %d" % (name, rounds, n // E, med[name], E, min(us), max(us), sum(c.graph_launches.values())))
    for name in list(med)[1:]:
        print("%s / AdaptiveController : %.4f (+%.1f us per cycle)" % (
            name, med[name] / med["AdaptiveController"], med[name] - med["AdaptiveController"]))
    model.close()
    plant.close()


if __name__ == "__main__":
    main()
