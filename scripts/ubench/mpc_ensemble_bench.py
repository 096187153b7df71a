#!/usr/bin/env python3
"""MPC_ENSEMBLE timings on one MI355X (profiles/mpc_ensemble/node_cost.txt):

    python scripts/ubench/mpc_ensemble_bench.py [plants] [samples] [horizon] [free]
    rocprofv3 --kernel-trace --stats -d <dir> -o ensemble -- python scripts/ubench/mpc_ensemble_bench.py --trace [plants] ...

Without ``--trace``: the whole control step from replayed graphs of the Controller's own capture (host clock around 50 replays
that end in a synchronise; median, minimum and maximum over nine rounds), in control steps per second: the plain controller
on a model without a table (the code this feature does not touch), the plain controller on a model with a DAMPING table bound
(``model_params=``: the table's own price, which the ensemble pays but does not cause), and ``EnsembleController`` with MEMBERS
1, 4 and 8 (RISK entropic, the dearest group cost) on that model.

With ``--trace``: thirty eager control steps of the plain controller and of ``EnsembleController`` with MEMBERS 4, for a kernel
trace: the per-launch times of ``vine_mpc_ensemble_node_kernel`` and ``vine_mpc_ensemble_update_kernel`` beside
``vine_mpc_node_kernel`` and ``vine_mpc_update_kernel`` are read from the trace's kernel statistics, not from events."""
import os
import sys
import time

import numpy as np
import torch

TRACE = "--trace" in sys.argv
sys.argv = [a for a in sys.argv if a != "--trace"]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_bench as base  # noqa: E402  (reads plants, samples, horizon, free from the command line)
from vine_robot_isaacgymenvs_amd import load_task_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_ensemble  # noqa: E402

M, K, H = base.M, base.K, base.H
PARAMS = {"DAMPING": [0.005, 0.1]}


def spec_of(members):
    return {"params": PARAMS, "MEMBERS": members, "RISK": "entropic", "THETA": 0.5}


def ensemble(plant, model, members, **kw):
    c = mpc_ensemble.EnsembleController(plant, model, K, spec_of(members), H, **kw)
    c.set_members(mpc_ensemble.draw_members(PARAMS, model._vcfg, model._lib, 43, M, members))
    return c


def main():
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % M])
    cfg["seed"] = 42
    if base.FREE:
        cfg["env"].update(CREATE_PIPE=False, CREATE_SHELF=False)
    plant = mpc.make_task(cfg)
    bare = mpc.make_task(mpc.model_config(cfg, M, K))
    mcfg = mpc.model_config(cfg, M, K)
    mcfg["env"]["ENV_PARAMS"] = dict(PARAMS)
    model = mpc.make_task(mcfg)
    print("%s, %d plants x %d samples = %d model envs, horizon %d, model step kernel %s without a table, %s with one" % (
        torch.cuda.get_device_name(0), M, K, M * K, H, bare.step_kernel_name, model.step_kernel_name), flush=True)
    if TRACE:
        for c in (mpc.Controller(plant, bare, K, H, graph=False), ensemble(plant, model, 4, graph=False)):
            for _ in range(30):
                c.control_step()
            torch.cuda.synchronize()
        print("30 eager control steps each of the plain controller and of MEMBERS 4: read the kernel statistics", flush=True)
    else:
        rounds, n, med = 9, 50, {}
        tabled = lambda: mpc.Controller(plant, model, K, H)      # noqa: E731
        for name, make in (("plain, no table", lambda: mpc.Controller(plant, bare, K, H)), ("plain, DAMPING table", tabled),
                           ("ensemble MEMBERS 1", lambda: ensemble(plant, model, 1)),
                           ("ensemble MEMBERS 4", lambda: ensemble(plant, model, 4)),
                           ("ensemble MEMBERS 8", lambda: ensemble(plant, model, 8))):
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
            print("%-22s %d rounds of %d replayed control steps: median %.1f us per control step (min %.1f, max %.1f) = %.1f control "
                  "steps/s; launches per control step %d" % (name, rounds, n, med[name], min(us), max(us), 1e6 / med[name],
                                                             sum(c.graph_launches.values())), flush=True)
        for name in list(med)[2:]:
            print("%s / plain, DAMPING table : %.4f (+%.1f us);  / plain, no table : %.4f" % (
                name, med[name] / med["plain, DAMPING table"], med[name] - med["plain, DAMPING table"], med[name] / med["plain, no table"]),
                flush=True)
    for t in (model, bare, plant):
        t.close()


if __name__ == "__main__":
    main()
