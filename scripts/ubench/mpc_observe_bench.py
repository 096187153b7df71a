#!/usr/bin/env python3
"""MPC_OBSERVE timings on one MI355X (profiles/mpc_observe/timings.txt):  python scripts/ubench/mpc_observe_bench.py [plants] [samples] [horizon] [catchup]

In the manner of scripts/ubench/mpc_bench.py: per-launch durations from replayed hipGraphs of 20 launches each, device events
around the replays -- the three launches of include/vine_mpc_observe.h (the measurement of a noisy and of a noise-free table,
the pin, the catch-up node on a step that counts and on one that does not) and the predictor's M-wide step -- then the whole
control step of an ObservingController (catch-up C, delay C, compensated) beside the plain Controller's on the same plants
(what the commit before the feature runs), in control steps per second (host clock around replays that end in a synchronise).
Free space.  The expectation to confirm or refute: C x two latency-sized M-wide launches on top of today's control step."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vine_robot_isaacgymenvs_amd import load_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_observe  # noqa: E402

M = int(sys.argv[1]) if len(sys.argv) > 1 else 64
K = int(sys.argv[2]) if len(sys.argv) > 2 else 256
H = int(sys.argv[3]) if len(sys.argv) > 3 else 20
C = int(sys.argv[4]) if len(sys.argv) > 4 else 3
LAUNCHES, REPLAYS = 20, 20


def graph_of(body):
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(LAUNCHES):
            body()
    return g


def per_launch_us(g):
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPLAYS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / LAUNCHES)
    return np.median(out), min(out), max(out)


def best_run_us(c, n, rounds=5):
    best = 1e9
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.run(n)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best / n * 1e6


def main():
    cfg = load_config(overrides=["num_envs=%d" % M])
    task = cfg["task"]
    task["seed"] = 42
    task["env"].update(CREATE_PIPE=False, CREATE_SHELF=False)
    plant = mpc.make_task(task)
    model = mpc.make_task(mpc.model_config(task, M, K))
    predictor = mpc.make_task(mpc.model_config(task, M, 1))
    observe = {"DELAY": C, "CATCHUP": C, "HOLD": 0.1, "NOISE_Q": 0.002, "NOISE_QD": 0.01}
    ctl = mpc_observe.ObservingController(plant, model, predictor, K, observe, H, graph=False)
    quiet = mpc_observe.ObservingController(plant, model, predictor, K, {"DELAY": C, "CATCHUP": C}, H, graph=False)
    print("%s, %d plants x %d samples = %d model envs, horizon %d, catch-up %d, predictor step kernel %s" % (
        torch.cuda.get_device_name(0), M, K, M * K, H, C, predictor.step_kernel_name))
    plant.step_into(ctl.plant_actions, ctl.plant_obs)
    for _ in range(C + 2):                               # (eager: every lazy initialisation done, the episodes C steps old)
        ctl.control_step()
    quiet.fresh.zero_()
    quiet.age.fill_(C)
    # (name, launch, the age every plant's episode has while it is timed)
    rows = [("measure (noise on q and qd)", ctl.measure, C), ("measure (no noise)", quiet.measure, C), ("pin", ctl.pin, C),
            ("predictor step (%d envs)" % M, lambda: predictor.step_into(ctl.predictor_actions, ctl.predictor_obs), C)]
    if C:
        rows += [("catchup, i = C (a step that counts)", lambda: ctl.catchup(C), C),
                 ("catchup, i = 1, age 0 (pinned again)", lambda: ctl.catchup(1), 0)]
    for name, fn, age in rows:
        g = graph_of(fn)
        ctl.age.fill_(age)                               # (the measurement moves it on: the others read what stands here)
        print("%-38s median %.2f us per launch (min %.2f, max %.2f) over %d replays of %d" % (name, *per_launch_us(g), REPLAYS, LAUNCHES))
    n = 50
    out = []
    for name, c in (("Controller (no observe)", mpc.Controller(plant, model, K, H)),
                    ("ObservingController, C = %d" % C, mpc_observe.ObservingController(plant, model, predictor, K, observe, H)),
                    ("ObservingController, C = 0", mpc_observe.ObservingController(plant, model, predictor, K, {"HOLD": 0.1}, H))):
        c.run(2)
        us = best_run_us(c, n)
        out.append(us)
        print("%-34s %d control steps (hipGraph replay, best of 5): %.1f us per control step = %.1f control steps/s" % (
            name, n, us, 1e6 / us))
    print("observe= adds %.1f us per control step with C = %d (%.1f us per catch-up step beyond C = 0), %.1f us with C = 0" % (
        out[1] - out[0], C, (out[1] - out[2]) / max(C, 1), out[2] - out[0]))
    predictor.close()
    model.close()
    plant.close()


if __name__ == "__main__":
    main()
