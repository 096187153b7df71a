#!/usr/bin/env python3
"""MPC_FILTER timings on one MI355X (profiles/mpc_filter/timings.txt):  python scripts/ubench/mpc_filter_bench.py [plants] [samples] [horizon] [catchup]

In the manner of scripts/ubench/mpc_observe_bench.py: per-launch durations from replayed hipGraphs of 20 launches each, device
events around the replays -- the two launches of include/vine_mpc_filter.h (the pin on plants that advance, the correction where
the estimate is in place, where every plant blends and where every frame is an episode's first, and the three launches a
control step adds in sequence) and the predictor's M-wide step -- then the whole control
step of a FilteringController beside the ObservingController's and the plain Controller's on the same plants, in control
steps per second (host clock around replays that end in a synchronise).  Free space.  The expectation to confirm or refute:
one more latency-sized predictor step plus two M-wide launches on top of the observing controller's control step."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vine_robot_isaacgymenvs_amd import load_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_filter, mpc_observe  # noqa: E402

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
    gains = {"GAIN_Q": 0.3, "GAIN_QD": 0.3}
    ctl = mpc_filter.FilteringController(plant, model, predictor, K, observe, gains, H, graph=False)
    print("%s, %d plants x %d samples = %d model envs, horizon %d, catch-up %d, predictor step kernel %s" % (
        torch.cuda.get_device_name(0), M, K, M * K, H, C, predictor.step_kernel_name))
    plant.step_into(ctl.plant_actions, ctl.plant_obs)
    for _ in range(C + 3):                               # (eager: every lazy initialisation done, every plant has an estimate)
        ctl.control_step()
    torch.cuda.synchronize()
    steps = int(plant.step_count)
    # what a launch finds while it is timed: est_index (the correction moves it on, so each case is pinned by the state it reads)
    advancing = lambda: (ctl.age.fill_(C + 1), ctl.est_index.fill_(steps - 1 - C - 1), ctl.fresh.zero_())          # noqa: E731
    first = lambda: ctl.age.fill_(0)                                                             # noqa: E731
    behind = steps - 1 - C - 1

    def blend():                                         # est_index put back in front of every correction: each one advances
        ctl.est_index.fill_(behind)
        ctl.filter_correct()

    def front():                                         # what a control step issues in front of the observe pin
        ctl.est_index.fill_(behind)
        ctl.advance()

    rows = [("filter pin (every plant advances)", ctl.filter_pin, advancing),
            ("predictor step (%d envs)" % M, lambda: predictor.step_into(ctl.predictor_actions, ctl.predictor_obs), advancing),
            ("filter correct (first launch blends, the rest find their estimate)", ctl.filter_correct, advancing),
            ("est_index fill alone (to be taken off the next two rows)", lambda: ctl.est_index.fill_(behind), advancing),
            ("fill + filter correct (every launch blends; HOLD 0.1)", blend, advancing),
            ("fill + pin + predictor step + correct (every launch blends)", front, advancing),
            ("filter correct (an episode's first frame: nine slots)", ctl.filter_correct, first)]
    for name, fn, prepare in rows:
        g = graph_of(fn)
        prepare()
        print("%-68s median %.2f us per launch (min %.2f, max %.2f) over %d replays of %d" % (name, *per_launch_us(g), REPLAYS, LAUNCHES))
    n = 50
    out = []
    for name, c in (("Controller (no observe)", mpc.Controller(plant, model, K, H)),
                    ("ObservingController, C = %d" % C, mpc_observe.ObservingController(plant, model, predictor, K, observe, H)),
                    ("FilteringController, C = %d" % C, mpc_filter.FilteringController(plant, model, predictor, K, observe, gains, H)),
                    ("FilteringController, C = 0", mpc_filter.FilteringController(plant, model, predictor, K, {"HOLD": 0.1, "NOISE_Q": 0.002},
                                                                                   gains, H))):
        c.run(2)
        us = best_run_us(c, n)
        out.append(us)
        print("%-34s %d control steps (hipGraph replay, best of 5): %.1f us per control step = %.1f control steps/s" % (
            name, n, us, 1e6 / us))
    print("filter= adds %.1f us per control step to observe= with C = %d; observe= and filter= together add %.1f us with C = %d and "
          "%.1f us with C = 0" % (out[2] - out[1], C, out[2] - out[0], C, out[3] - out[0]))
    # how often the nine-slot path is taken in such a run: control steps in which some plant's frame is an episode's first
    count = mpc_filter.FilteringController(plant, model, predictor, K, observe, gains, H, graph=False)
    firsts, total = 0, 5 * n
    count.run(2)
    for _ in range(total):
        count.run(1)
        firsts += int(bool((count.age == 0).any()))
    print("%d of %d control steps had a plant whose frame was its episode's first (the correction's nine-slot path)" % (firsts, total))
    predictor.close()
    model.close()
    plant.close()


if __name__ == "__main__":
    main()
