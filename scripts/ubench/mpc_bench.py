#!/usr/bin/env python3
"""MPC timings on one MI355X (profiles/mpc/timings.txt):  python scripts/ubench/mpc_bench.py [plants] [samples] [horizon] [free]
                                   (profiles/mpc_adapt/timings.txt):  ... mpc_bench.py --adapt [plants] [samples] [horizon] [free]

Per-launch durations from replayed hipGraphs of `horizon` launches each, device events around the replays: the model's step
alone, the step with the scoring node behind it (the difference is the node), the fork and the update; then the whole
control step (fork, horizon x (step + node), update, plant step) as the Controller captures it, in control steps per second
(host clock around replays that end in a synchronise), beside `horizon` bare model steps.  `free`: free space (the
four-lane step kernel) instead of the task's pipe.

`--track` (profiles/mpc_track/node_cost.txt): plants with a moving target (VEL_ALONG 0, +-0.1, +-0.4 over a SPAN of 0.05 m); the
whole control step from replayed graphs, without `track=` and with `held`, `linear` and `exact` on the same tree, each as
the median, minimum and maximum over rounds of 50 replays; and the plan and the track node alone, per launch.

`--adapt`: the five launches of include/vine_mpc_adapt.h instead (W = E = 8, DAMPING adapted), each from a replayed graph of
`horizon` launches, and one whole cycle of the AdaptiveController beside E control steps of a Controller without a table (what
the commit before the feature runs) and of a Controller whose model has a table bound (the one-lane step kernel: the table's
own price, which adaptation pays but does not cause)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vine_robot_isaacgymenvs_amd import load_task_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import mpc  # noqa: E402

ADAPT = "--adapt" in sys.argv
TRACK = "--track" in sys.argv
sys.argv = [a for a in sys.argv if a not in ("--adapt", "--track")]
M = int(sys.argv[1]) if len(sys.argv) > 1 else 64
K = int(sys.argv[2]) if len(sys.argv) > 2 else 256
H = int(sys.argv[3]) if len(sys.argv) > 3 else 20
FREE = len(sys.argv) > 4 and sys.argv[4] == "free"
REPLAYS = 20


def graph_of(body):
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(H):
            body()
    return g


def per_launch_us(g, before=None):
    for _ in range(3):
        if before:
            before()
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPLAYS):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / H)
    return np.median(out), min(out), max(out)


def best_run_us(c, n, rounds=5):
    """Microseconds per control step of c.run(n), best of `rounds` (host clock around runs that end in a synchronise)."""
    best = 1e9
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.run(n)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best / n * 1e6


def adapt_main():
    from vine_robot_isaacgymenvs_amd.utils import mpc_adapt
    W = E = 8
    spec = {"params": {"DAMPING": [0.005, 0.1]}, "window": W, "every": E}
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % M])
    cfg["seed"] = 42
    if FREE:
        cfg["env"].update(CREATE_PIPE=False, CREATE_SHELF=False)
    plant = mpc.make_task(cfg)
    bare_model = mpc.make_task(mpc.model_config(cfg, M, K))
    tcfg = mpc.model_config(cfg, M, K)
    tcfg["env"]["ENV_PARAMS"] = {"FPAM_K": 1.0}
    model = mpc.make_task(tcfg)
    ctl = mpc_adapt.AdaptiveController(plant, model, K, spec, H)
    print("%s, %d plants x %d samples = %d model envs, horizon %d, window %d, every %d; model step kernel %s (no table: %s)" % (
        torch.cuda.get_device_name(0), M, K, M * K, H, W, E, model.step_kernel_name, bare_model.step_kernel_name))
    plant.step_into(ctl.plant_actions, ctl.plant_obs)
    ctl.run(2 * E)                                       # (two captured cycles: every lazy initialisation done)
    ctl.graph = None
    launches = (("anchor", ctl.anchor, None), ("trace node", ctl.trace, None), ("pin", ctl.pin, None),
                ("score node in a window", ctl.score, "window"), ("score node outside one", ctl.score, None),
                ("estimate", ctl.estimate, None))
    for name, fn, mode in launches:
        g = graph_of(fn)
        if mode == "window":                             # every replay of H = 20 nodes must see k = 1 .. W: step the model too
            def body():
                model.step_into(ctl.actions, ctl.model_obs)
                ctl.score()
            steps = graph_of(lambda: model.step_into(ctl.actions, ctl.model_obs))
            s = per_launch_us(steps, ctl.pin)
            b = per_launch_us(graph_of(body), ctl.pin)
            print("%-26s median %.2f us (step + node %.2f - step alone %.2f; k <= W in %d of %d launches of a replay)" % (
                name, b[0] - s[0], b[0], s[0], min(W, H), H))
            continue
        print("%-26s median %.2f us per launch (min %.2f, max %.2f) over %d replays of %d" % (name, *per_launch_us(g), REPLAYS, H))
    n = 10 * E
    rows = []
    for name, c in (("Controller, model without a table", mpc.Controller(plant, bare_model, K, H, graph_steps=E)),
                    ("Controller, model with a table", mpc.Controller(plant, model, K, H, graph_steps=E)),
                    ("AdaptiveController", mpc_adapt.AdaptiveController(plant, model, K, spec, H))):
        c.run(2 * E)
        us = best_run_us(c, n)
        rows.append(us)
        print("%-36s %d control steps (hipGraph of %d): %.1f us per control step, %.1f us per %d control steps" % (
            name, n, E, us, us * E, E))
    print("one cycle against E bare control steps: +%.1f us (+%.2f%%) over the model with a table, +%.1f us (+%.2f%%) over the "
          "model without one; W / (E * H) = %.2f%% of the model steps are the candidates' replay" % (
              (rows[2] - rows[1]) * E, (rows[2] / rows[1] - 1) * 100, (rows[2] - rows[0]) * E, (rows[2] / rows[0] - 1) * 100,
              100.0 * W / (E * H)))
    model.close()
    bare_model.close()
    plant.close()


def track_main():
    from vine_robot_isaacgymenvs_amd.utils import mpc_track
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % M])
    cfg["seed"] = 42
    if FREE:
        cfg["env"].update(CREATE_PIPE=False, CREATE_SHELF=False)
    cfg["env"]["ENV_TARGET"] = {"VEL_ALONG": {"values": [0.0, 0.1, -0.1, 0.4, -0.4]}, "SPAN_ALONG": 0.05}
    plant = mpc.make_task(cfg)
    model = mpc.make_task(mpc.model_config(cfg, M, K))
    print("%s, %d plants x %d samples = %d model envs, horizon %d, model step kernel %s; ENV_TARGET %s" % (
        torch.cuda.get_device_name(0), M, K, M * K, H, model.step_kernel_name, cfg["env"]["ENV_TARGET"]))
    rounds, n = 9, 50
    for kind in (None,) + mpc_track.PATHS[::-1]:
        c = mpc.Controller(plant, model, K, H) if kind is None else mpc_track.TrackingController(plant, model, K, {"PATH": kind}, H)
        c.run(4)
        us = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.run(n)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) / n * 1e6)
        print("%-22s %d rounds of %d replayed control steps: median %.1f us per control step (min %.1f, max %.1f)%s" % (
            "without track=" if kind is None else "track={PATH: %s}" % kind, rounds, n, np.median(us), min(us), max(us),
            "" if kind is None else "; live %.2f of the plants" % float(c.live.float().mean())))
    ctl = mpc_track.TrackingController(plant, model, K, {"PATH": "exact"}, H, graph=False)
    ctl.control_step()
    print("plan                   median %.2f us per launch (min %.2f, max %.2f) over %d replays of %d" % (
        *per_launch_us(graph_of(ctl.plan)), REPLAYS, H))
    print("track node, no window  median %.2f us per launch (min %.2f, max %.2f)" % per_launch_us(graph_of(ctl.track_node)))
    steps = graph_of(lambda: mpc.Controller.model_step(ctl))
    both = graph_of(ctl.model_step)
    s, b = per_launch_us(steps, ctl.fork), per_launch_us(both, ctl.fork)
    print("step + node %.2f us, step + node + track node %.2f us inside a window: track node = %.2f us" % (s[0], b[0], b[0] - s[0]))
    model.close()
    plant.close()


def main():
    if ADAPT:
        return adapt_main()
    if TRACK:
        return track_main()
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % M])
    cfg["seed"] = 42
    if FREE:
        cfg["env"].update(CREATE_PIPE=False, CREATE_SHELF=False)
    plant = mpc.make_task(cfg)
    model = mpc.make_task(mpc.model_config(cfg, M, K))
    ctl = mpc.Controller(plant, model, K, H)
    print("%s, %d plants x %d samples = %d model envs, horizon %d, model step kernel %s" % (
        torch.cuda.get_device_name(0), M, K, M * K, H, model.step_kernel_name))
    plant.step_into(ctl.plant_actions, ctl.plant_obs)
    ctl.control_step()                                   # (eager: every lazy initialisation done)
    steps = graph_of(lambda: model.step_into(ctl.actions, ctl.model_obs))
    both = graph_of(ctl.model_step)
    forks = graph_of(ctl.fork)
    updates = graph_of(ctl.update)
    s = per_launch_us(steps, ctl.fork)
    print("step alone                    median %.2f us per launch (min %.2f, max %.2f) over %d replays of %d" % (*s, REPLAYS, H))
    b = per_launch_us(both, ctl.fork)                    # every replay scores a live window: k = 1 .. H
    print("step + node                   median %.2f us per pair   (min %.2f, max %.2f): node = %.2f us" % (*b, b[0] - s[0]))
    b = per_launch_us(both)                              # outside a window (k > H): the node returns at once
    print("step + node outside a window  median %.2f us per pair   (min %.2f, max %.2f): node = %.2f us" % (*b, b[0] - s[0]))
    f = per_launch_us(forks)
    print("fork                          median %.2f us per launch (min %.2f, max %.2f)" % f)
    u = per_launch_us(updates)
    print("update                        median %.2f us per launch (min %.2f, max %.2f)" % u)
    for graph in (True, False):
        c = mpc.Controller(plant, model, K, H, graph=graph)
        c.run(2)
        best, n = 1e9, 50
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.run(n)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        print("Controller.run (%s): %d control steps in %.2f ms (best of 5) = %.1f control steps/s, %.1f us per control step; "
              "%d bare model steps = %.1f us; %.3g model env-steps/s"
              % ("hipGraph replay" if c.use_graph else "eager launches", n, best * 1e3, n / best, best / n * 1e6, H, H * s[0],
                 n * M * K * H / best))
    model.close()
    plant.close()


if __name__ == "__main__":
    main()
