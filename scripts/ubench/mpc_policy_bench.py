#!/usr/bin/env python3
"""MPC_POLICY timings on one MI355X (profiles/mpc_policy/timings.txt):  python scripts/ubench/mpc_policy_bench.py [plants] [samples] [horizon]

In the manner of scripts/ubench/mpc_bench.py: per-launch durations from replayed hipGraphs of `horizon` launches each, device
events around the replays -- the four launches of include/vine_mpc_policy.h (the act inside the window with and without the
keep, the terminal at k == H) and the policy's trunk (its two inference launches, N rows) -- then the whole control step of a
PolicyController, without and with a terminal value, beside the plain Controller's on the same plants (what the commit before
the feature runs), in control steps per second (host clock around replays that end in a synchronise).  Free space; a freshly
initialised network."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vine_robot_isaacgymenvs_amd import load_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_policy  # noqa: E402

M = int(sys.argv[1]) if len(sys.argv) > 1 else 64
K = int(sys.argv[2]) if len(sys.argv) > 2 else 256
H = int(sys.argv[3]) if len(sys.argv) > 3 else 20
REPLAYS = 20


def graph_of(body):
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(H):
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
        out.append(a.elapsed_time(b) * 1000.0 / H)
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
    torch.manual_seed(0)
    net = mpc_policy.PolicyProposal(cfg["train"]["params"], M * K, int(plant.num_obs))
    ctl = mpc_policy.PolicyController(plant, model, K, net, H, graph=False, terminal_value=1.0)
    print("%s, %d plants x %d samples = %d model envs, horizon %d, model step kernel %s" % (
        torch.cuda.get_device_name(0), M, K, M * K, H, model.step_kernel_name))
    plant.step_into(ctl.plant_actions, ctl.plant_obs)
    ctl.control_step()                                   # (eager: every lazy initialisation done)
    y = net.rnn_states[0][0]
    rows = [("policy_fork", ctl.policy_fork, None), ("policy_act, k = 1", lambda: ctl.policy_act(y), 1),
            ("policy_act, k = 0 (with the keep)", lambda: ctl.policy_act(y), 0),
            ("policy_act outside the window", lambda: ctl.policy_act(y), -1),
            ("policy_terminal, k = H", lambda: ctl.policy_terminal(y), H),
            ("policy_terminal outside", lambda: ctl.policy_terminal(y), 0), ("policy_compose", ctl.policy_compose, None),
            ("trunk (split MLP + split LSTM step)", lambda: ctl.infer(), None)]
    with torch.no_grad():
        for name, fn, k in rows:
            if k is not None:
                ctl.window.fill_(int(model.step_count) - k)
            g = graph_of(fn)
            print("%-38s median %.2f us per launch (min %.2f, max %.2f) over %d replays of %d" % (name, *per_launch_us(g), REPLAYS, H))
    n = 50
    out = []
    for name, c in (("Controller (no policy)", mpc.Controller(plant, model, K, H)),
                    ("PolicyController", mpc_policy.PolicyController(plant, model, K, net, H)),
                    ("PolicyController, terminal_value", mpc_policy.PolicyController(plant, model, K, net, H, terminal_value=1.0))):
        c.run(2)
        us = best_run_us(c, n)
        out.append(us)
        print("%-34s %d control steps (hipGraph replay, best of 5): %.1f us per control step = %.1f control steps/s; %.1f us per "
              "horizon step" % (name, n, us, 1e6 / us, us / H))
    print("the policy adds %.1f us per horizon step (%.1f us per control step); the terminal value %.1f us per control step more"
          % ((out[1] - out[0]) / H, out[1] - out[0], out[2] - out[1]))
    model.close()
    plant.close()


if __name__ == "__main__":
    main()
