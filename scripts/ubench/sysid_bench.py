#!/usr/bin/env python3
"""SYSID timings on one MI355X (profiles/sysid/timings.txt):  python scripts/ubench/sysid_bench.py [num_envs] [horizon]

Per-launch durations from replayed hipGraphs of `horizon` launches each, device events around the replays: the step alone
(one-lane kernel, a parameter table bound), the step with the scoring node behind it (the difference is the node), and the
pin; then candidate-steps/s of Evaluator.evaluate over 8 windows (host clock around work that ends in a synchronise), graph
and eager."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vine_robot_isaacgymenvs_amd import abi, load_task_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import sysid  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
H = int(sys.argv[2]) if len(sys.argv) > 2 else 50
WINDOWS, REPLAYS = 8, 20
SPEC = {"DAMPING": [0.005, 0.1], "ACTION_DELAY": {"values": [0, 1, 2, 3]}, "FPAM_K": [0.7, 1.3]}


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


def main():
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % N])
    cfg["seed"] = 42
    T = WINDOWS * H + 1
    rng = np.random.default_rng(0)
    log = np.zeros((T, abi.RECORD_FIELDS), dtype=np.float32)
    log[:, abi.VRF_Q0 + 1:abi.VRF_Q0 + 6] = rng.uniform(-0.2, 0.2, (T, 5))
    log[:, abi.VRF_ACTION0] = rng.uniform(-0.05, 0.05, T)
    log[:, abi.VRF_ACTION0 + 1] = rng.uniform(-1, 1, T)
    log[:, abi.VRF_PROGRESS] = np.arange(T)
    task = sysid.candidate_task(cfg, SPEC, N, H)
    ev = sysid.Evaluator(task, log, H, weights=[1.0] * 16)
    ev_q = sysid.Evaluator(task, log, H)
    print("%s, %d envs, horizon %d, step kernel %s, table bound" % (torch.cuda.get_device_name(0), N, H, task.step_kernel_name))
    ev.pin(0)
    steps = graph_of(lambda: task.step_into(ev.actions, ev.obs))
    both = graph_of(ev.step)
    both_q = graph_of(ev_q.step)
    pins = graph_of(lambda: ev.pin(0))
    repin = lambda: ev.pin(0)      # noqa: E731  (every replay scores a live window: k = 1 .. H)
    s = per_launch_us(steps, repin)
    print("step alone                    median %.2f us per launch (min %.2f, max %.2f) over %d replays of %d" % (*s, REPLAYS, H))
    for name, g in (("step + node (16 weights, FK) ", both), ("step + node (q weights only)  ", both_q)):
        b = per_launch_us(g, repin)
        print("%s median %.2f us per pair   (min %.2f, max %.2f): node = %.2f us" % (name, *b, b[0] - s[0]))
    b = per_launch_us(both)      # outside a window (k > H): the node returns at once
    print("step + node outside a window  median %.2f us per pair   (min %.2f, max %.2f): node = %.2f us" % (*b, b[0] - s[0]))
    p = per_launch_us(pins)
    print("pin                           median %.2f us per launch (min %.2f, max %.2f)" % p)
    starts = sysid.windows(log, H, H)
    assert len(starts) == WINDOWS
    for graph in (True, False):
        e = sysid.Evaluator(task, log, H, graph=graph)
        e.evaluate(starts[:1])
        best = 1e9
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.evaluate(starts)
            best = min(best, time.perf_counter() - t0)
        print("Evaluator.evaluate (%s): %d windows x %d steps x %d candidates in %.2f ms (best of 5) = %.3g candidate-steps/s"
              % ("hipGraph replay" if graph else "eager launches", WINDOWS, H, N, best * 1e3, WINDOWS * H * N / best))
    task.close()


if __name__ == "__main__":
    main()
