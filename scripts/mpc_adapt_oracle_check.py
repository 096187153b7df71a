#!/usr/bin/env python3
"""MPC_ADAPT on the CPU: the numpy statements of utils/mpc_adapt.py (candidates, score, estimate) driven by float64 oracle
traces, for the plants of tests/test_mpc_adapt_gpu.py::test_it_adapts.  No GPU is needed.

  python scripts/mpc_adapt_oracle_check.py                     # the test's values: 4 plants, K = 64, W = E = 8, P = 10
  python scripts/mpc_adapt_oracle_check.py --temperature 0.3 --rate 0.7 --passes 6

Every plant is one float64 oracle env whose configuration carries that plant's DAMPING; every candidate is one more, created
with float32(theta) as its DAMPING, put onto the plant's state block at the anchor and fed the traced actions.  The plant is
driven by zero-mean random actions, uniform in +-``--scale`` and held for two steps each, NOT by the controller: what is
checked is whether eight steps of such a trajectory tell the dampings apart and whether the estimate then walks the belief
to the truth, which is what the four constants (temperature, rate, spread, floor) decide.  The rows and the candidates'
states are rounded to float32 before they are compared, as the device's are.  Prints, per plant, the belief after every pass
and |mean - truth| / |prior - truth| at the end: profiles/mpc_adapt/it_adapts.txt records them beside the device's."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import vine_oracle as vo  # noqa: E402
from vine_robot_isaacgymenvs_amd import abi, load_task_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.tasks.vine5link_moving_base import vine_config_from_cfg  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import mpc_adapt  # noqa: E402

DAMPINGS = [0.01, 0.03, 0.07, 0.095]
JOINTS = slice(abi.VF_Q0, abi.VF_Q0 + 12)


def plant_config(damping, seed=1):
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=1"])
    cfg["seed"] = seed
    cfg["task"]["vine_randomize"] = False
    cfg["env"].update(CREATE_PIPE=False, CREATE_SHELF=False, USE_TARGET_REACHED_RESET=False)
    c = vine_config_from_cfg(cfg, vo.load("f64"), seed=seed)
    c.damping = float(np.float32(damping))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--window", type=int, default=mpc_adapt.DEFAULTS["window"])
    ap.add_argument("--every", type=int, default=mpc_adapt.DEFAULTS["every"])
    ap.add_argument("--temperature", type=float, default=mpc_adapt.DEFAULTS["temperature"])
    ap.add_argument("--rate", type=float, default=mpc_adapt.DEFAULTS["rate"])
    ap.add_argument("--spread", type=float, default=mpc_adapt.DEFAULTS["spread"])
    ap.add_argument("--floor", type=float, default=mpc_adapt.DEFAULTS["floor"])
    ap.add_argument("--prior", type=float, default=0.0525)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    vo.build()
    M, K, W, E = len(DAMPINGS), a.samples, a.window, a.every
    spec = {"params": {"DAMPING": [0.005, 0.1]}, "window": W, "every": E, "temperature": a.temperature, "rate": a.rate,
            "spread": a.spread, "floor": a.floor}
    acfg, _ = mpc_adapt.adapt_config(spec, M, K, np.zeros(abi.VP_COUNT, np.float32), a.seed)
    dims = mpc_adapt.dims_of(acfg)
    lo, hi, floor = dims[0][2], dims[0][3], dims[0][4]
    weights = np.array(list(acfg.weights), dtype=np.float32)
    truth = np.array([np.float64(np.float32(d)) for d in DAMPINGS])
    prior = np.full(M, np.float64(np.float32(a.prior)))
    mean, std = prior[:, None].copy(), np.full((M, 1), a.spread * (hi - lo))
    passes = np.zeros(M, dtype=np.int64)
    plants = [vo.OracleEnv(plant_config(d, a.seed), "f64") for d in DAMPINGS]
    rng = np.random.default_rng(a.seed)
    for p in plants:                                          # the first step consumes the reset every env starts with
        p.step(np.zeros((1, 2), np.float32))
    print("plants DAMPING %s, prior %.4f, std %.4f, floor %.5f; K %d, W %d, E %d, temperature %g, rate %g; actions +-%g" % (
        DAMPINGS, a.prior, std[0, 0], floor, K, W, E, a.temperature, a.rate, a.scale))
    for it in range(a.passes):
        theta = mpc_adapt.candidates(mean, std, dims, a.seed, K, passes)
        err = np.zeros((M, K))
        trace_len, ended = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.uint8)
        for i, plant in enumerate(plants):
            anchor = plant.state[:, 0].copy()
            progress, count = plant.progress.copy(), plant.step_count
            is_open = plant.reset_buf[0] == 0
            rows, acts = np.zeros((1, W, 12), np.float32), np.zeros((W, 2), np.float32)
            held = None
            for s in range(1, E + 1):
                if s % 2 == 1:
                    held = rng.uniform(-a.scale, a.scale, (1, 2)).astype(np.float32)
                plant.step(held)
                raised = plant.reset_buf[0] != 0
                if s <= W and is_open:
                    rows[0, s - 1], acts[s - 1] = plant.state[JOINTS, 0].astype(np.float32), held[0]
                    trace_len[i] = s
                    is_open = not raised
                ended[i] |= raised
            tl = int(trace_len[i])
            states, resets = np.zeros((W, 12, K), np.float32), np.zeros((W, K), np.int64)
            for j in range(K if tl else 0):
                cand = vo.OracleEnv(plant_config(theta[i, j, 0], a.seed), "f64")
                cand.state[:, 0] = anchor
                cand.progress[:], cand.reset_buf[:] = progress, 0
                cand.step_count = count
                for k in range(1, tl + 1):
                    cand.step(acts[k - 1:k])
                    states[k - 1, :, j], resets[k - 1, j] = cand.state[JOINTS, 0].astype(np.float32), cand.reset_buf[0]
                cand.close()
            err[i], _ = mpc_adapt.score(states, resets, rows, [tl], weights, K)
        r = mpc_adapt.estimate(err.reshape(-1), theta, mean, std, mean, std, trace_len, ended, dims, acfg.min_steps,
                               a.temperature, a.rate, False)
        mean, std = r["mean"], r["std"]
        passes += 1
        best = theta[np.arange(M), np.argmin(err, axis=1), 0]
        print("pass %2d: trace_len %s  best candidate %s  mean %s  std %s" % (
            it + 1, trace_len, np.array2string(best, precision=4), np.array2string(mean[:, 0], precision=4),
            np.array2string(std[:, 0], precision=5)), flush=True)
    ratio = np.abs(mean[:, 0] - truth) / np.abs(prior - truth)
    print("truth %s" % np.array2string(truth, precision=4))
    print("|prior - truth| %s  (2 * std_floor = %.5f)" % (np.array2string(np.abs(prior - truth), precision=4), 2 * floor))
    print("|mean - truth| / |prior - truth| %s" % np.array2string(ratio, precision=4))
    print("condition (every ratio <= 0.5): %s" % ("met" if np.all(ratio <= 0.5) else "NOT met"))
    for p in plants:
        p.close()
    return 0 if np.all(ratio <= 0.5) else 1


if __name__ == "__main__":
    sys.exit(main())
