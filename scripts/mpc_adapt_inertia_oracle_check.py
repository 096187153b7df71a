#!/usr/bin/env python3
"""MPC_ADAPT masses on the CPU: the numpy statements of utils/mpc_adapt_inertia.py (mass_candidates, mass_estimate) and of
utils/mpc_adapt.py (candidates, score, estimate) driven by float64 oracle traces, for the plants of
tests/test_mpc_adapt_inertia_gpu.py::test_it_adapts.  No GPU is needed.

  python scripts/mpc_adapt_inertia_oracle_check.py --case link             # LINK_MASS 0.75 / 0.9 / 1.15 / 1.35, prior 1.0
  python scripts/mpc_adapt_inertia_oracle_check.py --case cart             # CART_MASS 0.6 / 0.8 / 1.4 / 1.8 x c over [0.5 c, 2 c]
  python scripts/mpc_adapt_inertia_oracle_check.py --case link_damping     # LINK_MASS as above together with DAMPING

Every plant is one float64 oracle env whose configuration carries that plant's masses (the oracle has per-env masses through
its configuration); every candidate is one more, created with the float32 masses its theta gives in the rounding of
``env_params.set_inertia_rows``, put onto the plant's state block at the anchor and fed the traced actions.  As in
scripts/mpc_adapt_oracle_check.py the plant is driven by zero-mean random actions held for two steps each, NOT by the
controller.  Prints, per plant, the belief after every pass and |mean - truth| / |prior - truth| at the end:
profiles/mpc_adapt_inertia/it_adapts_oracle.txt records them."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import vine_oracle as vo  # noqa: E402
from vine_robot_isaacgymenvs_amd import abi, load_task_config  # noqa: E402
from vine_robot_isaacgymenvs_amd.tasks.vine5link_moving_base import vine_config_from_cfg  # noqa: E402
from vine_robot_isaacgymenvs_amd.utils import env_params, mpc_adapt, mpc_adapt_inertia  # noqa: E402

LINKS = [0.75, 0.9, 1.15, 1.35]
CARTS = [0.6, 0.8, 1.4, 1.8]          # factors on the configuration's cart mass c
DAMPINGS = [0.01, 0.03, 0.07, 0.095]
JOINTS = slice(abi.VF_Q0, abi.VF_Q0 + 12)


def base_config(seed=1):
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=1"])
    cfg["seed"] = seed
    cfg["task"]["vine_randomize"] = False
    cfg["env"].update(CREATE_PIPE=False, CREATE_SHELF=False, USE_TARGET_REACHED_RESET=False)
    return vine_config_from_cfg(cfg, vo.load("f64"), seed=seed)


def base_primaries(c):
    return np.array([c.cart_mass] + list(c.link_mass) + list(c.link_inertia), dtype=np.float32)


def plant_config(base, values, damping=None, seed=1):
    """The configuration whose masses are ``values`` ({name: theta}) on the primaries ``base``, in the table's rounding."""
    c = base_config(seed)
    table = np.zeros((abi.VI_COUNT, 1), dtype=np.float32)
    table[:abi.VI_PRIMARY_COUNT, 0] = base
    row = np.zeros(abi.VI_COUNT, dtype=np.float32)
    row[:abi.VI_PRIMARY_COUNT] = base
    env_params.set_inertia_rows(table, row, {k: np.array([v], dtype=np.float64) for k, v in values.items()})
    c.cart_mass = float(table[abi.VI_CART_MASS, 0])
    for i in range(abi.NUM_LINKS):
        c.link_mass[i] = float(table[abi.VI_LINK_MASS0 + i, 0])
        c.link_inertia[i] = float(table[abi.VI_LINK_INERTIA0 + i, 0])
    if damping is not None:
        c.damping = float(np.float32(damping))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("link", "cart", "link_damping"), default="link")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--window", type=int, default=mpc_adapt.DEFAULTS["window"])
    ap.add_argument("--every", type=int, default=mpc_adapt.DEFAULTS["every"])
    ap.add_argument("--temperature", type=float, default=mpc_adapt.DEFAULTS["temperature"])
    ap.add_argument("--rate", type=float, default=mpc_adapt.DEFAULTS["rate"])
    ap.add_argument("--spread", type=float, default=mpc_adapt.DEFAULTS["spread"])
    ap.add_argument("--floor", type=float, default=mpc_adapt.DEFAULTS["floor"])
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    vo.build()
    base = base_primaries(base_config(a.seed))
    c = float(base[abi.VI_CART_MASS])
    M, K, W, E = 4, a.samples, a.window, a.every
    name = "CART_MASS" if a.case == "cart" else "LINK_MASS"
    rng_of = [0.5 * c, 2.0 * c] if a.case == "cart" else [0.7, 1.4]
    plant_values = [float(np.float32(f * c)) for f in CARTS] if a.case == "cart" else LINKS
    prior_value = c if a.case == "cart" else 1.0
    with_damping = a.case == "link_damping"
    spec = {"params": {"DAMPING": [0.005, 0.1]}, "masses": {name: rng_of}, "window": W, "every": E,
            "temperature": a.temperature, "rate": a.rate, "spread": a.spread, "floor": a.floor}
    acfg, _ = mpc_adapt.adapt_config({k: v for k, v in spec.items() if k != "masses"}, M, K, np.zeros(abi.VP_COUNT, np.float32),
                                     a.seed)
    dims = mpc_adapt.dims_of(acfg)
    icfg, _ = mpc_adapt_inertia.masses_config(spec, np.concatenate([base, np.zeros(abi.VI_COUNT - abi.VI_PRIMARY_COUNT, np.float32)]),
                                              1.0, 1.0, 9.81)      # (the geometry is not read here: the oracle derives its own)
    mdims = mpc_adapt_inertia.mass_dims_of(icfg)
    weights = np.array(list(acfg.weights), dtype=np.float32)
    truth = np.array(plant_values, dtype=np.float64)
    prior = np.full(M, np.float64(prior_value))
    mmean, mstd = prior[:, None].copy(), np.full((M, 1), a.spread * (mdims[0][2] - mdims[0][1]))
    dtruth = np.array([np.float64(np.float32(d)) for d in DAMPINGS])
    dprior = np.full(M, np.float64(np.float32(0.0525)))
    dmean = dprior[:, None].copy()
    dstd = np.full((M, 1), a.spread * (dims[0][3] - dims[0][2]) if with_damping else 0.0)
    if not with_damping:                                   # every plant and candidate has the configuration's damping
        dmean[:] = np.float64(np.float32(base_config(a.seed).damping))
    passes = np.zeros(M, dtype=np.int64)
    plants = [vo.OracleEnv(plant_config(base, {name: plant_values[i]}, DAMPINGS[i] if with_damping else None, a.seed), "f64")
              for i in range(M)]
    rng = np.random.default_rng(a.seed)
    for p in plants:                                          # the first step consumes the reset every env starts with
        p.step(np.zeros((1, 2), np.float32))
    print("case %s: plants %s %s%s, prior %.4g, std %.4g, floor %.5g; K %d, W %d, E %d, temperature %g, rate %g; actions +-%g" % (
        a.case, name, np.array2string(truth, precision=4), (" and DAMPING %s" % DAMPINGS) if with_damping else "", prior_value,
        mstd[0, 0], mdims[0][3], K, W, E, a.temperature, a.rate, a.scale))
    for it in range(a.passes):
        theta = mpc_adapt_inertia.mass_candidates(mmean, mstd, mdims, a.seed, K, passes)
        dtheta = mpc_adapt.candidates(dmean, dstd, dims, a.seed, K, passes)
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
                cand = vo.OracleEnv(plant_config(base, {name: theta[i, j, 0]}, dtheta[i, j, 0] if with_damping else None, a.seed),
                                    "f64")
                cand.state[:, 0] = anchor
                cand.progress[:], cand.reset_buf[:] = progress, 0
                cand.step_count = count
                for k in range(1, tl + 1):
                    cand.step(acts[k - 1:k])
                    states[k - 1, :, j], resets[k - 1, j] = cand.state[JOINTS, 0].astype(np.float32), cand.reset_buf[0]
                cand.close()
            err[i], _ = mpc_adapt.score(states, resets, rows, [tl], weights, K)
        r = mpc_adapt_inertia.mass_estimate(err.reshape(-1), theta, mmean, mstd, mmean, mstd, trace_len, ended, mdims,
                                            acfg.min_steps, a.temperature, a.rate, False)
        if with_damping:
            rd = mpc_adapt.estimate(err.reshape(-1), dtheta, dmean, dstd, dmean, dstd, trace_len, ended, dims, acfg.min_steps,
                                    a.temperature, a.rate, False)
            dmean, dstd = rd["mean"], rd["std"]
        mmean, mstd = r["mean"], r["std"]
        passes += 1
        print("pass %2d: trace_len %s  %s mean %s  std %s%s" % (
            it + 1, trace_len, name, np.array2string(mmean[:, 0], precision=4), np.array2string(mstd[:, 0], precision=4),
            ("  DAMPING mean %s" % np.array2string(dmean[:, 0], precision=4)) if with_damping else ""), flush=True)
    ratio = np.abs(mmean[:, 0] - truth) / np.abs(prior - truth)
    print("truth %s" % np.array2string(truth, precision=4))
    print("%s |mean - truth| / |prior - truth| %s" % (name, np.array2string(ratio, precision=4)))
    if with_damping:
        print("DAMPING |mean - truth| / |prior - truth| %s" % np.array2string(
            np.abs(dmean[:, 0] - dtruth) / np.abs(dprior - dtruth), precision=4))
    print("oracle reaches 0.25 (the device test then asserts 0.5) for plants: %s" % np.flatnonzero(ratio <= 0.25).tolist())
    for p in plants:
        p.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
