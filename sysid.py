#!/usr/bin/env python3
"""Fit per-env plant parameters to a recorded trajectory (vine_robot_isaacgymenvs_amd/utils/sysid.py).

  python sysid.py task=Vine5LinkMovingBase log=<file>.mat \\
      'params={DAMPING: [0.005, 0.1], ACTION_DELAY: {values: [0, 1, 2, 3]}, FPAM_K: [0.7, 1.3]}' \\
      num_envs=4096 iterations=8 horizon=50 stride=25

``params`` also takes the masses: ``CART_MASS`` in kg, ``LINK_MASS`` and ``TIP_LINK_MASS`` as factors on
the configuration's link masses and inertias, e.g. ``'params={CART_MASS: [0.5, 2.0], LINK_MASS: [0.7, 1.4], DAMPING: [0.005, 0.1]}'``.

``log``, ``params`` (an ``ENV_PARAMS``-style spec), ``iterations``, ``horizon``, ``stride``, ``weights`` (16 numbers, one per
row field), ``elite_fraction`` and ``out`` (directory of the .npz; default ``runs/sysid``) are this tool's own
keys; every other ``key=value`` is an override of the project's configuration, in its syntax (``num_envs=``, ``seed=``,
``task.env.DAMPING=`` ...)."""
import logging
import sys

OWN = {"log": None, "params": None, "iterations": 8, "horizon": 50, "stride": 25, "weights": None, "elite_fraction": 0.1,
       "out": "runs/sysid"}


def main(argv=None):
    from vine_robot_isaacgymenvs_amd.utils import sysid
    from vine_robot_isaacgymenvs_amd.utils.config import ConfigError, load_config, parse_scalar
    argv = sys.argv[1:] if argv is None else list(argv)
    own, overrides = dict(OWN), []
    for arg in argv:
        key, eq, val = arg.partition("=")
        if eq and key in OWN:
            own[key] = val if key in ("log", "out") else parse_scalar(val)
        else:
            overrides.append(arg)
    if not own["log"]:
        raise ConfigError("sysid: log=<file>.mat is required")
    if not hasattr(own["params"], "keys") or not len(own["params"]):
        raise ConfigError("sysid: params={NAME: [lo, hi] | {values: [...]} | number, ...} is required")
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    cfg = load_config("config", overrides=overrides)
    seed = cfg.get("seed", 0)
    task_cfg = cfg["task"]
    task_cfg["seed"] = seed
    return sysid.fit(task_cfg, own["log"], own["params"], num_envs=int(task_cfg["env"]["numEnvs"]),
                     iterations=int(own["iterations"]), horizon=int(own["horizon"]), stride=int(own["stride"]),
                     seed=int(seed) if isinstance(seed, int) and seed >= 0 else 0, weights=own["weights"],
                     directory=own["out"], elite_fraction=float(own["elite_fraction"]),
                     device=cfg.get("sim_device", "cuda:0"))


if __name__ == "__main__":
    main()
