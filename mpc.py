#!/usr/bin/env python3
"""Sampling-based predictive control of the plants on the device (vine_robot_isaacgymenvs_amd/utils/mpc.py).

  python mpc.py task=Vine5LinkMovingBase plants=64 samples=256 horizon=20 steps=2000 task.env.EPISODE_LOG=True

  python mpc.py plants=64 steps=2000 task.env.EPISODE_LOG=True \\
      'task.env.ENV_PARAMS={DAMPING: [0.005, 0.1], LINK_MASS: [0.7, 1.4]}'          # such plants, the nominal model

  python mpc.py plants=64 'model_params={DAMPING: [0.005, 0.1]}'                     # the nominal plant, such models

  python mpc.py plants=64 steps=2000 'task.env.ENV_PARAMS={DAMPING: [0.005, 0.1]}' \\
      'adapt={params: {DAMPING: [0.005, 0.1], FPAM_K: [0.7, 1.3]}, window: 8, every: 8}'   # the model follows each plant

  python mpc.py plants=64 steps=2000 'task.env.ENV_PARAMS={DAMPING: [0.005, 0.1], LINK_MASS: [0.7, 1.4]}' \\
      'adapt={params: {DAMPING: [0.005, 0.1]}, masses: {LINK_MASS: [0.7, 1.4]}}'       # ... in its masses too

  python mpc.py plants=64 steps=2000 task.env.EPISODE_LOG=True policy=runs/Vine5LinkMovingBase/nn/Vine5LinkMovingBase.pth \\
      terminal_value=1.0                                                             # the samples roll this policy

  python mpc.py plants=64 steps=2000 task.env.EPISODE_LOG=True \\
      'observe={DELAY: 3, HOLD: 0.1, NOISE_Q: 0.002, COMPENSATE: True}'              # the planner's own delayed, noisy sensor

  python mpc.py plants=64 steps=2000 task.env.EPISODE_LOG=True 'observe={DELAY: 1, NOISE_Q: 0.01, NOISE_QD: 0.1}' \\
      'filter={GAIN_Q: 0.3, GAIN_QD: {values: [0.1, 0.3, 1.0]}}'                     # ... averaged over successive frames

  python mpc.py plants=64 steps=2000 task.env.EPISODE_LOG=True \\
      'task.env.ENV_TARGET={VEL_ALONG: {values: [0, 0.1, -0.1]}, SPAN_ALONG: 0.05}' \\
      'track={PATH: exact}'                                                          # the samples' targets move as the plant's will

  python mpc.py plants=64 steps=2000 task.env.EPISODE_LOG=True \\
      'noise={BETA: 0.8, ADAPT: {RATE: 0.2, SIGMA_MIN: 0.05, SIGMA_MAX: 1.0}}'       # correlated samples, a sigma per plant

  python mpc.py plants=64 samples=1024 steps=2000 task.env.EPISODE_LOG=True \\
      'task.env.ENV_PARAMS={DAMPING: [0.005, 0.1], LINK_MASS: [0.7, 1.4]}' \\
      'ensemble={params: {DAMPING: [0.005, 0.1], LINK_MASS: [0.7, 1.4]}, MEMBERS: 4, RISK: entropic, THETA: 0.5}'
                                                                                     # every sequence on four candidate plants

``plants``, ``samples``, ``horizon``, ``lambda``, ``sigma`` (one number or ``[rail, fpam]``), ``steps``, ``cost`` (a mapping of
``*_REWARD_WEIGHT`` keys for the model only; default ``{POSITION_REWARD_WEIGHT: 1.0}``), ``model_params`` (an ``ENV_PARAMS``-style
spec, drawn once per plant and repeated over the plant's samples), ``adapt`` (online adaptation of the model to each plant,
DESIGN.md section 25: ``params`` maps names of the ``ENV_PARAMS`` table to the range ``[lo, hi]`` the belief lives in; ``window``,
``every``, ``min_steps``, ``temperature``, ``rate``, ``spread``, ``floor``, ``weights``; ``masses`` maps ``CART_MASS`` (kg), ``LINK_MASS``
and ``TIP_LINK_MASS`` (factors on the model configuration's link masses and inertias) to such a range and may stand without
``params``), ``policy`` (a checkpoint of ``train.py``:
the samples roll it and the planner's sequence is a residual on its mean; the network is the composed
configuration's ``train.params``; plants * samples must be a multiple of 512), ``terminal_value`` (the weight of the critic's
value behind the horizon; default 0), ``observe`` (the planner sees its plants through a sensing path of its own, DESIGN.md
section 27: ``DELAY``, ``HOLD``, ``NOISE_Q``, ``NOISE_QD`` as ``ENV_SENSOR`` takes them, ``COMPENSATE``, ``CATCHUP``), ``filter``
(a fixed-gain corrector over those frames, DESIGN.md section 28: ``GAIN_Q``, ``GAIN_QD`` in [0, 1]; needs ``observe``), ``track``
(the samples' targets follow their plant's ``task.env.ENV_TARGET`` path over the horizon, DESIGN.md section 30: ``PATH`` is
``exact``, ``linear`` or ``held``; refused with ``policy``, ``adapt``, ``observe`` and ``filter``), ``noise`` (the samples'
perturbations are correlated over the horizon, DESIGN.md section 32: ``BETA`` in [0, 1), one number or ``[rail, fpam]``, and
optionally ``ADAPT`` with ``RATE``, ``SIGMA_MIN``, ``SIGMA_MAX`` for a sigma per plant; refused with every other variant),
``ensemble`` (every action sequence is rolled through ``MEMBERS`` candidate plants drawn from the ``ENV_PARAMS``-style ``params``
and weighted by ``RISK`` -- ``mean``, ``max`` or ``entropic`` with ``THETA`` -- over their costs; ``samples``
must be a multiple of ``MEMBERS``; refused with every other variant and with ``model_params``) and ``out``
(directory of the episode log's .npz; default ``runs/mpc``) are this tool's own keys; every other ``key=value`` is an override of the project's configuration for the PLANT, in its syntax (``seed=``, ``task.env.CREATE_PIPE=`` ...)."""
import logging
import sys

OWN = {"plants": 64, "samples": 256, "horizon": 20, "lambda": 0.05, "sigma": 0.5, "steps": 500, "cost": None,
       "model_params": None, "adapt": None, "policy": None, "terminal_value": 0.0, "observe": None, "filter": None,
       "track": None, "noise": None, "ensemble": None, "out": "runs/mpc"}


def main(argv=None):
    from vine_robot_isaacgymenvs_amd.utils import mpc
    from vine_robot_isaacgymenvs_amd.utils.config import ConfigError, load_config, parse_scalar
    argv = sys.argv[1:] if argv is None else list(argv)
    own, overrides = dict(OWN), []
    for arg in argv:
        key, eq, val = arg.partition("=")
        if eq and key in OWN:
            own[key] = val if key in ("out", "policy") else parse_scalar(val)
        else:
            overrides.append(arg)
    for key in ("cost", "model_params", "adapt", "observe", "filter", "track", "noise", "ensemble"):
        if own[key] is not None and not hasattr(own[key], "keys"):
            raise ConfigError("mpc: %s={NAME: value, ...} must be a mapping, not %r" % (key, own[key]))
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    cfg = load_config("config", overrides=overrides)
    seed = cfg.get("seed", 0)
    task_cfg = cfg["task"]
    task_cfg["seed"] = seed
    if not task_cfg["env"].get("EPISODE_LOG_DIR"):
        task_cfg["env"]["EPISODE_LOG_DIR"] = own["out"]
    return mpc.play(task_cfg, plants=own["plants"], samples=own["samples"], horizon=own["horizon"], lam=own["lambda"],
                    sigma=own["sigma"], steps=int(own["steps"]), cost=own["cost"], model_params=own["model_params"],
                    seed=int(seed) if isinstance(seed, int) and seed >= 0 else 0, device=cfg.get("sim_device", "cuda:0"),
                    adapt=own["adapt"], policy=own["policy"], terminal_value=own["terminal_value"],
                    policy_params=cfg["train"]["params"] if own["policy"] else None, observe=own["observe"],
                    filter=own["filter"], track=own["track"], noise=own["noise"], ensemble=own["ensemble"])


if __name__ == "__main__":
    main()
