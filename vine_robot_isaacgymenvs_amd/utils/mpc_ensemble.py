"""MPC_ENSEMBLE on the host side: the predictive controller scores every action sequence on several candidate plants and
weights it by a risk over their costs (ensemble, or risk-sensitive, MPPI).  The semantics are stated once, in
include/vine_mpc_ensemble.h.  What is left for the host: the ``ensemble=`` mapping (``ensemble_config``), the checked
``abi.VineMpcEnsembleConfig`` (``ensemble_struct``), the members' draw (``draw_members``, ``tile_members``), the numpy statement
of the two launches every GPU test compares against (``group_actions``, ``group_costs``, ``ensemble_replay``), and the
controller that enqueues the launches (``EnsembleController``).

``ensemble=`` maps

  ``params``    an ``ENV_PARAMS``-style spec (numbers, ranges ``[lo, hi]``, ``{values: [..]}``; the mass names included): what
                the planner knows of its plant.  Member m of plant p is one draw from it.  Required, not empty.
  ``MEMBERS``   E, 1 .. 16, a divisor of ``samples`` (default 4): the K samples of a plant are K / E sequences times E members
  ``RISK``      ``mean`` (default), ``max`` or ``entropic``: how a sequence's member costs become its cost
  ``THETA``     with ``entropic``: the risk aversion, > 0 (towards 0 the mean, towards infinity the maximum)
  ``SEED``      the seed of the members' draw (default: the planner's seed + 1; with the plants' own seed member m of plant p
                would be drawn as the plant of the same global id is, and the ensemble would hold the truth)"""
import copy

import numpy as np

from .. import abi
from . import env_params, mpc
from .config import ConfigError

_KEY = "ensemble"
KEYS = ("params", "MEMBERS", "RISK", "THETA", "SEED")
DEFAULT_MEMBERS = 4


# ---- configuration
def ensemble_config(spec):
    """The checked ``ensemble=`` mapping: ``{"params": forms, "MEMBERS": E, "RISK": name, "THETA": theta | None, "SEED": seed |
    None}`` (``forms``: ``env_params.spec_forms``; ``SEED`` ``None``: the planner's seed + 1).  ``ConfigError``, naming the key,
    for anything else."""
    if not hasattr(spec, "keys"):
        raise ConfigError("%s={params: {NAME: [lo, hi], ...}, ...} must be a mapping, not %r" % (_KEY, spec))
    unknown = sorted(str(k) for k in set(spec.keys()) - set(KEYS))
    if unknown:
        raise ConfigError("%s: unknown key(s) %s" % (_KEY, ", ".join(unknown)))
    params = spec.get("params")
    if params is None:
        raise ConfigError("%s.params is missing: an ENV_PARAMS-style spec of what the planner knows of its plant" % _KEY)
    if not hasattr(params, "keys") or not len(params):
        raise ConfigError("%s.params must be a mapping of parameter names that is not empty, not %r" % (_KEY, params))
    try:
        forms = env_params.spec_forms(params)
    except ConfigError as e:
        raise ConfigError("%s.params: %s" % (_KEY, e)) from None
    members = spec.get("MEMBERS", DEFAULT_MEMBERS)
    if isinstance(members, bool) or not isinstance(members, (int, np.integer)) or not 1 <= members <= abi.MPC_ENSEMBLE_MAX_MEMBERS:
        raise ConfigError("%s.MEMBERS must be an integer in 1 .. %d, not %r" % (_KEY, abi.MPC_ENSEMBLE_MAX_MEMBERS, members))
    risk = spec.get("RISK", "mean")
    if risk not in abi.MPC_RISK_NAMES:
        raise ConfigError("%s.RISK must be one of %s, not %r" % (_KEY, ", ".join(abi.MPC_RISK_NAMES), risk))
    theta = spec.get("THETA")
    if risk == "entropic":
        if theta is None:
            raise ConfigError("%s.THETA is missing: RISK entropic needs its risk aversion, a number > 0" % _KEY)
        if isinstance(theta, bool) or not isinstance(theta, (int, float, np.integer, np.floating)) or not np.isfinite(theta) \
                or not theta > 0:
            raise ConfigError("%s.THETA must be a finite number > 0, not %r" % (_KEY, theta))
        theta = float(theta)
    elif theta is not None:
        raise ConfigError("%s.THETA is refused with RISK %s: only entropic reads it" % (_KEY, risk))
    seed = spec.get("SEED")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0):
        raise ConfigError("%s.SEED must be an integer >= 0, not %r" % (_KEY, seed))
    return {"params": forms, "MEMBERS": int(members), "RISK": str(risk), "THETA": theta, "SEED": None if seed is None else int(seed)}


def ensemble_struct(spec, mcfg):
    """The ``abi.VineMpcEnsembleConfig`` of an ``ensemble=`` mapping beside the controller's ``abi.VineMpcConfig``:
    ``ConfigError`` for a ``samples`` that is no multiple of ``MEMBERS``, which the library would refuse too."""
    spec = ensemble_config(spec)
    if mcfg.samples % spec["MEMBERS"]:
        raise ConfigError("mpc: samples = %d is not a multiple of %s.MEMBERS = %d: a plant's samples are sequences x members" % (
            mcfg.samples, _KEY, spec["MEMBERS"]))
    c = abi.VineMpcEnsembleConfig()
    c.abi_version = abi.MPC_ENSEMBLE_ABI_VERSION
    c.members = spec["MEMBERS"]
    c.risk = abi.MPC_RISK_NAMES.index(spec["RISK"])
    c.theta = spec["THETA"] if spec["THETA"] is not None else 1.0
    return c


def draw_members(spec, vcfg, lib, seed, num_plants, members):
    """``{name: float64 [M, E]}``: the ``ENV_PARAMS``-style ``spec`` drawn once per (plant, member) with ``env_params``' own draw
    under the global id ``p * E + m``: the value itself, a factor for the FPAM vectors and the link masses.  A pure function
    of its arguments."""
    M, E = int(num_plants), int(members)
    draws = {}
    env_params.draw_table(spec, env_params.config_row(lib, vcfg), seed, M * E, draws=draws)
    return {name: np.asarray(v, dtype=np.float64).reshape(M, E) for name, v in draws.items()}


def tile_members(values, groups):
    """``{name: [M, E]}`` as ``{name: [M * K]}``, K = ``groups`` * E: each plant's E values tiled over its groups, sample j of
    plant p taking member j mod E -- what ``set_env_params`` of the model task takes."""
    out = {}
    for name, v in values.items():
        v = np.asarray(v, dtype=np.float64)
        if v.ndim != 2:
            raise ValueError("tile_members: %s takes an array [plants, members], not %s" % (name, v.shape))
        out[name] = np.tile(v, (1, int(groups))).reshape(-1)
    return out


# ---- the launches, in numpy
def group_actions(nominal, sigma, seed, samples, members, tick, clip):
    """float32 [M, G, H, 2]: ``u_g`` of include/vine_mpc_ensemble.h around ``nominal`` [M, H, 2] -- ``mpc.sample_actions`` of a
    controller with G = ``samples`` / ``members`` samples: the counter's first word is the group's index p * G + g, and group 0
    is the clamped nominal.  ``member_actions`` spreads it over the model envs."""
    K, E = int(samples), int(members)
    if K % E:
        raise ValueError("group_actions: samples = %d is not a multiple of members = %d" % (K, E))
    return mpc.sample_actions(nominal, sigma, seed, K // E, tick, clip)


def member_actions(u, members):
    """[M, G, H, 2] as [M, K, H, 2]: every member of a group holds the group's words."""
    return np.repeat(np.asarray(u), int(members), axis=1)


def group_costs(cost, members, risk, theta=None):
    """float64 [M, G]: ``C_g`` of include/vine_mpc_ensemble.h from ``cost`` [M, K] (or [M * K] with M = 1).  The member loop
    is written out in ascending m: ``np.sum`` adds pairwise, the device one after the other."""
    cost = np.asarray(cost, dtype=np.float64)
    cost = cost.reshape(1, -1) if cost.ndim == 1 else cost
    M, K, E = cost.shape[0], cost.shape[1], int(members)
    if risk not in abi.MPC_RISK_NAMES:
        raise ValueError("group_costs: risk must be one of %s, not %r" % (", ".join(abi.MPC_RISK_NAMES), risk))
    if K % E:
        raise ValueError("group_costs: %d costs per plant are not a multiple of members = %d" % (K, E))
    c = cost.reshape(M, K // E, E)
    finite = np.isfinite(c).all(axis=2)
    safe = np.where(finite[..., None], c, 0.0)                             # (a discarded group's arithmetic is not looked at)
    cmax = safe[..., 0].copy()
    for m in range(1, E):
        cmax = np.maximum(cmax, safe[..., m])
    if risk == "max":
        out = cmax
    elif risk == "mean":
        s = safe[..., 0].copy()
        for m in range(1, E):
            s = s + safe[..., m]
        out = s / np.float64(E)
    else:
        theta = np.float64(theta)
        if not np.isfinite(theta) or not theta > 0:
            raise ValueError("group_costs: entropic needs a finite theta > 0, not %r" % (theta,))
        s = np.exp(theta * (safe[..., 0] - cmax))
        for m in range(1, E):
            s = s + np.exp(theta * (safe[..., m] - cmax))
        out = cmax + np.log(s / np.float64(E)) / theta
    return np.where(finite, out, np.inf)


def ensemble_replay(nominal, cost, sigma, lam, seed, tick, clip, members, risk, theta=None, plant_reset=None, history=None,
                    group_cost=None):
    """``vine_mpc_ensemble_update`` on the host: ``mpc.mpc_replay`` with the groups in the place of the samples -- ``group_costs``
    for the costs and ``group_actions`` for ``u``.  ``group_cost`` [M, G]: the group costs where they are not ``group_costs``'
    (the device's own, so that the weights are compared apart from them).  Returns ``mpc_replay``'s dict, whose ``u`` is [M, G,
    H, 2] and ``weights`` [M, G], and ``group_cost`` [M, G] and ``member_weights`` [M, K]."""
    nominal = np.asarray(nominal, dtype=np.float32)
    M = nominal.shape[0]
    cost = np.asarray(cost, dtype=np.float64).reshape(M, -1)
    K, E = cost.shape[1], int(members)
    C = group_costs(cost, E, risk, theta) if group_cost is None else np.asarray(group_cost, dtype=np.float64).reshape(M, K // E)
    u = group_actions(nominal, sigma, seed, K, E, tick, clip)
    r = mpc.mpc_replay(nominal, C.reshape(-1), sigma, lam, seed, tick, clip, plant_reset, history, u=u)
    r.update(group_cost=C, member_weights=np.repeat(r["weights"], E, axis=1))
    return r


# ---- the device
class EnsembleController(mpc.Controller):
    """``mpc.Controller`` whose K samples per plant are G sequences x E members: the members of a sequence are fed one action
    and differ in the model task's tables (``set_members``), and the update weights a sequence by ``RISK`` over their costs.

    ``control_step()`` = ``fork()``, ``ensemble_node()``, H x (``model.step_into`` + ``node()`` + ``ensemble_node()``), the
    update of include/vine_mpc_ensemble.h, the plant step: still one linear chain in a captured graph.  ``launches`` gains
    ``"ensemble"``.  ``keep_weights``: the last update's ``weights`` [N] and ``group_cost`` [M * G] are kept."""

    def __init__(self, plant_task, model_task, samples, ensemble, horizon=mpc.DEFAULTS["horizon"], lam=mpc.DEFAULTS["lambda"],
                 sigma=mpc.DEFAULTS["sigma"], seed=mpc.DEFAULTS["seed"], graph=True, graph_steps=1, keep_weights=False):
        import torch
        self.ensemble = ensemble_config(ensemble)
        super().__init__(plant_task, model_task, samples, horizon, lam, sigma, seed, graph=graph, graph_steps=graph_steps,
                         keep_weights=keep_weights)
        self.ecfg = ensemble_struct(self.ensemble, self.mcfg)
        self.E = self.ensemble["MEMBERS"]
        self.G = self.K // self.E
        self.group_cost = (torch.zeros(self.M * self.G, dtype=torch.float64, device=self.device) if keep_weights else None)
        self.launches["ensemble"] = 0

    def tensors(self):
        return super().tensors() + ([self.group_cost] if self.group_cost is not None else [])

    def ensemble_node(self):
        from .. import native
        native.check(self.lib.vine_mpc_ensemble_scheduled(
            self.model._handle, self.mcfg, self.ecfg, self.nominal.data_ptr(), self.tick.data_ptr(), self.window.data_ptr(),
            self.actions.data_ptr(), self._stream()), self.lib)
        self.launches["ensemble"] += 1

    def update(self):
        from .. import native
        native.check(self.lib.vine_mpc_ensemble_update(
            self.model._handle, self.mcfg, self.ecfg, self.cost.data_ptr(), self.plant.reset_buf.data_ptr(),
            self.nominal.data_ptr(), self.history.data_ptr(), self.tick.data_ptr(), self.plant_actions.data_ptr(),
            self.weights.data_ptr() if self.weights is not None else None,
            self.group_cost.data_ptr() if self.group_cost is not None else None, self._stream()), self.lib)
        self.launches["update"] += 1

    def after_fork(self):
        self.ensemble_node()

    def model_step(self):
        """One model step, the scoring node behind it and the group's next action behind that."""
        super().model_step()
        self.ensemble_node()

    def set_members(self, values):
        """``{name: array [M, E]}``: each plant's E values tiled over its G groups into the model's bound table(s),
        ``model.set_env_params``.  Not inside a graph capture; a captured graph reads the new table at its next replay."""
        for name, v in values.items():
            if np.shape(v) != (self.M, self.E):
                raise ValueError("set_members: %s takes an array [%d, %d], not %s" % (name, self.M, self.E, np.shape(v)))
        self.model.set_env_params(tile_members(values, self.G))


# ---- a run
class Play(mpc.PlayVariant):
    """``ensemble=`` of ``mpc.play``."""

    def check(self, run):
        self.spec = ensemble_config(self.spec)
        for key in mpc.VARIANTS + ("model_params",):
            if run.args.get(key) is not None:
                raise ConfigError("mpc: ensemble= together with %s= is refused: %s" % (key, (
                    "the members ARE the model's parameters" if key == "model_params" else
                    "that controller keeps its own update or its own model and was not built for groups of members")))
        ensemble_struct(self.spec, mpc.mpc_config(run.M, run.samples, *run.planner))
        self.seed = self.spec["SEED"] if self.spec["SEED"] is not None else int(run.planner[3]) + 1

    def bind(self, run):
        run.mcfg["env"]["ENV_PARAMS"] = copy.deepcopy(self.spec["params"])      # binds the model's table(s); filled in make()

    def make(self, run):
        E = self.spec["MEMBERS"]
        self.members = draw_members(self.spec["params"], run.model._vcfg, run.model._lib, self.seed, run.M, E)
        run.model.set_env_params(tile_members(self.members, int(run.samples) // E))

    def controller(self, run):
        return EnsembleController(run.plant, run.model, run.samples, self.spec, *run.planner, graph=run.graph)

    def banner(self, run):
        s = self.spec
        print("mpc: every sequence is scored on %d candidate plants drawn from %s (seed %d); RISK %s%s; %d sequences per plant" % (
            s["MEMBERS"], s["params"], self.seed, s["RISK"], "" if s["THETA"] is None else ", THETA %g" % s["THETA"],
            int(run.samples) // s["MEMBERS"]), flush=True)

    def result(self, run, out):
        s, ctl = self.spec, run.ctl
        stats = {name: {"mean": float(v.mean()), "min": float(v.min()), "max": float(v.max())} for name, v in self.members.items()}
        c = ctl.cost.cpu().numpy().reshape(ctl.M, ctl.G, ctl.E)                # the last update's member costs
        whole = np.isfinite(c).all(axis=2)
        spread = float((c.max(axis=2) - c.min(axis=2))[whole].mean()) if whole.any() else float("nan")
        table = run.model.env_params.cpu().numpy()                             # read back: what the samples were stepped with
        rows = {name: table[abi.ENV_PARAM_ROWS[name][0]].reshape(ctl.M, ctl.K) for name in self.members
                if name in abi.ENV_PARAM_ROWS and abi.ENV_PARAM_ROWS[name][1] == 1}
        out["ensemble"] = {"params": s["params"], "MEMBERS": s["MEMBERS"], "RISK": s["RISK"], "THETA": s["THETA"], "SEED": self.seed,
                           "values": dict(self.members), "members": stats, "model_table": rows, "disagreement": spread}
        for name, st in stats.items():
            print("mpc: ensemble members' %s: mean %.4g, min %.4g, max %.4g" % (name, st["mean"], st["min"], st["max"]), flush=True)
        print("mpc: the members of a sequence disagree by %.4g in cost (mean of max - min over the last update's groups)" % spread,
              flush=True)
