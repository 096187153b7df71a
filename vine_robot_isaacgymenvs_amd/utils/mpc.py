"""MPC on the host side: sampling-based predictive control (MPPI) of the plants of one handle with the samples of another.

The semantics are stated once, in include/vine_mpc.h.  A *plant* task of M envs is what is controlled; a *model* task of
M * K envs holds K samples per plant.  Every control step forks the samples from their plant's state (``vine_mpc_fork``),
rolls them H steps on noisy action sequences with a scoring node behind every step (``vine_mpc_scheduled``), averages the
sequences with weights from their costs (``vine_mpc_update``) and steps the plant on the first action.  What is left for
the host: the configuration (``mpc_config``, ``model_config``), the numpy statement every GPU test compares against
(``mpc_replay``), the buffers and the captured graph (``Controller``) and a run with its report (``play``); ``mpc.py`` at
the repository root is its command line."""
import contextlib
import copy
import logging
import time

import numpy as np

from .. import abi
from . import env_params, env_sensor
from .config import ConfigError

DEFAULTS = {"samples": 256, "horizon": 20, "lambda": 0.05, "sigma": 0.5, "seed": 0}
DEFAULT_COST = {"POSITION_REWARD_WEIGHT": 1.0}


# ---------------------------------------------------------------------------------------------------------- configuration
def check_integer(key, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ConfigError("mpc: %s must be an integer, not %r" % (key, v))
    if v < lo or (hi is not None and v > hi):
        raise ConfigError("mpc: %s must be %s, not %d" % (key, ">= %d" % lo if hi is None else "in %d .. %d" % (lo, hi), v))
    return int(v)


def check_real(key, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ConfigError("mpc: %s: %r is not a finite number" % (key, v))
    return float(v)


def mpc_config(num_plants, samples=DEFAULTS["samples"], horizon=DEFAULTS["horizon"], lam=DEFAULTS["lambda"],
               sigma=DEFAULTS["sigma"], seed=DEFAULTS["seed"]):
    """The checked ``abi.VineMpcConfig``: what include/vine_mpc.h refuses is refused here with a ``ConfigError`` naming the
    key (``plants``, ``samples``, ``horizon``, ``lambda``, ``sigma``, ``seed``).  ``sigma``: one number for both action
    components, or two."""
    c = abi.VineMpcConfig()
    c.abi_version = abi.MPC_ABI_VERSION
    c.num_plants = check_integer("plants", num_plants, 1)
    c.samples = check_integer("samples", samples, 2)
    c.horizon = check_integer("horizon", horizon, 1, abi.MPC_MAX_HORIZON)
    if c.num_plants * c.samples > 0x7FFFFFFF:
        raise ConfigError("mpc: plants * samples = %d does not fit an int32" % (c.num_plants * c.samples))
    lam = check_real("lambda", lam)
    if not lam > 0.0:
        raise ConfigError("mpc: lambda must be positive, not %g" % lam)
    c.lambda_ = lam
    pair = list(sigma) if isinstance(sigma, (list, tuple, np.ndarray)) else [sigma, sigma]
    if len(pair) != 2:
        raise ConfigError("mpc: sigma is one number or two, not %r" % (sigma,))
    for a, s in enumerate(pair):
        s = check_real("sigma", s)
        if s < 0.0 or s > float(np.finfo(np.float32).max):
            raise ConfigError("mpc: sigma must not be negative (and fit a float32), not %g" % s)
        c.sigma[a] = s
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed <= 0xFFFFFFFFFFFFFFFF:
        raise ConfigError("mpc: seed must be an integer in 0 .. 2^64 - 1, not %r" % (seed,))
    c.seed = int(seed)
    return c


FORCED = (
    # (section, key, value): what a batch of samples must be, whatever the plant's configuration says
    ("task", "vine_randomize", False),
    ("randomization_parameters", "OBSERVATION_NOISE_STD", 0.0),
    ("randomization_parameters", "ACTION_NOISE_STD", 0.0),
    ("env", "CAPTURE_VIDEO", False),
    ("env", "RECORD_TRAJECTORIES", False),
    ("env", "EPISODE_LOG", False),
    ("env", "MAT_FILE", ""),
    ("env", "ENV_PARAMS_PER_EPISODE", False),      # a sample keeps its plant: the model's table IS the model
    ("env", "ENV_PARAMS_ADR", {}),
    ("env", "ENV_SENSOR", {}),                     # the planner reads the state as it is
    ("env", "ENV_PUSH", {}),                       # ... and nothing but its own actions moves a sample
    ("env", "ENV_DRAW_ADR", {}),                   # ... and no range of those draws moves
    ("env", "ENV_TARGET", {}),                     # ... and no target moves by itself
)


def model_config(cfg, num_plants, samples, cost=None, logger=None):
    """A copy of the task config ``cfg`` (the plant's) with what a batch of samples needs forced, each change logged: no
    randomisation and no noise, no observer, no per-episode redraw, no ADR, no sensor and no push model, no MAT replay, and
    ``numEnvs = num_plants * samples``.  The obstacles, the three optional resets and ``maxEpisodeLength`` stay the plant's.
    ``cost``: ``{<NAME>_REWARD_WEIGHT: value}`` for the model only, on top of the task's own weights (default
    ``DEFAULT_COST``: the task's reward is sparse, and a planner with a short horizon needs a slope)."""
    logger = logger or logging.getLogger(__name__)
    cfg = copy.deepcopy(cfg)
    cfg["task"].setdefault("randomization_parameters", {})
    for section, key, value in FORCED:
        node = cfg["task"] if section == "task" else cfg["task"]["randomization_parameters"] if section != "env" else cfg["env"]
        if node.get(key, value) != value:
            logger.info("mpc: model %s.%s forced from %r to %r", section, key, node.get(key), value)
        node[key] = value
    n = int(num_plants) * int(samples)
    if int(cfg["env"]["numEnvs"]) != n:
        logger.info("mpc: model env.numEnvs set to %d plants x %d samples = %d", int(num_plants), int(samples), n)
        cfg["env"]["numEnvs"] = n
    cost = dict(DEFAULT_COST if cost is None else cost)
    for key, value in cost.items():
        if not str(key).endswith("_REWARD_WEIGHT") or key not in cfg["env"]:
            raise ConfigError("mpc: cost: %r is not a reward weight of the task (a *_REWARD_WEIGHT key of task.env)" % (key,))
        value = check_real("cost." + str(key), value)
        if cfg["env"][key] != value:
            logger.info("mpc: model env.%s set from %r to %r", key, cfg["env"][key], value)
        cfg["env"][key] = value
    return cfg


def make_task(cfg, device="cuda:0"):
    from ..tasks import isaacgym_task_map
    return isaacgym_task_map[cfg.get("name", "Vine5LinkMovingBase")](cfg=cfg, rl_device=device, sim_device=device,
                                                                    graphics_device_id=0, headless=True)


# ---------------------------------------------------------------------------------------------------- the launches, in numpy
def noise_deviate(seed, num_plants, samples, tick, horizon):
    """float32 [M, K, H, 2]: the deviate z of every (plant, sample, horizon step, component) at the plants' control steps
    ``tick`` ([M] or one number): the sensor's eight-uniform sum under purpose word ``abi.MPC_RNG_NOISE``; sample 0 has 0."""
    M, K, H = int(num_plants), int(samples), int(horizon)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    tick = np.broadcast_to(np.asarray(tick, dtype=np.int64), (M,)).astype(np.uint64)
    e = (np.arange(M * K, dtype=np.int64).reshape(M, K, 1) & 0xFFFFFFFF)
    c1 = (tick & np.uint64(0xFFFFFFFF)).reshape(M, 1, 1)
    c2 = (np.uint64(abi.MPC_RNG_NOISE) | (((tick >> np.uint64(32)) << np.uint64(8)) & np.uint64(0xFFFFFFFF))).reshape(M, 1, 1)
    w = env_sensor.philox4x32_10(e, c1, c2, np.arange(2 * H, dtype=np.int64).reshape(1, 1, -1), seed & 0xFFFFFFFF, seed >> 32)
    total = sum((x & np.uint32(0xFFFF)).astype(np.int64) + (x >> np.uint32(16)).astype(np.int64) for x in w)
    z = (2 * total - 524280).astype(np.float32).reshape(M, K, H, 2)
    z[:, 0] = 0.0
    return z


def sample_actions(nominal, sigma, seed, samples, tick, clip):
    """float32 [M, K, H, 2]: u of include/vine_mpc.h around ``nominal`` [M, H, 2] -- one float32 multiply, one float32 add,
    the clamp to +-``clip``."""
    nominal = np.asarray(nominal, dtype=np.float32)
    M, H = nominal.shape[0], nominal.shape[1]
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (2,))
    c = (sigma.astype(np.float64) * env_sensor.NOISE_SCALE).astype(np.float32)
    z = noise_deviate(seed, M, samples, tick, H)
    x = nominal[:, None] + z * c                                          # float32 throughout
    clip = np.float32(clip)
    return np.minimum(np.maximum(x, -clip), clip)


def cost_sums(rew, reset):
    """The node's sums on the host: ``rew`` [H, N] float32 and ``reset`` [H, N], the model's buffers behind each of the H
    steps.  Returns ``(cost float64 [N], alive uint8 [N])``."""
    rew = np.asarray(rew, dtype=np.float32)
    reset = np.asarray(reset) != 0
    n = rew.shape[1]
    cost, alive = np.zeros(n, dtype=np.float64), np.ones(n, dtype=bool)
    for k in range(rew.shape[0]):
        bad = alive & ~np.isfinite(rew[k])
        good = alive & np.isfinite(rew[k])
        cost[good] += -rew[k][good].astype(np.float64)
        cost[bad] = np.inf
        alive = alive & ~bad & ~(good & reset[k])
    return cost, alive.astype(np.uint8)


def mpc_replay(nominal, cost, sigma, lam, seed, tick, clip, plant_reset=None, history=None, u=None):
    """One control step's update on the host: the numpy statement of ``u``, the weights, the new nominal, the shift, the
    reset branch and the history.  ``nominal`` [M, H, 2] float32; ``cost`` [M * K] float64 (+inf allowed); ``tick`` [M];
    ``clip``: the model's clipActions; ``plant_reset`` [M] (default none raised); ``history`` [M, MAX_DELAY, 2] (default
    zeros); ``u`` [M, K, H, 2]: the samples' actions where they are not ``sample_actions``' (utils/mpc_noise.py).  Returns a
    dict: ``u`` [M, K, H, 2], ``weights`` [M, K] float64, ``new`` [M, H, 2] float32 (before the shift), ``nominal`` (after),
    ``plant_actions`` [M, 2], ``history``, ``tick``."""
    nominal = np.asarray(nominal, dtype=np.float32)
    M, H = nominal.shape[0], nominal.shape[1]
    cost = np.asarray(cost, dtype=np.float64).reshape(M, -1)
    K = cost.shape[1]
    tick = np.broadcast_to(np.asarray(tick, dtype=np.int64), (M,))
    u = sample_actions(nominal, sigma, seed, K, tick, clip) if u is None else np.asarray(u, dtype=np.float32)
    beta = cost.min(axis=1)
    finite = np.isfinite(beta)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(np.isfinite(cost), np.exp(-(cost - beta[:, None]) / np.float64(lam)), 0.0)
    w[~finite] = 0.0
    new = nominal.copy()
    for p in np.flatnonzero(finite):
        new[p] = ((w[p][:, None, None] * u[p].astype(np.float64)).sum(axis=0) / w[p].sum()).astype(np.float32)
    consumed = np.zeros(M, dtype=bool) if plant_reset is None else np.asarray(plant_reset).reshape(M) != 0
    shifted = np.concatenate([new[:, 1:], new[:, -1:]], axis=1)
    shifted[consumed] = 0.0
    act = new[:, 0].copy()
    act[consumed] = 0.0
    history = (np.zeros((M, abi.MAX_DELAY, 2), dtype=np.float32) if history is None
               else np.asarray(history, dtype=np.float32).reshape(M, abi.MAX_DELAY, 2))
    history = np.concatenate([act[:, None], history[:, :-1]], axis=1)
    return {"u": u, "weights": w, "new": new, "nominal": shifted, "plant_actions": act, "history": history,
            "tick": tick + 1}


# ------------------------------------------------------------------------------------------------------------ the device
class _Tasks:
    """The controller's tasks as the one env ``graph_capture.capture_rolled_back`` rolls back."""

    def __init__(self, tasks):
        self.tasks = tasks

    @property
    def step_count(self):
        return tuple(t.step_count for t in self.tasks)

    @step_count.setter
    def step_count(self, v):
        for t, c in zip(self.tasks, v):
            t.step_count = c

    @contextlib.contextmanager
    def observers_paused(self):
        with contextlib.ExitStack() as stack:
            for t in self.tasks:
                stack.enter_context(t.observers_paused())
            yield


class Controller:
    """The controller's buffers and launches for a plant task of M envs and a model task of M * K envs.

    ``control_step()`` = ``fork()``, H x ``model_step()`` (``model.step_into`` + ``node()``), ``update()``,
    ``plant.step_into(plant_actions, plant_obs)``, stated here alone: a variant extends ``model_step``, puts launches between
    those at ``after_fork``, ``before_update`` and ``after_update``, and in front of the fork or behind the plant step by
    wrapping ``control_step``.  ``run(n)`` issues n of them: a *unit* (``unit()``: here ``graph_steps`` control steps) is
    captured once as one hipGraph (``graph_capture.capture_rolled_back`` over ``tasks``) and replayed, the plant's observers
    told of every replay (``replay_observed``), wherever a whole unit is left and ``at_boundary()`` holds; every other step,
    or every step where a task is not capturable (``graph=False`` forces that), is an ``eager_step()``.  ``launches`` counts
    what the host enqueued, by kind."""

    def __init__(self, plant_task, model_task, samples, horizon=DEFAULTS["horizon"], lam=DEFAULTS["lambda"],
                 sigma=DEFAULTS["sigma"], seed=DEFAULTS["seed"], graph=True, graph_steps=1, keep_weights=False):
        import torch
        self.plant, self.model, self.lib = plant_task, model_task, plant_task._lib
        self.tasks = (plant_task, model_task)        # what a capture rolls back, in order
        self.fork_source = plant_task                # the task whose state the samples are forked from
        self.device = plant_task.device
        self.M, self.K, self.H = int(plant_task.num_envs), int(samples), int(horizon)
        self.mcfg = mpc_config(self.M, self.K, self.H, lam, sigma, seed)
        if int(model_task.num_envs) != self.M * self.K:
            raise ConfigError("mpc: the model task has %d envs, not plants * samples = %d * %d" % (
                int(model_task.num_envs), self.M, self.K))
        if model_task.device != self.device:
            raise ConfigError("mpc: the model task sits on %s, the plant on %s" % (model_task.device, self.device))
        N, dev, f32 = self.M * self.K, self.device, torch.float32
        self.nominal = torch.zeros((self.M, self.H, 2), dtype=f32, device=dev)
        self.history = torch.zeros((self.M, abi.MAX_DELAY, 2), dtype=f32, device=dev)
        self.tick = torch.zeros(self.M, dtype=torch.int64, device=dev)
        self.cost = torch.zeros(N, dtype=torch.float64, device=dev)
        self.alive = torch.ones(N, dtype=torch.uint8, device=dev)
        self.window = torch.zeros(1, dtype=torch.int64, device=dev)
        self.actions = torch.zeros((N, abi.NUM_ACTIONS), dtype=f32, device=dev)
        self.plant_actions = torch.zeros((self.M, abi.NUM_ACTIONS), dtype=f32, device=dev)
        self.model_obs = torch.zeros((N, model_task.num_obs), dtype=f32, device=dev)
        self.plant_obs = torch.zeros((self.M, plant_task.num_obs), dtype=f32, device=dev)
        # a diagnostic: the last update's weights (include/vine_mpc.h vine_mpc_update), stored only on request
        self.weights = torch.zeros(N, dtype=torch.float64, device=dev) if keep_weights else None
        self.graph_steps = self.unit_steps = max(1, int(graph_steps))
        self.use_graph = (bool(graph) and bool(getattr(plant_task, "graph_capturable", False))
                          and bool(getattr(model_task, "graph_capturable", False)) and getattr(plant_task, "video", None) is None)
        self.graph = None
        self.launches = {"fork": 0, "step": 0, "node": 0, "update": 0, "plant_step": 0}
        self.control_steps = 0

    def tensors(self):
        """Every tensor of the controller that a control step writes."""
        return [self.nominal, self.history, self.tick, self.cost, self.alive, self.window, self.actions, self.plant_actions,
                self.model_obs, self.plant_obs] + ([self.weights] if self.weights is not None else [])

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    # -- the three launches ----------------------------------------------------------------------------------------------
    def fork(self):
        from .. import native
        p, m = self.fork_source, self.model
        native.check(self.lib.vine_mpc_fork(
            p._handle, m._handle, self.mcfg, p.progress_buf.data_ptr(), self.nominal.data_ptr(), self.history.data_ptr(),
            self.tick.data_ptr(), self.actions.data_ptr(), m.rew_buf.data_ptr(), m.reset_buf.data_ptr(),
            m.progress_buf.data_ptr(), self.cost.data_ptr(), self.alive.data_ptr(), self.window.data_ptr(), self._stream()),
            self.lib)
        self.launches["fork"] += 1

    def node(self):
        from .. import native
        m = self.model
        native.check(self.lib.vine_mpc_scheduled(
            m._handle, self.mcfg, self.nominal.data_ptr(), self.tick.data_ptr(), self.window.data_ptr(),
            self.actions.data_ptr(), m.rew_buf.data_ptr(), m.reset_buf.data_ptr(), self.cost.data_ptr(),
            self.alive.data_ptr(), self._stream()), self.lib)
        self.launches["node"] += 1

    def update(self):
        from .. import native
        native.check(self.lib.vine_mpc_update(
            self.model._handle, self.mcfg, self.cost.data_ptr(), self.plant.reset_buf.data_ptr(), self.nominal.data_ptr(),
            self.history.data_ptr(), self.tick.data_ptr(), self.plant_actions.data_ptr(),
            self.weights.data_ptr() if self.weights is not None else None, self._stream()), self.lib)
        self.launches["update"] += 1

    def model_step(self):
        """One model step on the actions the fork or the node left, and the node behind it."""
        self.model.step_into(self.actions, self.model_obs)
        self.launches["step"] += 1
        self.node()

    def after_fork(self):
        pass

    def before_update(self):
        pass

    def after_update(self):
        pass

    def control_step(self):
        """One control step, eagerly (or into a capture)."""
        self.fork()
        self.after_fork()
        for _ in range(self.H):
            self.model_step()
        self.before_update()
        self.update()
        self.after_update()
        self.plant.step_into(self.plant_actions, self.plant_obs)
        self.launches["plant_step"] += 1

    # -- many of them ----------------------------------------------------------------------------------------------------
    def unit(self):
        """What one replay stands for: ``unit_steps`` control steps from a boundary."""
        for _ in range(self.unit_steps):
            self.control_step()

    def at_boundary(self):
        return True

    def eager_step(self):
        self.control_step()

    def _capture(self, body):
        """``body`` captured as one hipGraph, with nothing of it left behind but what one replay stands for: ``graph_launches``
        by kind and ``graph_num_steps`` per task of ``tasks``."""
        from ..learning import graph_capture
        counted, steps = dict(self.launches), [t.num_steps for t in self.tasks]
        live = self.tensors()
        for t in self.tasks:
            live = live + t.live_tensors()
        graph = graph_capture.capture_rolled_back(self.device, body, live, _Tasks(self.tasks))
        # the warm-up pass was rolled back and the capture pass executed nothing: what the capture pass enqueued is the graph
        self.graph_launches = {k: (v - counted[k]) // 2 for k, v in self.launches.items()}
        self.graph_num_steps = [(t.num_steps - n) // 2 for t, n in zip(self.tasks, steps)]
        self.launches = counted
        for t, n in zip(self.tasks, steps):
            t.num_steps = n
        return graph

    def run(self, n):
        """``n`` control steps."""
        from ..learning import graph_capture
        left, unit = int(n), self.unit_steps
        while left > 0:
            if self.use_graph and left >= unit and self.at_boundary():
                if self.graph is None:
                    self.graph = self._capture(self.unit)
                graph_capture.replay_observed(self.graph, self.plant, unit)
                for t, steps in zip(self.tasks, self.graph_num_steps):
                    t.num_steps += steps
                for k, v in self.graph_launches.items():
                    self.launches[k] += v
                left -= unit
            else:
                self.eager_step()
                left -= 1
        self.control_steps += int(n)

    # -- from outside the step -------------------------------------------------------------------------------------------
    def set_model_params(self, values):
        """``{name: array [M]}`` (or a scalar): each plant's value repeated over its K samples into the model's bound
        table(s), ``model.set_env_params``.  Not inside a graph capture; a captured graph reads the new table at its next
        replay."""
        out = {}
        for name, v in values.items():
            v = np.asarray(v, dtype=np.float64)
            if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != self.M):
                raise ValueError("set_model_params: %s takes a scalar or an array [%d], not %s" % (name, self.M, v.shape))
            out[name] = np.repeat(v, self.K) if v.ndim == 1 else v
        self.model.set_env_params(out)

    def reset_plants(self, ids):
        """Plants reset from outside the step (``plant.reset_idx``), and ``clear_rows`` for them."""
        import torch
        ids = torch.as_tensor(ids, device=self.device).to(torch.long)
        if ids.numel() == 0:
            return
        self.plant.reset_idx(ids)
        self.clear_rows(ids)

    def clear_rows(self, ids):
        """What the controller keeps of the plants ``ids`` (a long tensor, not empty) starts anew: their nominal sequence
        and action history.  A variant adds its own rows."""
        self.nominal[ids] = 0.0
        self.history[ids] = 0.0


# ------------------------------------------------------------------------------------------------------------------ a run
def draw_model_params(spec, vcfg, lib, seed, num_plants):
    """``{name: float64 [M]}``: an ``ENV_PARAMS``-style ``spec`` drawn once per plant with ``env_params``' own draw (global
    env id = the plant's index): the value itself, a factor for the FPAM vectors and the link masses."""
    draws = {}
    env_params.draw_table(spec, env_params.config_row(lib, vcfg), seed, num_plants, draws=draws)
    return draws


# What play() refuses, checked in this order before any task is created: the first entry whose keys all hold raises its message.
# A key is a keyword of play() that was given, ``terminal_value`` where it is not zero, ``ENV_TARGET`` where the plant's
# task.env has a target spec that is not empty; ``!key``: the key does not hold.
RULES = (
    (("track", "!ENV_TARGET"), "mpc: track= needs a plant with task.env.ENV_TARGET: there is no path to follow"),
    (("track", "policy"), "mpc: track= together with policy= is refused: the samples' observation would need the target's velocity columns"),
    (("track", "adapt"), "mpc: track= together with adapt= is refused: the adaptive controller's traces were built for a resting target"),
    (("track", "observe"), "mpc: track= together with observe= or filter= is refused: the predictor was built for a resting target"),
    (("track", "filter"), "mpc: track= together with observe= or filter= is refused: the predictor was built for a resting target"),
    (("filter", "!observe"), "mpc: filter= needs observe=: the frames it corrects are the sensing path's"),
    (("filter", "observe", "adapt"), "mpc: filter= together with adapt= is refused: the adaptive controller traces the plant's exact state"),
    (("filter", "observe", "policy"), "mpc: filter= together with policy= is refused: the policy's memory is forked from the plant's exact state"),
    (("observe", "adapt"), "mpc: observe= together with adapt= is refused: the adaptive controller traces the plant's exact state"),
    (("observe", "policy"), "mpc: observe= together with policy= is refused: the policy's memory is forked from the plant's exact state"),
    (("terminal_value", "!policy"), "mpc: terminal_value needs policy=<checkpoint>: the critic is the policy's"),
    (("policy", "adapt"), "mpc: policy= together with adapt= is refused: the adaptive controller does not roll the policy yet"),
)


def refuse(holding):
    """A ``ConfigError`` with the message of the first entry of ``RULES`` that the set of keys ``holding`` meets."""
    for keys, message in RULES:
        if all(k[1:] not in holding if k.startswith("!") else k in holding for k in keys):
            raise ConfigError(message)


class PlayVariant:
    """What one keyword of ``play`` adds to a run.  Each variant's module states its own once, as ``Play``, and ``play`` walks
    those given in the order of ``VARIANTS``, calling what each defines of: ``check(run)``, the argument ``spec`` checked before
    any task is created; ``bind(run)``, the model's task config edited; ``make(run)``, what must exist before the controller (a
    third task, a network); ``controller(run)``, asked of the last one given only; ``banner(run)``; ``stepped(ctl)`` behind every
    ``ctl.run(1)``; ``result(run, out)``, its entries of the result and its lines in front of the timing; ``report_rows(run,
    rows)``, columns added to the finished episodes; ``epilogue(run, out)`` behind the report.  ``run``: what ``play`` knows, by
    name -- ``cfg`` and ``mcfg`` (the plant's and the model's task config), ``M``, ``samples``, ``planner`` (horizon, lambda,
    sigma, seed: a controller's next four arguments), ``graph``, ``steps``, ``device``, ``model_params``, ``draws`` (the model's
    drawn parameters still to be set, or ``None``), ``args`` (``play``'s keywords), ``given`` (the variants by key) and, once
    made, ``plant``, ``model``, ``predictor``, ``ctl``."""
    single_run = False         # True: one ``ctl.run(steps)`` that sums ``ctl.returns``, not ``run(1)`` + ``plant.rew_buf`` per step
    report_params = False      # True: the report takes the plant's parameter columns even where it has no ENV_PARAMS

    def __init__(self, spec):
        self.spec = spec

    def controller(self, run):
        return Controller(run.plant, run.model, run.samples, *run.planner, graph=run.graph)


# the order they are walked in; each is utils/mpc_<key>.Play.  "noise" stands alone, and stands first: its check is the refusal of
# every other, which must come before any of theirs (it is not in RULES, whose keys a test pins)
VARIANTS = ("noise", "track", "observe", "filter", "policy", "adapt")
# ... and in front of them all, from a tuple of its own (a test pins VARIANTS): "ensemble" (utils/mpc_ensemble.Play), whose check
# is the refusal of every key of VARIANTS and of model_params=, as noise's is of the others
FIRST = ("ensemble",)


def play(cfg, plants=None, samples=DEFAULTS["samples"], horizon=DEFAULTS["horizon"], lam=DEFAULTS["lambda"],
         sigma=DEFAULTS["sigma"], steps=500, cost=None, model_params=None, seed=None, device="cuda:0", graph=True,
         logger=None, adapt=None, policy=None, terminal_value=0.0, policy_params=None, observe=None, filter=None, track=None,
         noise=None, ensemble=None):
    """Run ``steps`` control steps of MPC on the task config ``cfg`` (the ``task`` block of the composed configuration; its
    ``env.numEnvs`` plants unless ``plants`` is given) and report through the plant's ``EPISODE_LOG`` when it is on:
    ``episodes.report`` of the episodes finished in the run, and ``reached_ever_rate`` by every varying plant parameter when
    the plant has ``ENV_PARAMS`` -- the numbers ``test=True`` prints for the policy.  ``model_params``: an ``ENV_PARAMS``-style
    spec for the MODEL, drawn once per plant and repeated over its samples (default: the model is the configuration's own
    plant).  Returns a dict: ``report`` (or ``None``), ``by_param``, ``path`` (the log's ``.npz``), ``control_steps_per_second``,
    ``plant_return`` (float64 [M], the summed plant reward) and ``controller``'s launch counts.

    ``adapt``: a spec of ``mpc_adapt.adapt_config`` -- the model follows each plant online (include/vine_mpc_adapt.h), with
    ``forget_on_reset`` when the plant has ``ENV_PARAMS_PER_EPISODE``.  The result then holds ``adapt``: ``names``, the final
    ``mean`` and ``std`` [M, D], ``prior_mean``, and, where the plant carries an ``ENV_PARAMS`` table, ``truth`` and per name
    the mean absolute error of the prior and of the final belief (printed too).  With ``masses`` in the spec the belief carries
    mass dimensions too (include/vine_mpc_adapt_inertia.h, ``mpc_adapt_inertia.AdaptiveInertiaController``) and ``adapt`` gains
    ``mass_names``, ``mass_mean``, ``mass_std``, ``mass_prior_mean`` and ``mass_truth``.  Without it nothing of this is launched.

    ``policy``: a checkpoint of ``train.py`` -- the samples roll that policy and the planner's sequence is a residual on its
    mean (include/vine_mpc_policy.h, ``mpc_policy.PolicyController``); ``policy_params`` is the ``train.params`` block of the
    composed configuration the network is built from, as ``train.py test=True`` builds it; ``terminal_value``: the weight of
    the critic's value behind the horizon (0: the extra inference and the terminal launch are not issued).  The result then
    holds ``policy`` (the path).  ``policy`` together with ``adapt`` is refused.  Without it nothing of this is launched.

    ``observe``: a spec of ``mpc_observe.observe_config`` -- the planner sees each plant through a delayed, noisy sensor of
    its own and predicts the delivered frame forward through a third task, the predictor (include/vine_mpc_observe.h,
    ``mpc_observe.ObservingController``).  The result then holds ``observe``: the per-plant ``table`` [4, M], its ``names``,
    ``catchup``, ``compensate`` and the mean ``lag``.  ``observe`` together with ``adapt`` or ``policy`` is refused.  Without
    it nothing of this is constructed or launched.

    ``filter``: a spec of ``mpc_filter.filter_config`` -- a fixed-gain corrector over successive frames (include/vine_mpc_filter.h,
    ``mpc_filter.FilteringController``): the pin and the catch-up are delivered its estimate instead of the raw frame.  It needs
    ``observe=`` and is refused together with ``adapt`` or ``policy``, and where the largest ``DELAY`` plus the model's largest
    ``ACTION_DELAY`` reaches beyond the action log.  The result then holds ``filter``: the per-plant ``gain`` [2, M], its
    ``names`` and the mean ``innov`` [2]; the per-parameter report has ``param_FILTER_<NAME>`` for a gain that varies.  Without
    it nothing of this is constructed or launched.

    ``track``: a spec of ``mpc_track.track_config``, ``{PATH: exact | linear | held}`` -- the samples' targets move over the
    horizon along their plant's ``ENV_TARGET`` path (include/vine_mpc_track.h, ``mpc_track.TrackingController``).  It needs a
    plant with ``task.env.ENV_TARGET`` and is refused together with ``policy`` (the samples' observation would need the
    velocity columns) and with ``adapt``, ``observe`` or ``filter`` (their third handles and traces were built for a resting
    target).  The result then holds ``track``: ``PATH`` and ``live_fraction``, the share of (plant, control step) pairs whose
    samples followed a path; the per-parameter report has the plant's varying ``param_TARGET_*`` columns.  Without it nothing
    of this is constructed or launched.

    ``noise``: a spec of ``mpc_noise.noise_config``, ``{BETA: 0.8}`` or ``{BETA: [0.9, 0.7], ADAPT: {RATE: .., SIGMA_MIN: ..,
    SIGMA_MAX: ..}}`` -- the samples' perturbations are correlated over the horizon and, with ``ADAPT``, each plant's amplitude
    follows the spread of the samples its weights preferred (include/vine_mpc_noise.h, ``mpc_noise.NoiseController``).  It is
    refused together with every other variant (``mpc_noise.Play.check``, not ``RULES``: they compute their own perturbations).
    The result then holds ``noise``: ``BETA``, ``ADAPT`` and the mean, minimum and maximum of the final ``sigma_p``.  Without it
    nothing of this is constructed or launched.

    ``ensemble``: a spec of ``mpc_ensemble.ensemble_config``, ``{params: {DAMPING: [0.005, 0.1], ...}, MEMBERS: 4, RISK: mean | max
    | entropic, THETA: .., SEED: ..}`` -- a plant's samples are ``samples / MEMBERS`` action sequences, each rolled through
    ``MEMBERS`` candidate plants drawn from ``params`` once per run, and a sequence is weighted by ``RISK`` over its members' costs
    (include/vine_mpc_ensemble.h, ``mpc_ensemble.EnsembleController``): the planner knows the range of its plant, as a
    domain-randomised policy does.  It is refused together with every key of ``VARIANTS`` and with ``model_params``
    (``mpc_ensemble.Play.check``, not ``RULES``), and where ``samples`` is no multiple of ``MEMBERS``.  The result then holds
    ``ensemble``: the spec, the seed of the draw, per parameter the members' mean, minimum and maximum, and ``disagreement``, the
    mean over the last update's sequences of the largest minus the smallest member cost.  Without it nothing of this is
    constructed or launched."""
    import importlib
    import types

    import torch
    from . import episodes
    logger = logger or logging.getLogger(__name__)
    cfg = copy.deepcopy(cfg)
    if len(cfg["env"].get("ENV_DRAW_ADR") or {}):      # the plants are measured on the whole of what they may meet
        logger.info("mpc: plant env.ENV_DRAW_ADR is forced off, the sensor, the push and the target draw from their full limits")
        cfg["env"]["ENV_DRAW_ADR"] = {}
    if plants is not None:
        cfg["env"]["numEnvs"] = check_integer("plants", plants, 1)
    M = int(cfg["env"]["numEnvs"])
    seed = cfg.get("seed", 0) if seed is None else seed
    seed = int(seed) if isinstance(seed, (int, np.integer)) and seed >= 0 else 0
    mpc_config(M, samples, horizon, lam, sigma, seed)                      # refuse a bad key before anything is created
    args = {"adapt": adapt, "policy": policy, "terminal_value": terminal_value, "policy_params": policy_params,
            "observe": observe, "filter": filter, "track": track, "noise": noise, "ensemble": ensemble,
            "model_params": model_params}
    refuse({k for k in VARIANTS if args[k] is not None} | ({"terminal_value"} if terminal_value else set())
           | ({"ENV_TARGET"} if cfg["env"].get("ENV_TARGET") else set()))
    given = {k: importlib.import_module(".mpc_" + k, __package__).Play(args[k]) for k in FIRST + VARIANTS if args[k] is not None}
    active = list(given.values())

    def each(what, *a):
        for v in active:
            getattr(v, what, lambda *a: None)(*a)

    run = types.SimpleNamespace(cfg=cfg, M=M, samples=samples, planner=(horizon, lam, sigma, seed), graph=graph, steps=int(steps),
                                device=device, model_params=model_params, draws=None, args=args, given=given, plant=None,
                                model=None, predictor=None, ctl=None)
    each("check", run)
    run.mcfg = mcfg = model_config(cfg, M, samples, cost, logger)
    if model_params:
        env_params.spec_forms(model_params)
        mcfg["env"]["ENV_PARAMS"] = copy.deepcopy(dict(model_params))       # binds the model's table(s); filled per plant below
    elif mcfg["env"].get("ENV_PARAMS"):
        logger.info("mpc: model env.ENV_PARAMS forced from %r to {} (the model is the configuration's own plant)",
                    mcfg["env"]["ENV_PARAMS"])
        mcfg["env"]["ENV_PARAMS"] = {}
    each("bind", run)
    run.plant = plant = make_task(cfg, device)
    try:
        run.model = model = make_task(mcfg, device)
        if model_params:
            run.draws = draw_model_params(model_params, model._vcfg, model._lib, seed, M)
        each("make", run)
        run.ctl = ctl = (active[-1] if active else PlayVariant(None)).controller(run)
        if run.draws:
            ctl.set_model_params(run.draws)
        each("banner", run)
        log = getattr(plant, "episode_log", None)
        start = None
        if log is not None:
            log.harvest()
            start = int(plant.step_count)
        print("mpc: %d plants x %d samples, horizon %d, lambda %g, sigma %s, %s; model step kernel %s" % (
            M, ctl.K, ctl.H, float(lam), sigma, "hipGraph replay" if ctl.use_graph else "eager launches",
            model.step_kernel_name), flush=True)
        total = torch.zeros(M, dtype=torch.float64, device=plant.device)
        torch.cuda.synchronize(plant.device)
        t0 = time.perf_counter()
        if any(v.single_run for v in active):            # whole units replay from one graph: the controller sums the reward
            ctl.run(int(steps))
            total += ctl.returns
        else:
            for _ in range(int(steps)):
                ctl.run(1)
                total += plant.rew_buf
                each("stepped", ctl)
        torch.cuda.synchronize(plant.device)
        seconds = time.perf_counter() - t0
        out = {"report": None, "by_param": {}, "path": None, "control_steps_per_second": int(steps) / max(seconds, 1e-9),
               "plant_return": total.cpu().numpy(), "launches": dict(ctl.launches), "graphed": ctl.use_graph,
               "model_step_kernel": model.step_kernel_name, "model_table_bound": model.env_params is not None}
        each("result", run, out)
        print("mpc: %d control steps in %.3f s (%.4g control steps/s, %.4g model env-steps/s)" % (
            int(steps), seconds, out["control_steps_per_second"], out["control_steps_per_second"] * M * ctl.K * ctl.H), flush=True)
        if log is not None:
            from ..learning.player import format_report
            log.harvest()
            with_params = plant.env_params is not None or any(v.report_params for v in active)
            rows = log.rows_with_params() if with_params else log.rows()
            keep = rows["end_step"] >= start
            rows = {k: v[keep] for k, v in rows.items()}
            each("report_rows", run, rows)
            out["report"] = episodes.report(rows)
            print(format_report(out["report"]), flush=True)
            for column in [k for k in rows if k.startswith("param_")]:
                if not len(rows["env"]):
                    print("  reached_ever_rate by %s: no episode finished" % column, flush=True)
                    continue
                rate, count, edges = episodes.binned_rate(rows, column, 5)
                out["by_param"][column] = (edges, rate, count)
                print("  reached_ever_rate by %s:" % column, flush=True)
                for i in range(len(rate)):
                    print("    [%.4g, %.4g%s  %.4g  (%d episodes)" % (edges[i], edges[i + 1], "]" if i == len(rate) - 1 else ")",
                                                                      rate[i], count[i]), flush=True)
            out["path"] = log.path                       # (written when the plant is closed, below)
        each("epilogue", run, out)
        return out
    finally:
        for task in (run.predictor, run.model, plant):
            if task is not None:
                task.close()
