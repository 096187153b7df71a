"""MPC_ADAPT on the host side: the predictive controller of utils/mpc.py fits its model to each plant online.

The semantics are stated once, in include/vine_mpc_adapt.h.  Every ``every`` control steps the K samples of each plant become
K candidate plants drawn around that plant's belief (``mean``, ``std`` per adapted dimension), are put back onto the plant's
state at the cycle's start (``vine_mpc_adapt_pin``), fed the actions the plant received and scored against what the plant did
(``vine_mpc_adapt_scheduled``); the belief moves to the weighted mean (``vine_mpc_adapt_estimate``), which is written into
the model's bound parameter table, and the planner plans with it from then on.  What is left for the host: the configuration
(``adapt_config``), the numpy statements every GPU test compares against (``candidates``, ``table_rows``, ``score``,
``estimate``) and the buffers and the captured graph (``AdaptiveController``)."""
import numpy as np

from .. import abi
from . import env_sensor
from .config import ConfigError
from .mpc import DEFAULTS as MPC_DEFAULTS
from .mpc import Controller, PlayVariant, check_integer, check_real

# temperature, rate, spread and floor: see DESIGN.md section 25 ("The four constants") for what they were checked against
DEFAULTS = {"window": 8, "every": 8, "min_steps": 4, "temperature": 0.1, "rate": 0.5, "spread": 0.25, "floor": 0.01}
KEYS = ("params", "masses") + tuple(DEFAULTS) + ("weights",)      # masses: utils/mpc_adapt_inertia.py
REFUSED = {
    "ACTION_DELAY": "an integer: its belief is not Gaussian, and a weighted mean of delays is no delay",
    "CART_MASS": "it lives in the inertia table, whose derived rows need the composites formed on the host",
    "LINK_MASS": "it lives in the inertia table, whose derived rows need the composites formed on the host",
    "TIP_LINK_MASS": "it lives in the inertia table, whose derived rows need the composites formed on the host",
}
FIELD_NAMES = tuple("q%d" % i for i in range(6)) + tuple("qd%d" % i for i in range(6))


# ---------------------------------------------------------------------------------------------------------- configuration
def adapt_config(spec, num_plants, samples, base_row, seed=0, forget_on_reset=False):
    """``(abi.VineMpcAdaptConfig, names)`` of an ``adapt`` spec: ``{params: {NAME: [lo, hi], ..}, window, every, min_steps,
    temperature, rate, spread, floor, weights}``.  ``params`` names rows of the ``ENV_PARAMS`` table (an FPAM vector's value
    is a factor on the model configuration's five constants); ``weights`` maps ``q0..q5`` / ``qd0..qd5`` to the score's
    weights (default 1 on the six q).  ``base_row``: the model configuration's ``env_params.config_row``.  ``std_floor`` of a
    dimension is ``floor * (hi - lo)``.  What include/vine_mpc_adapt.h refuses is refused here with a ``ConfigError`` naming
    the key."""
    if not hasattr(spec, "keys"):
        raise ConfigError("mpc adapt: adapt={params: {NAME: [lo, hi]}, ...} must be a mapping, not %r" % (spec,))
    for key in spec.keys():
        if key not in KEYS:
            raise ConfigError("mpc adapt: unknown key %r (known: %s)" % (key, ", ".join(KEYS)))
    params = spec.get("params")
    if not hasattr(params, "keys") or len(params) == 0:
        raise ConfigError("mpc adapt: params must be a non-empty mapping {NAME: [lo, hi]}, not %r" % (params,))
    c = abi.VineMpcAdaptConfig()
    c.abi_version = abi.MPC_ADAPT_ABI_VERSION
    c.num_plants = check_integer("adapt plants", num_plants, 1)
    c.samples = check_integer("adapt samples", samples, 2)
    c.window = check_integer("adapt.window", spec.get("window", DEFAULTS["window"]), 1, abi.MPC_ADAPT_MAX_WINDOW)
    c.every = check_integer("adapt.every", spec.get("every", max(DEFAULTS["every"], c.window)), 1)
    if c.every < c.window:
        raise ConfigError("mpc adapt: every = %d must be at least window = %d (a cycle traces its first `window` steps)" % (
            c.every, c.window))
    c.min_steps = check_integer("adapt.min_steps", spec.get("min_steps", min(DEFAULTS["min_steps"], c.window)), 1, c.window)
    c.temperature = check_real("adapt.temperature", spec.get("temperature", DEFAULTS["temperature"]))
    if not c.temperature > 0.0:
        raise ConfigError("mpc adapt: temperature must be positive, not %g" % c.temperature)
    c.rate = check_real("adapt.rate", spec.get("rate", DEFAULTS["rate"]))
    if not 0.0 < c.rate <= 1.0:
        raise ConfigError("mpc adapt: rate must be in (0, 1], not %g" % c.rate)
    spread = check_real("adapt.spread", spec.get("spread", DEFAULTS["spread"]))
    floor = check_real("adapt.floor", spec.get("floor", DEFAULTS["floor"]))
    if spread < 0.0 or floor < 0.0:
        raise ConfigError("mpc adapt: spread and floor must not be negative, not %g and %g" % (spread, floor))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed <= 0xFFFFFFFFFFFFFFFF:
        raise ConfigError("mpc adapt: seed must be an integer in 0 .. 2^64 - 1, not %r" % (seed,))
    c.seed = int(seed)
    c.forget_on_reset = int(bool(forget_on_reset))
    weights = spec.get("weights")
    if weights is None:
        weights = {name: 1.0 for name in FIELD_NAMES[:6]}
    if not hasattr(weights, "keys"):
        raise ConfigError("mpc adapt: weights must be a mapping of %s, not %r" % (", ".join(FIELD_NAMES), weights))
    for name, w in weights.items():
        if name not in FIELD_NAMES:
            raise ConfigError("mpc adapt: weights: unknown field %r (known: %s)" % (name, ", ".join(FIELD_NAMES)))
        w = check_real("adapt.weights." + name, w)
        if w < 0.0 or w > float(np.finfo(np.float32).max):
            raise ConfigError("mpc adapt: weights.%s must not be negative (and fit a float32), not %g" % (name, w))
        c.weights[FIELD_NAMES.index(name)] = w
    base_row = np.asarray(base_row, dtype=np.float32)
    for r in range(abi.MPC_ADAPT_BASE_ROWS):
        c.base_rows[r] = float(base_row[abi.VP_FPAM_K0 + r])
    names = list(params.keys())
    if len(names) > abi.MPC_ADAPT_MAX_DIMS:
        raise ConfigError("mpc adapt: params holds %d names, at most %d" % (len(names), abi.MPC_ADAPT_MAX_DIMS))
    c.num_dims = len(names)
    for d, name in enumerate(names):
        if name in REFUSED:
            raise ConfigError("mpc adapt: params.%s is refused: %s" % (name, REFUSED[name]))
        if name not in abi.ENV_PARAM_ROWS:
            raise ConfigError("mpc adapt: params: unknown parameter %r (known: %s)" % (
                name, ", ".join(n for n in abi.ENV_PARAM_NAMES if n not in REFUSED)))
        entry = params[name]
        if not isinstance(entry, (list, tuple)) or len(entry) != 2:
            raise ConfigError("mpc adapt: params.%s must be a range [lo, hi], not %r" % (name, entry))
        lo, hi = check_real("adapt.params." + name, entry[0]), check_real("adapt.params." + name, entry[1])
        if lo > hi:
            raise ConfigError("mpc adapt: params.%s: lo > hi in [%g, %g]" % (name, lo, hi))
        first, count = abi.ENV_PARAM_ROWS[name]
        c.dims[d].first_row, c.dims[d].num_rows = first, count
        c.dims[d].lo, c.dims[d].hi, c.dims[d].std_floor = lo, hi, floor * (hi - lo)
    c.spread = spread                                     # (a Python attribute, not a field: the prior's std / (hi - lo))
    return c, names


def dims_of(cfg):
    """``[(first_row, num_rows, lo, hi, std_floor), ..]`` of a configuration."""
    return [(m.first_row, m.num_rows, m.lo, m.hi, m.std_floor) for m in list(cfg.dims)[:cfg.num_dims]]


# ---------------------------------------------------------------------------------------------------- the launches, in numpy
def deviate(seed, num_plants, samples, passes, num_dims, purpose=None):
    """float32 [M, K, D]: z of include/vine_mpc_adapt.h -- the eight-uniform sum under purpose word ``abi.MPC_ADAPT_RNG``,
    float32(float64(2 S - 524280) * K0); candidate 0 has 0."""
    M, K, D = int(num_plants), int(samples), int(num_dims)
    purpose = abi.MPC_ADAPT_RNG if purpose is None else int(purpose)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    t = np.broadcast_to(np.asarray(passes, dtype=np.int64), (M,)).astype(np.uint64)
    e = (np.arange(M * K, dtype=np.int64).reshape(M, K, 1) & 0xFFFFFFFF)
    c1 = (t & np.uint64(0xFFFFFFFF)).reshape(M, 1, 1)
    c2 = (np.uint64(purpose) | (((t >> np.uint64(32)) << np.uint64(8)) & np.uint64(0xFFFFFFFF))).reshape(M, 1, 1)
    w = env_sensor.philox4x32_10(e, c1, c2, np.arange(D, dtype=np.int64).reshape(1, 1, -1), seed & 0xFFFFFFFF, seed >> 32)
    total = sum((x & np.uint32(0xFFFF)).astype(np.int64) + (x >> np.uint32(16)).astype(np.int64) for x in w)
    z = ((2 * total - 524280).astype(np.float64) * env_sensor.NOISE_SCALE).astype(np.float32).reshape(M, K, D)
    z[:, 0] = 0.0
    return z


def candidates(mean, std, dims, seed, samples, passes):
    """float64 [M, K, D]: theta of every candidate -- one float64 multiply, one add, the clamp to the dimension's range."""
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    M, D = mean.shape
    z = deviate(seed, M, samples, passes, D).astype(np.float64)
    x = mean[:, None, :] + z * std[:, None, :]
    lo = np.array([d[2] for d in dims], dtype=np.float64)
    hi = np.array([d[3] for d in dims], dtype=np.float64)
    return np.minimum(np.maximum(x, lo), hi)


def table_rows(theta, dims, base_row):
    """``{row: float32 [...]}``: the table values of ``theta`` [..., D] in the rounding of ``env_params.set_rows``."""
    theta = np.asarray(theta, dtype=np.float64)
    base = np.asarray(base_row, dtype=np.float32).astype(np.float64)
    out = {}
    for d, (first, count, _lo, _hi, _floor) in enumerate(dims):
        for r in range(first, first + count):
            out[r] = (theta[..., d] if count == 1 else base[r] * theta[..., d]).astype(np.float32)
    return out


def score(states, resets, trace_rows, trace_len, weights, samples):
    """The score node's sums on the host.  ``states`` float32 [W, 12, N]: the model's twelve joint fields behind each of the
    W steps; ``resets`` [W, N]; ``trace_rows`` float32 [M, W, 12]; ``trace_len`` [M].  Returns ``(err float64 [N], alive
    uint8 [N])``."""
    states = np.asarray(states, dtype=np.float32)
    W, _, N = states.shape
    K = int(samples)
    plant_of = np.arange(N) // K
    w = np.asarray(weights, dtype=np.float32)
    used = np.flatnonzero(w != 0)
    tl = np.asarray(trace_len).astype(np.int64)[plant_of]
    rows = np.asarray(trace_rows, dtype=np.float32)
    err, alive = np.zeros(N, dtype=np.float64), np.ones(N, dtype=bool)
    for k in range(1, W + 1):
        x = states[k - 1]
        on = alive & (k <= tl)
        finite = np.isfinite(x[used]).all(axis=0) if len(used) else np.ones(N, dtype=bool)
        total = np.zeros(N, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            for f in used:
                dx = x[f].astype(np.float64) - rows[plant_of, k - 1, f].astype(np.float64)
                total = total + np.float64(w[f]) * (dx * dx)
        good, bad = on & finite, on & ~finite
        err[good] = err[good] + total[good]
        left = good & (np.asarray(resets[k - 1]) != 0) & (k < tl)
        err[bad | left] = np.inf
        alive &= ~(bad | left)
    return err, alive.astype(np.uint8)


def estimate(err, theta, mean, std, prior_mean, prior_std, trace_len, episode_ended, dims, min_steps, temperature, rate,
             forget_on_reset=False):
    """The estimate on the host (include/vine_mpc_adapt.h 5): ``err`` float64 [M * K] (+inf allowed), ``theta`` [M, K, D] the
    candidates of this pass.  Returns a dict: ``mean``, ``std`` [M, D], ``weights`` [M, K], ``estimated`` and ``forgot``
    bool [M], ``plan`` [M, D] (the planning value: the new mean clamped to the range)."""
    mean, std = np.array(mean, dtype=np.float64), np.array(std, dtype=np.float64)
    M, D = mean.shape
    err = np.asarray(err, dtype=np.float64).reshape(M, -1)
    theta = np.asarray(theta, dtype=np.float64)
    K = err.shape[1]
    rate, temperature = np.float64(rate), np.float64(temperature)
    w = np.zeros((M, K), dtype=np.float64)
    estimated, forgot = np.zeros(M, dtype=bool), np.zeros(M, dtype=bool)
    for p in range(M):
        fin = np.isfinite(err[p])
        if forget_on_reset and np.asarray(episode_ended).reshape(M)[p]:
            mean[p], std[p], forgot[p] = np.asarray(prior_mean, dtype=np.float64)[p], np.asarray(prior_std, dtype=np.float64)[p], True
            continue
        if int(np.asarray(trace_len).reshape(M)[p]) < int(min_steps) or not fin.any():
            continue
        beta = err[p][fin].min()
        ebar = err[p][fin].sum() / np.float64(fin.sum())
        tau = temperature * (ebar - beta)
        if tau > 0.0:
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                w[p] = np.where(fin, np.exp(-(err[p] - beta) / tau), 0.0)
        else:
            w[p] = fin.astype(np.float64)
        sw = w[p].sum()
        for d in range(D):
            m = (w[p] * theta[p, :, d]).sum() / sw
            dv = theta[p, :, d] - m
            v = (w[p] * (dv * dv)).sum() / sw
            keep = np.float64(1.0) - rate
            new_mean = keep * mean[p, d] + rate * m
            new_std = max(keep * std[p, d] + rate * np.sqrt(v), np.float64(dims[d][4]))
            mean[p, d], std[p, d] = new_mean, new_std
        estimated[p] = True
    lo = np.array([d[2] for d in dims], dtype=np.float64)
    hi = np.array([d[3] for d in dims], dtype=np.float64)
    return {"mean": mean, "std": std, "weights": w, "estimated": estimated, "forgot": forgot,
            "plan": np.minimum(np.maximum(mean, lo), hi)}


# ------------------------------------------------------------------------------------------------------------ the device
class AdaptiveController(Controller):
    """A ``Controller`` whose model follows its plants: the extra buffers of include/vine_mpc_adapt.h and the five launches.

    A cycle is ``anchor()``, ``every`` x (``control_step()`` + ``trace()``), ``pin()``, ``window`` x (model step +
    ``score()``), ``estimate()``.  ``run(n)`` issues n control steps: the unit of ``Controller.run`` is ``graph_cycles`` whole
    cycles, replayed from one captured hipGraph where they start on a cycle's boundary; what is left over is issued eagerly
    with the phase (control steps done in the running cycle) kept on the host.  The model task must have a parameter table
    bound (``task.env.ENV_PARAMS``): the device writes its adapted rows, so ``model._env_params_host`` is stale for them;
    ``set_model_params`` refuses an adapted name and refreshes those rows of the mirror from the device before it rewrites
    any other."""
    owns_masses = False        # utils/mpc_adapt_inertia.py AdaptiveInertiaController: the mass dimensions of ``adapt.masses``

    def __init__(self, plant_task, model_task, samples, adapt, horizon=MPC_DEFAULTS["horizon"], lam=MPC_DEFAULTS["lambda"],
                 sigma=MPC_DEFAULTS["sigma"], seed=MPC_DEFAULTS["seed"], graph=True, graph_cycles=1, keep_weights=False,
                 forget_on_reset=False):
        import torch
        from . import env_params
        if hasattr(adapt, "keys") and "masses" in adapt.keys() and not self.owns_masses:
            raise ConfigError("mpc adapt: masses is mpc_adapt_inertia.AdaptiveInertiaController's key; this controller has no mass "
                              "dimensions")
        super().__init__(plant_task, model_task, samples, horizon, lam, sigma, seed, graph=graph, graph_steps=1,
                         keep_weights=keep_weights)
        if model_task.env_params is None:
            raise ConfigError("mpc adapt: the model task has no per-env parameter table bound (task.env.ENV_PARAMS is empty): "
                              "the table is what is adapted")
        self.base_row = env_params.config_row(self.lib, model_task._vcfg)
        self.acfg, self.names = adapt_config(adapt, self.M, self.K, self.base_row, seed, forget_on_reset)
        self.dims = dims_of(self.acfg)
        self.W, self.E, self.D = int(self.acfg.window), int(self.acfg.every), int(self.acfg.num_dims)
        M, N, W, D, dev = self.M, self.M * self.K, self.W, self.D, self.device
        f32, f64, i64, u8 = torch.float32, torch.float64, torch.int64, torch.uint8
        prior_mean, prior_std = self._prior(model_task.env_params.cpu().numpy())
        self.prior_mean = torch.as_tensor(prior_mean, device=dev)
        self.prior_std = torch.as_tensor(prior_std, device=dev)
        self.mean, self.std = self.prior_mean.clone(), self.prior_std.clone()
        self.passes = torch.zeros(M, dtype=i64, device=dev)
        self.anchor_state = torch.zeros((abi.VF_COUNT, M), dtype=f32, device=dev)
        self.anchor_history = torch.zeros((M, abi.MAX_DELAY, 2), dtype=f32, device=dev)
        self.anchor_progress = torch.zeros(M, dtype=i64, device=dev)
        self.anchor_count = torch.zeros(1, dtype=i64, device=dev)
        self.trace_actions = torch.zeros((M, W, 2), dtype=f32, device=dev)
        self.trace_rows = torch.zeros((M, W, abi.MPC_ADAPT_FIELDS), dtype=f32, device=dev)
        self.trace_len = torch.zeros(M, dtype=torch.int32, device=dev)
        self.trace_open = torch.zeros(M, dtype=u8, device=dev)
        self.episode_ended = torch.zeros(M, dtype=u8, device=dev)
        self.err = torch.zeros(N, dtype=f64, device=dev)
        self.adapt_alive = torch.ones(N, dtype=u8, device=dev)
        self.adapt_window = torch.zeros(1, dtype=i64, device=dev)
        self.returns = torch.zeros(M, dtype=f64, device=dev)          # the summed plant reward, by the trace node
        self.adapt_weights = torch.zeros(N, dtype=f64, device=dev) if keep_weights else None
        self.phase = 0
        self.graph_cycles = max(1, int(graph_cycles))
        self.unit_steps = self.E * self.graph_cycles
        self.launches.update({"anchor": 0, "trace": 0, "pin": 0, "adapt_step": 0, "score": 0, "estimate": 0})
        self._write_plan()

    def _prior(self, table):
        """The prior of every plant: the model's current value (sample 0 of the plant; an FPAM vector's factor from its first
        constant that is not zero) clamped into the range, and ``spread * (hi - lo)``."""
        mean = np.zeros((self.M, self.D), dtype=np.float64)
        std = np.zeros((self.M, self.D), dtype=np.float64)
        col = table[:, ::self.K].astype(np.float64)
        for d, (first, count, lo, hi, _floor) in enumerate(self.dims):
            v = col[first]
            if count > 1:
                nz = [r for r in range(first, first + count) if self.base_row[r] != 0]
                v = col[nz[0]] / np.float64(self.base_row[nz[0]]) if nz else np.ones(self.M)
            mean[:, d] = np.minimum(np.maximum(v, lo), hi)
            std[:, d] = self.acfg.spread * (hi - lo)
        return mean, std

    def _write_plan(self):
        """The planning value of the current belief into the model's table, from the host (at construction only: a prior
        outside its range was clamped)."""
        import torch
        plan = np.repeat(self.mean.cpu().numpy(), self.K, axis=0)
        for r, v in table_rows(plan, self.dims, self.base_row).items():
            self.model.env_params[r].copy_(torch.from_numpy(np.ascontiguousarray(v)))

    def tensors(self):
        extra = [self.mean, self.std, self.passes, self.anchor_state, self.anchor_history, self.anchor_progress,
                 self.anchor_count, self.trace_actions, self.trace_rows, self.trace_len, self.trace_open, self.episode_ended,
                 self.err, self.adapt_alive, self.adapt_window, self.returns, self.model.env_params]
        return super().tensors() + extra + ([self.adapt_weights] if self.adapt_weights is not None else [])

    # -- the five launches -----------------------------------------------------------------------------------------------
    def anchor(self):
        from .. import native
        p = self.plant
        native.check(self.lib.vine_mpc_adapt_anchor(
            p._handle, self.acfg, p.progress_buf.data_ptr(), p.reset_buf.data_ptr(), self.history.data_ptr(),
            self.anchor_state.data_ptr(), self.anchor_history.data_ptr(), self.anchor_progress.data_ptr(),
            self.anchor_count.data_ptr(), self.trace_len.data_ptr(), self.trace_open.data_ptr(),
            self.episode_ended.data_ptr(), self._stream()), self.lib)
        self.launches["anchor"] += 1

    def trace(self):
        from .. import native
        p = self.plant
        native.check(self.lib.vine_mpc_adapt_trace(
            p._handle, self.acfg, self.plant_actions.data_ptr(), p.reset_buf.data_ptr(), p.rew_buf.data_ptr(),
            self.anchor_count.data_ptr(), self.trace_actions.data_ptr(), self.trace_rows.data_ptr(), self.trace_len.data_ptr(),
            self.trace_open.data_ptr(), self.episode_ended.data_ptr(), self.returns.data_ptr(), self._stream()), self.lib)
        self.launches["trace"] += 1

    def pin(self):
        from .. import native
        m = self.model
        native.check(self.lib.vine_mpc_adapt_pin(
            m._handle, self.acfg, self.mean.data_ptr(), self.std.data_ptr(), self.passes.data_ptr(),
            self.anchor_state.data_ptr(), self.anchor_history.data_ptr(), self.anchor_progress.data_ptr(),
            self.trace_actions.data_ptr(), self.actions.data_ptr(), m.rew_buf.data_ptr(), m.reset_buf.data_ptr(),
            m.progress_buf.data_ptr(), self.err.data_ptr(), self.adapt_alive.data_ptr(), self.adapt_window.data_ptr(),
            self._stream()), self.lib)
        self.launches["pin"] += 1

    def score(self):
        from .. import native
        m = self.model
        native.check(self.lib.vine_mpc_adapt_scheduled(
            m._handle, self.acfg, self.trace_actions.data_ptr(), self.trace_rows.data_ptr(), self.trace_len.data_ptr(),
            self.adapt_window.data_ptr(), self.actions.data_ptr(), m.reset_buf.data_ptr(), self.err.data_ptr(),
            self.adapt_alive.data_ptr(), self._stream()), self.lib)
        self.launches["score"] += 1

    def estimate(self):
        from .. import native
        native.check(self.lib.vine_mpc_adapt_estimate(
            self.model._handle, self.acfg, self.err.data_ptr(), self.trace_len.data_ptr(), self.episode_ended.data_ptr(),
            self.mean.data_ptr(), self.std.data_ptr(), self.prior_mean.data_ptr(), self.prior_std.data_ptr(),
            self.passes.data_ptr(), self.adapt_weights.data_ptr() if self.adapt_weights is not None else None,
            self._stream()), self.lib)
        self.launches["estimate"] += 1

    def adapt_pass(self):
        """The second half of a cycle: the candidates replay the traced steps and the belief moves."""
        self.pin()
        for _ in range(self.W):
            self.model.step_into(self.actions, self.model_obs)
            self.launches["adapt_step"] += 1
            self.score()
        self.estimate()

    def cycle(self):
        """One whole cycle, eagerly (or into a capture)."""
        self.anchor()
        for _ in range(self.E):
            self.control_step()
            self.trace()
        self.adapt_pass()

    # -- many of them: Controller.run with whole cycles as the unit ---------------------------------------------------------
    def at_boundary(self):
        return self.phase == 0

    def unit(self):
        for _ in range(self.graph_cycles):
            self.cycle()

    def eager_step(self):
        """One control step of the running cycle, the phase kept on the host."""
        if self.phase == 0:
            self.anchor()
        self.control_step()
        self.trace()
        self.phase += 1
        if self.phase == self.E:
            self.adapt_pass()
            self.phase = 0

    # -- from outside the step -------------------------------------------------------------------------------------------
    def adapted_rows(self):
        return [r for first, count, _lo, _hi, _floor in self.dims for r in range(first, first + count)]

    def set_model_params(self, values):
        """``Controller.set_model_params`` for the rows the belief does not own: an adapted name (or a single row of an
        adapted FPAM vector) is refused by name, and the mirror's adapted rows are refreshed from the device first."""
        for name in values:
            rows = []
            if name in abi.ENV_PARAM_ROWS:
                first, count = abi.ENV_PARAM_ROWS[name]
                rows = list(range(first, first + count))
            elif name in self.model.env_param_names:
                rows = [self.model.env_param_names.index(name)]
            if set(rows) & set(self.adapted_rows()):
                raise ValueError("set_model_params: %s is adapted on the device (adapt.params: %s); the belief owns its rows"
                                 % (name, ", ".join(self.names)))
        rows = self.adapted_rows()
        self.model._env_params_host[rows] = self.model.env_params[rows].cpu().numpy()
        super().set_model_params(values)

    def belief(self):
        """``(mean, std)`` float64 [M, D] as of now (synchronises)."""
        return self.mean.cpu().numpy(), self.std.cpu().numpy()

    def truth(self):
        """float64 [M, D]: the PLANT's own value of every adapted dimension, where the plant task carries a parameter table
        (else ``None``).  The plant's configuration is taken to have the model's FPAM constants."""
        if self.plant.env_params is None:
            return None
        table = self.plant.env_params.cpu().numpy().astype(np.float64)
        out = np.zeros((self.M, self.D), dtype=np.float64)
        for d, (first, count, _lo, _hi, _floor) in enumerate(self.dims):
            v = table[first]
            if count > 1:
                nz = [r for r in range(first, first + count) if self.base_row[r] != 0]
                v = table[nz[0]] / np.float64(self.base_row[nz[0]]) if nz else np.ones(self.M)
            out[:, d] = v
        return out


# ------------------------------------------------------------------------------------------------------------------ a run
class Play(PlayVariant):
    """``adapt=`` of ``mpc.play``."""
    single_run = True          # whole cycles replay from one graph: the trace node sums the reward into ``ctl.returns``

    def masses(self):
        """utils/mpc_adapt_inertia.py where the spec has ``masses``, else ``None``: without the key
        nothing of that module is imported."""
        if not (hasattr(self.spec, "keys") and "masses" in self.spec.keys()):
            return None
        from . import mpc_adapt_inertia
        return mpc_adapt_inertia

    def check(self, run):
        if self.masses() is not None:
            self.masses().check_masses(self.spec)

    def bind(self, run):
        if not run.mcfg["env"].get("ENV_PARAMS"):
            run.mcfg["env"]["ENV_PARAMS"] = {"FPAM_K": 1.0}      # binds a table of the configuration's own row: what is adapted
        if self.masses() is not None:
            self.masses().bind(run)                              # ... and an inertia table of it, likewise

    def controller(self, run):
        from . import env_params
        if self.masses() is not None:
            return self.masses().controller(run, self.spec, env_params.per_episode(run.cfg["env"]))
        if run.draws:              # the one exception: the prior is the model's value when the controller is made
            run.model.set_env_params({k: np.repeat(v, int(run.samples)) for k, v in run.draws.items()})
            run.draws = None
        return AdaptiveController(run.plant, run.model, run.samples, self.spec, *run.planner, graph=run.graph,
                                  forget_on_reset=env_params.per_episode(run.cfg["env"]))

    def banner(self, run):
        ctl = run.ctl
        names = list(ctl.names) + list(getattr(ctl, "mass_names", ()))
        print("mpc: adapting %s every %d control steps over a window of %d" % (", ".join(names), ctl.E, ctl.W), flush=True)

    def epilogue(self, run, out):
        ctl = run.ctl
        mean, std = ctl.belief()
        prior, truth = ctl.prior_mean.cpu().numpy(), ctl.truth()
        out["adapt"] = {"names": list(ctl.names), "mean": mean, "std": std, "prior_mean": prior, "truth": truth,
                        "passes": ctl.passes.cpu().numpy(), "prior_error": {}, "final_error": {}}
        for d, name in enumerate(ctl.names):
            if truth is None:
                print("  adapt %s: final mean %s" % (name, np.array2string(mean[:, d], precision=4)), flush=True)
                continue
            out["adapt"]["prior_error"][name] = float(np.abs(prior[:, d] - truth[:, d]).mean())
            out["adapt"]["final_error"][name] = float(np.abs(mean[:, d] - truth[:, d]).mean())
            print("  adapt %s: mean |prior - truth| %.4g, mean |belief - truth| %.4g" % (
                name, out["adapt"]["prior_error"][name], out["adapt"]["final_error"][name]), flush=True)
        if self.masses() is not None:
            self.masses().epilogue(ctl, out)
