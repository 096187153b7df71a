"""MPC_NOISE on the host side: the predictive controller's samples are drawn with perturbations correlated over the horizon
and, on request, with an amplitude per plant that follows the spread of the samples the weights preferred.  The semantics are
stated once, in include/vine_mpc_noise.h.  What is left for the host: the ``noise=`` mapping (``noise_config``), the checked
``abi.VineMpcNoiseConfig`` (``noise_struct``), the numpy statement of the three launches every GPU test compares against
(``colored_deviate``, ``colored_actions``, ``noise_replay``), and the controller that owns the table and the amplitudes and
enqueues the launches (``NoiseController``).

``noise=`` maps

  ``BETA``    the correlation of successive horizon steps, in [0, 1): one number for both action components, or two.  0 is
              the white noise of include/vine_mpc.h, word for word.
  ``ADAPT``   optional: a mapping of ``RATE`` (in (0, 1], default 0.2), ``SIGMA_MIN`` (default 0.05) and ``SIGMA_MAX``
              (default 1.0), each one number or two; the planner's ``sigma`` must lie between the two bounds."""
import numpy as np

from .. import abi
from . import env_sensor, mpc
from .config import ConfigError

_KEY = "noise"
ADAPT_DEFAULTS = {"RATE": 0.2, "SIGMA_MIN": 0.05, "SIGMA_MAX": 1.0}
OTHERS = ("track", "observe", "filter", "policy", "adapt")      # the variants ``noise=`` is refused together with


# ---- configuration
def _real(key, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ConfigError("%s.%s: %r is not a finite number" % (_KEY, key, v))
    return float(v)


def _pair(key, v):
    pair = list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v, v]
    if len(pair) != 2:
        raise ConfigError("%s.%s is one number or two, not %r" % (_KEY, key, v))
    return [_real(key, x) for x in pair]


def noise_config(spec):
    """The checked ``noise=`` mapping: ``{"BETA": [b0, b1], "ADAPT": None | {"RATE": r, "SIGMA_MIN": [..], "SIGMA_MAX": [..]}}``.
    ``ConfigError``, naming the key, for anything else."""
    if not hasattr(spec, "keys"):
        raise ConfigError("%s={BETA: value, ...} must be a mapping, not %r" % (_KEY, spec))
    unknown = sorted(str(k) for k in set(spec.keys()) - {"BETA", "ADAPT"})
    if unknown:
        raise ConfigError("%s: unknown key(s) %s" % (_KEY, ", ".join(unknown)))
    if "BETA" not in spec:
        raise ConfigError("%s.BETA is missing: the correlation of successive horizon steps, in [0, 1)" % _KEY)
    beta = _pair("BETA", spec["BETA"])
    for b in beta:
        if not 0.0 <= b < 1.0 or not float(np.float32(b)) < 1.0:
            raise ConfigError("%s.BETA must lie in [0, 1), not %g" % (_KEY, b))
    adapt = spec.get("ADAPT")
    if adapt is not None:
        if not hasattr(adapt, "keys"):
            raise ConfigError("%s.ADAPT={RATE: value, ...} must be a mapping, not %r" % (_KEY, adapt))
        unknown = sorted(str(k) for k in set(adapt.keys()) - set(ADAPT_DEFAULTS))
        if unknown:
            raise ConfigError("%s.ADAPT: unknown key(s) %s" % (_KEY, ", ".join(unknown)))
        full = dict(ADAPT_DEFAULTS, **{str(k): adapt[k] for k in adapt.keys()})
        rate = _real("ADAPT.RATE", full["RATE"])
        if not 0.0 < rate <= 1.0:
            raise ConfigError("%s.ADAPT.RATE must lie in (0, 1], not %g" % (_KEY, rate))
        lo, hi = _pair("ADAPT.SIGMA_MIN", full["SIGMA_MIN"]), _pair("ADAPT.SIGMA_MAX", full["SIGMA_MAX"])
        big = float(np.finfo(np.float32).max)
        for a in range(2):
            if lo[a] < 0.0:
                raise ConfigError("%s.ADAPT.SIGMA_MIN must not be negative, not %g" % (_KEY, lo[a]))
            if hi[a] > big:
                raise ConfigError("%s.ADAPT.SIGMA_MAX must fit a float32, not %g" % (_KEY, hi[a]))
            if lo[a] > hi[a]:
                raise ConfigError("%s.ADAPT.SIGMA_MIN %g lies above SIGMA_MAX %g" % (_KEY, lo[a], hi[a]))
        adapt = {"RATE": rate, "SIGMA_MIN": lo, "SIGMA_MAX": hi}
    return {"BETA": beta, "ADAPT": adapt}


def noise_struct(spec, mcfg):
    """The ``abi.VineMpcNoiseConfig`` of a ``noise=`` mapping beside the controller's ``abi.VineMpcConfig``: ``ConfigError`` for
    a ``sigma`` outside ``ADAPT``'s bounds, which the library would refuse too."""
    spec = noise_config(spec)
    c = abi.VineMpcNoiseConfig()
    c.abi_version = abi.MPC_NOISE_ABI_VERSION
    c.beta[0], c.beta[1] = spec["BETA"]
    c.adapt, c.rate = 0, ADAPT_DEFAULTS["RATE"]
    c.sigma_min[0] = c.sigma_min[1] = 0.0
    c.sigma_max[0] = c.sigma_max[1] = float(np.finfo(np.float32).max)
    if spec["ADAPT"] is not None:
        ad = spec["ADAPT"]
        c.adapt, c.rate = 1, ad["RATE"]
        for a in range(2):
            c.sigma_min[a], c.sigma_max[a] = ad["SIGMA_MIN"][a], ad["SIGMA_MAX"][a]
            if not c.sigma_min[a] <= mcfg.sigma[a] <= c.sigma_max[a]:
                raise ConfigError("%s.ADAPT: sigma %g lies outside SIGMA_MIN .. SIGMA_MAX = %g .. %g" % (
                    _KEY, mcfg.sigma[a], c.sigma_min[a], c.sigma_max[a]))
    return c


# ---- the launches, in numpy
def gains(beta):
    """float32 ``(b [2], g [2])`` of include/vine_mpc_noise.h: ``g = float32(sqrt(1 - (double)b^2))``."""
    b = np.broadcast_to(np.asarray(beta, dtype=np.float32), (2,)).copy()
    g = np.sqrt(1.0 - b.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
    return b, g


def colored_deviate(seed, num_plants, samples, tick, horizon, beta):
    """float32 [M, K, H, 2]: ``eps`` of ``vine_mpc_noise_draw`` -- ``mpc.noise_deviate`` passed through the first-order recursion
    ``eps[k] = b * eps[k - 1] + g * z[k]``, two float32 multiplies and one float32 add.  The device keeps it as [H, M * K, 2]:
    ``table_layout``."""
    z = mpc.noise_deviate(seed, num_plants, samples, tick, horizon)
    b, g = gains(beta)
    eps = np.empty_like(z)
    eps[:, :, 0] = z[:, :, 0]
    for k in range(1, z.shape[2]):
        eps[:, :, k] = (b * eps[:, :, k - 1]).astype(np.float32) + (g * z[:, :, k]).astype(np.float32)
    return eps


def table_layout(eps):
    """[M, K, H, 2] as the device's table [H, M * K, 2]."""
    M, K, H, _ = eps.shape
    return np.ascontiguousarray(eps.reshape(M * K, H, 2).transpose(1, 0, 2))


def colored_actions(nominal, sigma_p, eps, clip):
    """float32 [M, K, H, 2]: ``u'`` of include/vine_mpc_noise.h around ``nominal`` [M, H, 2] with the amplitudes ``sigma_p``
    [M, 2] (or [2]) and the perturbations ``eps`` [M, K, H, 2] -- one float32 multiply, one float32 add, the clamp."""
    nominal = np.asarray(nominal, dtype=np.float32)
    M = nominal.shape[0]
    sigma_p = np.broadcast_to(np.asarray(sigma_p, dtype=np.float32), (M, 2))
    c = (sigma_p.astype(np.float64) * env_sensor.NOISE_SCALE).astype(np.float32)
    x = nominal[:, None] + (np.asarray(eps, dtype=np.float32) * c[:, None, None, :]).astype(np.float32)
    clip = np.float32(clip)
    return np.minimum(np.maximum(x, -clip), clip)


def noise_replay(nominal, cost, sigma, lam, seed, tick, clip, beta, sigma_p=None, adapt=None, plant_reset=None, history=None,
                 eps=None):
    """``vine_mpc_noise_update`` on the host: ``mpc.mpc_replay`` with ``u'`` in the place of ``u``, and ``sigma``.  ``sigma``:
    the configuration's (one number or two); ``sigma_p`` [M, 2]: the amplitudes in force (default ``sigma``); ``adapt``:
    ``None`` or ``{"RATE", "SIGMA_MIN", "SIGMA_MAX"}`` as ``noise_config`` returns it; ``eps`` [M, K, H, 2]: the table where it
    is not ``colored_deviate``'s (hand-made cases).  Returns ``mpc_replay``'s dict and ``sigma`` float32 [M, 2] (the new
    amplitudes), ``v`` float64 [M, 2] (the weighted mean square; NaN where no cost is finite) and ``eps``."""
    nominal = np.asarray(nominal, dtype=np.float32)
    M, H = nominal.shape[0], nominal.shape[1]
    cost = np.asarray(cost, dtype=np.float64).reshape(M, -1)
    K = cost.shape[1]
    tick = np.broadcast_to(np.asarray(tick, dtype=np.int64), (M,))
    sigma0 = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (2,))
    sigma_p = (np.broadcast_to(sigma0, (M, 2)) if sigma_p is None else np.asarray(sigma_p, dtype=np.float32).reshape(M, 2)).copy()
    if eps is None:
        eps = colored_deviate(seed, M, K, tick, H, beta)
    u = colored_actions(nominal, sigma_p, eps, clip)
    r = mpc.mpc_replay(nominal, cost, sigma, lam, seed, tick, clip, plant_reset, history, u=u)
    w = r["weights"]
    new_sigma, v = sigma_p.copy(), np.full((M, 2), np.nan)
    finite = w.sum(axis=1) > 0.0
    consumed = np.zeros(M, dtype=bool) if plant_reset is None else np.asarray(plant_reset).reshape(M) != 0
    d = u.astype(np.float64) - nominal.astype(np.float64)[:, None]
    for p in np.flatnonzero(finite):
        v[p] = (w[p][:, None, None] * (d[p] * d[p])).sum(axis=(0, 1)) / (w[p].sum() * H)
    if adapt is not None:
        rate = np.float64(adapt["RATE"])
        lo = np.broadcast_to(np.asarray(adapt["SIGMA_MIN"], dtype=np.float32), (2,)).astype(np.float64)
        hi = np.broadcast_to(np.asarray(adapt["SIGMA_MAX"], dtype=np.float32), (2,)).astype(np.float64)
        for p in np.flatnonzero(finite & ~consumed):
            s = sigma_p[p].astype(np.float64)
            new_sigma[p] = np.minimum(np.maximum(np.sqrt((1.0 - rate) * s * s + rate * v[p]), lo), hi).astype(np.float32)
        new_sigma[consumed] = sigma0
    r.update(sigma=new_sigma, v=v, eps=eps)
    return r


# ---- the device
class NoiseController(mpc.Controller):
    """``mpc.Controller`` whose samples are drawn from the table ``eps`` [H, M * K, 2] with the amplitudes ``sigma_p`` [M, 2].

    ``control_step()`` = ``draw()``, ``fork()``, ``noise_node()``, H x (``model.step_into`` + ``node()`` + ``noise_node()``),
    the update of include/vine_mpc_noise.h, the plant step: still one linear chain in a captured graph.  ``launches`` gains
    ``"draw"`` and ``"noise"``."""

    def __init__(self, plant_task, model_task, samples, noise, horizon=mpc.DEFAULTS["horizon"], lam=mpc.DEFAULTS["lambda"],
                 sigma=mpc.DEFAULTS["sigma"], seed=mpc.DEFAULTS["seed"], graph=True, graph_steps=1, keep_weights=False):
        import torch
        self.noise = noise_config(noise)
        super().__init__(plant_task, model_task, samples, horizon, lam, sigma, seed, graph=graph, graph_steps=graph_steps,
                         keep_weights=keep_weights)
        self.ncfg = noise_struct(self.noise, self.mcfg)
        self.eps = torch.zeros((self.H, self.M * self.K, 2), dtype=torch.float32, device=self.device)
        self.sigma0 = torch.tensor([self.mcfg.sigma[0], self.mcfg.sigma[1]], dtype=torch.float32, device=self.device)
        self.sigma_p = self.sigma0.repeat(self.M, 1).contiguous()
        self.launches.update({"draw": 0, "noise": 0})

    def tensors(self):
        return super().tensors() + [self.eps, self.sigma_p]

    def draw(self):
        from .. import native
        native.check(self.lib.vine_mpc_noise_draw(self.model._handle, self.mcfg, self.ncfg, self.tick.data_ptr(),
                                                  self.eps.data_ptr(), self._stream()), self.lib)
        self.launches["draw"] += 1

    def noise_node(self):
        from .. import native
        native.check(self.lib.vine_mpc_noise_scheduled(
            self.model._handle, self.mcfg, self.ncfg, self.nominal.data_ptr(), self.window.data_ptr(), self.eps.data_ptr(),
            self.sigma_p.data_ptr(), self.actions.data_ptr(), self._stream()), self.lib)
        self.launches["noise"] += 1

    def update(self):
        from .. import native
        native.check(self.lib.vine_mpc_noise_update(
            self.model._handle, self.mcfg, self.ncfg, self.cost.data_ptr(), self.plant.reset_buf.data_ptr(), self.eps.data_ptr(),
            self.nominal.data_ptr(), self.history.data_ptr(), self.tick.data_ptr(), self.plant_actions.data_ptr(),
            self.sigma_p.data_ptr(), self.weights.data_ptr() if self.weights is not None else None, self._stream()), self.lib)
        self.launches["update"] += 1

    def after_fork(self):
        self.noise_node()

    def model_step(self):
        """One model step, the scoring node behind it and the table's next action behind that."""
        super().model_step()
        self.noise_node()

    def control_step(self):
        self.draw()
        super().control_step()

    def clear_rows(self, ids):
        super().clear_rows(ids)
        self.sigma_p[ids] = self.sigma0


# ---- a run
class Play(mpc.PlayVariant):
    """``noise=`` of ``mpc.play``."""

    def check(self, run):
        self.spec = noise_config(self.spec)
        for key in OTHERS:
            if run.args.get(key) is not None:
                raise ConfigError("mpc: noise= together with %s= is refused: that controller computes its own perturbations and "
                                  "was not built for a table" % key)
        noise_struct(self.spec, mpc.mpc_config(run.M, run.samples, *run.planner))

    def controller(self, run):
        return NoiseController(run.plant, run.model, run.samples, self.spec, *run.planner, graph=run.graph)

    def banner(self, run):
        ad = self.spec["ADAPT"]
        print("mpc: the samples' perturbations are correlated over the horizon, BETA %s; %s" % (
            self.spec["BETA"], "each plant's sigma fixed" if ad is None else
            "each plant's sigma adapts at RATE %g inside %s .. %s" % (ad["RATE"], ad["SIGMA_MIN"], ad["SIGMA_MAX"])), flush=True)

    def result(self, run, out):
        s = run.ctl.sigma_p.cpu().numpy().astype(np.float64)
        out["noise"] = {"BETA": list(self.spec["BETA"]), "ADAPT": self.spec["ADAPT"], "sigma_mean": s.mean(axis=0).tolist(),
                        "sigma_min": s.min(axis=0).tolist(), "sigma_max": s.max(axis=0).tolist()}
        print("mpc: final sigma per plant [rail, fpam]: mean %s, min %s, max %s" % (
            np.array2string(s.mean(axis=0), precision=4), np.array2string(s.min(axis=0), precision=4),
            np.array2string(s.max(axis=0), precision=4)), flush=True)
