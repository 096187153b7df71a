"""MPC_ADAPT masses on the host side: the belief of utils/mpc_adapt.py carries up to three mass dimensions.

The semantics are stated once, in include/vine_mpc_adapt_inertia.h.  ``adapt={params: {...}, masses: {CART_MASS: [lo, hi],
LINK_MASS: [lo, hi], TIP_LINK_MASS: [lo, hi]}}``: beside the rows of the parameter table the K candidates of a plant differ in
the cart's mass (kg), in a factor on the model configuration's five link masses and inertias, and in a further factor on the
tip link's -- the semantics of ``env_params.set_inertia_rows``.  ``vine_mpc_adapt_inertia_pin`` writes each candidate's column
of the model's INERTIA table, derived rows included, directly behind the base pin; ``vine_mpc_adapt_inertia_estimate`` moves
the mass belief with the base estimate's weights, in front of it, and writes the planning column.  What is left for the host:
the configuration (``masses_config``), the numpy statements every GPU test compares against (``mass_candidates``,
``inertia_rows``, ``mass_estimate``) and the buffers (``AdaptiveInertiaController``).  Nothing here is imported unless
``masses`` is given."""
import logging

import numpy as np

from .. import abi
from . import env_params, mpc_adapt
from .config import ConfigError
from .mpc import check_real

NAMES = abi.ENV_INERTIA_NAMES                      # CART_MASS, LINK_MASS, TIP_LINK_MASS: the header's names 0, 1, 2
PLACEHOLDER = "DAMPING"                            # the one table dimension the base launches get where ``params`` is absent


# ---------------------------------------------------------------------------------------------------------- configuration
def check_masses(spec):
    """``[(name, lo, hi), ..]`` of ``spec["masses"]``, in its order; what include/vine_mpc_adapt_inertia.h refuses of a range
    is refused here with a ``ConfigError`` naming the key."""
    masses = spec.get("masses")
    if not hasattr(masses, "keys") or len(masses) == 0:
        raise ConfigError("mpc adapt: masses must be a non-empty mapping {NAME: [lo, hi]} of %s, not %r" % (
            ", ".join(NAMES), masses))
    out = []
    for name in masses.keys():
        if name not in NAMES:
            raise ConfigError("mpc adapt: masses: unknown name %r (known: %s)" % (name, ", ".join(NAMES)))
        entry = masses[name]
        if not isinstance(entry, (list, tuple)) or len(entry) != 2:
            raise ConfigError("mpc adapt: masses.%s must be a range [lo, hi], not %r" % (name, entry))
        lo, hi = check_real("adapt.masses." + name, entry[0]), check_real("adapt.masses." + name, entry[1])
        if lo > hi:
            raise ConfigError("mpc adapt: masses.%s: lo > hi in [%g, %g]" % (name, lo, hi))
        if not lo > 0.0:
            raise ConfigError("mpc adapt: masses.%s: lo must be positive (a candidate mass must be), not %g" % (name, lo))
        if hi > float(np.finfo(np.float32).max) or np.float32(lo) == 0.0:
            raise ConfigError("mpc adapt: masses.%s: [%g, %g] does not fit a float32" % (name, lo, hi))
        out.append((name, lo, hi))
    return out


def masses_config(spec, base_inertia, link_length, link_com, gravity):
    """``(abi.VineMpcAdaptInertiaConfig, names)`` of the ``masses`` of an ``adapt`` spec.  ``base_inertia``: the model
    configuration's ``env_params.inertia_config_row`` (its primaries are taken); ``link_length``, ``link_com``, ``gravity``:
    that configuration's.  ``std_floor`` of a dimension is ``floor * (hi - lo)`` with the spec's ``floor``, as for ``params``."""
    if not hasattr(spec, "keys"):
        raise ConfigError("mpc adapt: adapt={params: {NAME: [lo, hi]}, ...} must be a mapping, not %r" % (spec,))
    ranges = check_masses(spec)
    floor = check_real("adapt.floor", spec.get("floor", mpc_adapt.DEFAULTS["floor"]))
    if floor < 0.0:
        raise ConfigError("mpc adapt: spread and floor must not be negative, not floor %g" % floor)
    c = abi.VineMpcAdaptInertiaConfig()
    c.abi_version = abi.MPC_ADAPT_INERTIA_ABI_VERSION
    c.num_mass_dims = len(ranges)
    for i, (name, lo, hi) in enumerate(ranges):
        c.dims[i].name, c.dims[i].lo, c.dims[i].hi, c.dims[i].std_floor = NAMES.index(name), lo, hi, floor * (hi - lo)
    base = np.asarray(base_inertia, dtype=np.float32)
    for r in range(abi.VI_PRIMARY_COUNT):
        c.base_inertia[r] = float(base[r])
    c.link_length, c.link_com, c.gravity = float(link_length), float(link_com), float(gravity)
    return c, [name for name, _lo, _hi in ranges]


def mass_dims_of(icfg):
    """``[(name index, lo, hi, std_floor), ..]`` of a configuration."""
    return [(int(m.name), m.lo, m.hi, m.std_floor) for m in list(icfg.dims)[:icfg.num_mass_dims]]


def estimate_dims(mdims):
    """The mass dimensions in the form ``mpc_adapt.estimate`` reads its ``dims`` in (it reads lo, hi and the floor only)."""
    return [(None, 1, lo, hi, floor) for _name, lo, hi, floor in mdims]


# ---------------------------------------------------------------------------------------------------- the launches, in numpy
def mass_deviate(seed, num_plants, samples, passes, num_mass_dims):
    """float32 [M, K, Dm]: z of the mass dimensions -- ``mpc_adapt.deviate`` with the counter's last word
    ``abi.MPC_ADAPT_MAX_DIMS + i``; candidate 0 has 0."""
    z = mpc_adapt.deviate(seed, num_plants, samples, passes, abi.MPC_ADAPT_MAX_DIMS + int(num_mass_dims))
    return np.ascontiguousarray(z[:, :, abi.MPC_ADAPT_MAX_DIMS:])


def mass_candidates(mean, std, mdims, seed, samples, passes):
    """float64 [M, K, Dm]: theta of every candidate -- one float64 multiply, one add, the clamp to the dimension's range."""
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    M, Dm = mean.shape
    z = mass_deviate(seed, M, samples, passes, Dm).astype(np.float64)
    x = mean[:, None, :] + z * std[:, None, :]
    lo = np.array([d[1] for d in mdims], dtype=np.float64)
    hi = np.array([d[2] for d in mdims], dtype=np.float64)
    return np.minimum(np.maximum(x, lo), hi)


def inertia_rows(theta, mdims, base_inertia, derive):
    """float32 [VI_COUNT, n]: the inertia columns of ``theta`` [n, Dm] (or [M, K, Dm], flattened to n = M * K) -- the primary
    rows through ``env_params.set_inertia_rows`` on the configuration's row ``base_inertia`` (an absent name keeps the
    configuration's), the derived rows through ``derive`` (``env_params.derive_inertia`` bound to a library and a
    configuration): the statements the plants' own tables are made with, not a second formula."""
    theta = np.asarray(theta, dtype=np.float64)
    theta = theta.reshape(-1, theta.shape[-1])
    base = np.asarray(base_inertia, dtype=np.float32)
    table = np.repeat(base[:, None], theta.shape[0], axis=1)
    env_params.set_inertia_rows(table, base, {NAMES[name]: theta[:, i] for i, (name, _lo, _hi, _floor) in enumerate(mdims)})
    return derive(table)


def mass_estimate(err, theta, mean, std, prior_mean, prior_std, trace_len, episode_ended, mdims, min_steps, temperature, rate,
                  forget_on_reset=False):
    """The estimate of the mass dimensions on the host: ``mpc_adapt.estimate``'s body on the mass belief and its candidates
    (``theta`` [M, K, Dm]).  The same dict; ``plan`` [M, Dm] is the new mean clamped to the ranges."""
    return mpc_adapt.estimate(err, theta, mean, std, prior_mean, prior_std, trace_len, episode_ended, estimate_dims(mdims),
                              min_steps, temperature, rate, forget_on_reset)


def mass_values(table, mdims, base_inertia):
    """float64 [n, Dm]: the value of every mass dimension that the inertia columns ``table`` [VI_COUNT, n] hold -- the cart's
    mass from its row, ``LINK_MASS`` as m_0 / base m_0, ``TIP_LINK_MASS`` as (m_4 / base m_4) / (m_0 / base m_0)."""
    t = np.asarray(table, dtype=np.float64)
    base = np.asarray(base_inertia, dtype=np.float64)
    link = t[abi.VI_LINK_MASS0] / base[abi.VI_LINK_MASS0]
    last = abi.VI_LINK_MASS0 + abi.NUM_LINKS - 1
    by_name = (t[abi.VI_CART_MASS], link, (t[last] / base[last]) / link)
    return np.stack([by_name[name] for name, _lo, _hi, _floor in mdims], axis=1)


# ------------------------------------------------------------------------------------------------------------ the device
def base_spec(spec, model_table):
    """``(spec for mpc_adapt.adapt_config, placeholder)``: the spec without ``masses``; where it has no ``params``, one
    placeholder dimension -- ``PLACEHOLDER`` over the [min, max] of the model's own row -- since the five base launches refuse
    ``num_dims < 1``."""
    out = {k: spec[k] for k in spec.keys() if k != "masses"}
    if "params" in spec.keys():
        return out, False
    row = np.asarray(model_table, dtype=np.float64)[abi.ENV_PARAM_ROWS[PLACEHOLDER][0]]
    out["params"] = {PLACEHOLDER: [float(row.min()), float(row.max())]}
    return out, True


class AdaptiveInertiaController(mpc_adapt.AdaptiveController):
    """An ``AdaptiveController`` whose belief has mass dimensions too: the four buffers of include/vine_mpc_adapt_inertia.h
    and its two launches, ``inertia_pin`` directly behind ``pin`` and ``inertia_estimate`` in front of ``estimate``.  The model
    task must have an inertia table bound beside its parameter table; the device writes ALL of its rows (an absent name is
    held at the configuration's value), so ``model._env_inertia_host`` is stale: ``set_model_params`` refuses every name of
    that table and refreshes the mirror from the device before it rewrites any other."""
    owns_masses = True

    def __init__(self, plant_task, model_task, samples, adapt, *args, **kwargs):
        import torch
        if not hasattr(adapt, "keys"):
            raise ConfigError("mpc adapt: adapt={params: {NAME: [lo, hi]}, ...} must be a mapping, not %r" % (adapt,))
        check_masses(adapt)
        if model_task.env_params is None:
            raise ConfigError("mpc adapt: the model task has no per-env parameter table bound (task.env.ENV_PARAMS is empty): "
                              "the table is what is adapted")
        if model_task.env_inertia is None:
            raise ConfigError("mpc adapt: masses needs an inertia table bound to the model task (a mass name in its "
                              "task.env.ENV_PARAMS): that table is what is adapted")
        self.spec = adapt
        base, self.placeholder = base_spec(adapt, model_task.env_params.cpu().numpy())
        super().__init__(plant_task, model_task, samples, base, *args, **kwargs)
        if self.placeholder:       # prior std, std and floor 0: its candidates and planning value are the model's own bits
            logging.getLogger(__name__).info(
                "mpc adapt: masses without params: the base launches get the placeholder dimension %s with std 0 (the model's "
                "own values)", PLACEHOLDER)
            self.names = []
            self.acfg.dims[0].std_floor = 0.0
            self.dims = mpc_adapt.dims_of(self.acfg)
            self.prior_std.zero_()
            self.std.zero_()
        vcfg = model_task._vcfg
        self.base_inertia = env_params.inertia_config_row(self.lib, vcfg)
        self.icfg, self.mass_names = masses_config(adapt, self.base_inertia, vcfg.link_length, vcfg.link_com, vcfg.gravity)
        self.mdims = mass_dims_of(self.icfg)
        self.Dm = int(self.icfg.num_mass_dims)
        self.derive = lambda t: env_params.derive_inertia(self.lib, vcfg, t)
        held = mass_values(model_task.env_inertia[:, ::self.K].cpu().numpy(), self.mdims, self.base_inertia)
        lo = np.array([d[1] for d in self.mdims], dtype=np.float64)
        hi = np.array([d[2] for d in self.mdims], dtype=np.float64)
        dev = self.device
        self.mass_prior_mean = torch.as_tensor(np.minimum(np.maximum(held, lo), hi), device=dev)
        self.mass_prior_std = torch.as_tensor(np.broadcast_to(self.acfg.spread * (hi - lo), held.shape).copy(), device=dev)
        self.mass_mean, self.mass_std = self.mass_prior_mean.clone(), self.mass_prior_std.clone()
        keep = self.adapt_weights is not None                            # (``keep_weights``: the diagnostic, as the base's)
        self.mass_weights = torch.zeros(self.M * self.K, dtype=torch.float64, device=dev) if keep else None
        self.launches.update({"inertia_pin": 0, "inertia_estimate": 0})
        self._write_mass_plan()

    def _write_mass_plan(self):
        """The planning column of the current mass belief into the model's inertia table, from the host (at construction
        only: a prior outside its range was clamped, and an absent name is held at the configuration's value)."""
        import torch
        plan = np.repeat(self.mass_mean.cpu().numpy(), self.K, axis=0)
        self.model.env_inertia.copy_(torch.from_numpy(inertia_rows(plan, self.mdims, self.base_inertia, self.derive)))

    def tensors(self):
        extra = [self.mass_mean, self.mass_std, self.model.env_inertia]
        return super().tensors() + extra + ([self.mass_weights] if self.mass_weights is not None else [])

    # -- the two launches ------------------------------------------------------------------------------------------------
    def inertia_pin(self):
        from .. import native
        m = self.model
        native.check(self.lib.vine_mpc_adapt_inertia_pin(
            m._handle, self.acfg, self.icfg, m.env_inertia.data_ptr(), self.mass_mean.data_ptr(), self.mass_std.data_ptr(),
            self.passes.data_ptr(), self._stream()), self.lib)
        self.launches["inertia_pin"] += 1

    def inertia_estimate(self):
        from .. import native
        m = self.model
        native.check(self.lib.vine_mpc_adapt_inertia_estimate(
            m._handle, self.acfg, self.icfg, m.env_inertia.data_ptr(), self.err.data_ptr(), self.trace_len.data_ptr(),
            self.episode_ended.data_ptr(), self.mass_mean.data_ptr(), self.mass_std.data_ptr(), self.mass_prior_mean.data_ptr(),
            self.mass_prior_std.data_ptr(), self.passes.data_ptr(),
            self.mass_weights.data_ptr() if self.mass_weights is not None else None, self._stream()), self.lib)
        self.launches["inertia_estimate"] += 1

    def pin(self):
        super().pin()
        self.inertia_pin()              # directly behind the base pin, which does not read the inertia table

    def estimate(self):
        self.inertia_estimate()         # in front of the base estimate: passes[p] is still the pin's
        super().estimate()

    # -- from outside the step -------------------------------------------------------------------------------------------
    def set_model_params(self, values):
        """``AdaptiveController.set_model_params`` for what the mass belief does not own: a name of the inertia table is
        refused by name (the device rewrites the whole column every pass), and the inertia mirror is refreshed from the
        device first."""
        primary = self.model.env_inertia_names[:abi.VI_PRIMARY_COUNT]
        for name in values:
            if name in self.mass_names:
                raise ValueError("set_model_params: %s is adapted on the device (adapt.masses: %s); the belief owns it"
                                 % (name, ", ".join(self.mass_names)))
            if name in NAMES or name in primary:
                raise ValueError("set_model_params: %s lies in the inertia table, whose whole column the mass belief writes "
                                 "(adapt.masses: %s; an absent name is held at the configuration's value)"
                                 % (name, ", ".join(self.mass_names)))
        self.model._env_inertia_host = self.model.env_inertia.cpu().numpy()
        super().set_model_params(values)

    def mass_belief(self):
        """``(mass_mean, mass_std)`` float64 [M, Dm] as of now (synchronises)."""
        return self.mass_mean.cpu().numpy(), self.mass_std.cpu().numpy()

    def mass_truth(self):
        """float64 [M, Dm]: the PLANT's own value of every mass dimension, where the plant task carries an inertia table (else
        ``None``).  The plant's configuration is taken to have the model's masses."""
        if self.plant.env_inertia is None:
            return None
        return mass_values(self.plant.env_inertia.cpu().numpy(), self.mdims, self.base_inertia)


# ------------------------------------------------------------------------------------------------------------------ a run
def bind(run):
    """An inertia table for the model where none would be bound: the configuration's own row, as ``{FPAM_K: 1.0}`` binds the
    parameter table."""
    spec = run.mcfg["env"]["ENV_PARAMS"]
    if not any(name in spec for name in NAMES):
        spec["LINK_MASS"] = 1.0


def controller(run, spec, forget_on_reset):
    mass_names = [name for name, _lo, _hi in check_masses(spec)]
    if run.draws:                  # the prior is the model's value when the controller is made
        for name in run.draws:
            if name in NAMES and name not in mass_names:
                raise ConfigError("mpc adapt: model_params.%s is not among adapt.masses (%s): the mass belief writes the whole "
                                  "inertia column and holds an absent name at the configuration's value" % (
                                      name, ", ".join(mass_names)))
        run.model.set_env_params({k: np.repeat(v, int(run.samples)) for k, v in run.draws.items()})
        run.draws = None
    return AdaptiveInertiaController(run.plant, run.model, run.samples, spec, *run.planner, graph=run.graph,
                                     forget_on_reset=forget_on_reset)


def epilogue(ctl, out):
    """The mass names' entries of ``out["adapt"]`` and their printed lines."""
    mean, std = ctl.mass_belief()
    prior, truth = ctl.mass_prior_mean.cpu().numpy(), ctl.mass_truth()
    a = out["adapt"]
    a["mass_names"] = list(ctl.mass_names)
    a["names"] = list(a["names"]) + list(ctl.mass_names)
    a.update({"mass_mean": mean, "mass_std": std, "mass_prior_mean": prior, "mass_truth": truth})
    for i, name in enumerate(ctl.mass_names):
        if truth is None:
            print("  adapt %s: final mean %s, std %s" % (name, np.array2string(mean[:, i], precision=4),
                                                         np.array2string(std[:, i], precision=4)), flush=True)
            continue
        a["prior_error"][name] = float(np.abs(prior[:, i] - truth[:, i]).mean())
        a["final_error"][name] = float(np.abs(mean[:, i] - truth[:, i]).mean())
        print("  adapt %s: mean |prior - truth| %.4g, mean |belief - truth| %.4g (final mean %.4g, std %.4g on average)" % (
            name, a["prior_error"][name], a["final_error"][name], mean[:, i].mean(), std[:, i].mean()), flush=True)
