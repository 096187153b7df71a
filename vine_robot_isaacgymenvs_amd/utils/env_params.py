"""ENV_PARAMS on the host side: the per-env parameter table of ``vine_bind_env_params`` (include/vine_env_params.h) from a
spec in the task config.

``task.env.ENV_PARAMS`` maps a parameter name (``abi.ENV_PARAM_NAMES``: the task YAML's own keys) to one of

  a number               every env gets it;
  ``[lo, hi]``           uniform per env (for ``ACTION_DELAY``: over the integers lo..hi, both ends included);
  ``{values: [v0, ..]}`` env ``g`` gets ``values[digit]``: the ``values`` entries of a spec together count ``g`` in a mixed
                         radix, the first entry being the fastest digit, so every combination recurs every ``prod(len)`` envs.

A name that is absent keeps the configuration's value (``vine_env_params_row``).  The four FPAM vectors (``FPAM_K``, ``FPAM_C``,
``FPAM_b``, ``FPAM_B``) take all three forms as a FACTOR on the configuration's five constants, which differ by design.

Three more names fill the inertia table of ``vine_bind_env_inertia`` (include/vine_env_inertia.h) instead, in the same three
forms and in the same mixed-radix count: ``CART_MASS`` in kg; ``LINK_MASS``, one factor per env on the configuration's five
link masses and on their inertias about the COM (the geometry is unchanged, so the inertia scales with the mass);
``TIP_LINK_MASS``, a further factor on link 4's mass and inertia only, the payload case: link 4 gets
``configuration * LINK_MASS * TIP_LINK_MASS``.  ``build_table`` passes over them, ``build_inertia_table`` over the others.

What env ``g`` gets depends on ``(seed, name, g)`` with ``g`` the GLOBAL env id (``env_id_offset`` + local index), never on
the batch size: a rank's shard equals its slice of the whole batch, the rule the step's own random streams follow."""
import ctypes as C

import numpy as np

from .. import abi
from . import named_draw
from .config import ConfigError
from .named_draw import name_key, uniform01_episode  # noqa: F401  (the hash is stated in named_draw; callers find it here too)

INTEGER = ("ACTION_DELAY",)      # the names whose range is over the integers


def uniform01(seed, name, gids):
    """One float64 in [0, 1) per global env id, a pure function of ``(seed, name, id)``: episode 0 of ``uniform01_episode``."""
    return uniform01_episode(seed, name, gids, 0)


def config_row(lib, vcfg):
    """``vine_env_params_row``: the configuration's own value of every row, float32 [VP_COUNT]."""
    row = (C.c_float * abi.VP_COUNT)()
    rc = lib.vine_env_params_row(C.byref(vcfg), row)
    if rc != abi.OK:
        raise ValueError(lib.vine_last_error().decode(errors="replace"))
    return np.array(row, dtype=np.float32)


def check_table(lib, vcfg, table):
    """``vine_env_params_check`` on a host table [VP_COUNT, N]; raises ``ValueError`` naming the parameter and the env."""
    t = np.ascontiguousarray(table, dtype=np.float32)
    if t.ndim != 2 or t.shape[0] != abi.VP_COUNT or t.shape[1] < 1:
        raise ValueError("env params: the table must be [%d, num_envs], not %s" % (abi.VP_COUNT, t.shape))
    rc = lib.vine_env_params_check(C.byref(vcfg) if vcfg is not None else None, t.ctypes.data, t.shape[1])
    if rc != abi.OK:
        raise ValueError(lib.vine_last_error().decode(errors="replace"))
    return t


def inertia_config_row(lib, vcfg):
    """``vine_env_inertia_row``: the configuration's own value of every row, primary and derived, float32 [VI_COUNT]."""
    row = (C.c_float * abi.VI_COUNT)()
    rc = lib.vine_env_inertia_row(C.byref(vcfg), row)
    if rc != abi.OK:
        raise ValueError(lib.vine_last_error().decode(errors="replace"))
    return np.array(row, dtype=np.float32)


def _inertia_table(table):
    t = np.ascontiguousarray(table, dtype=np.float32)
    if t.ndim != 2 or t.shape[0] != abi.VI_COUNT or t.shape[1] < 1:
        raise ValueError("env inertia: the table must be [%d, num_envs], not %s" % (abi.VI_COUNT, t.shape))
    return t


def derive_inertia(lib, vcfg, table):
    """``vine_env_inertia_derive``: a copy of the host table [VI_COUNT, N] with the derived rows filled from the primary."""
    t = _inertia_table(table).copy()
    rc = lib.vine_env_inertia_derive(C.byref(vcfg), t.ctypes.data, t.shape[1])
    if rc != abi.OK:
        raise ValueError(lib.vine_last_error().decode(errors="replace"))
    return t


def check_inertia_table(lib, vcfg, table):
    """``vine_env_inertia_check`` on a host table [VI_COUNT, N]; raises ``ValueError`` naming the row and the env."""
    t = _inertia_table(table)
    rc = lib.vine_env_inertia_check(C.byref(vcfg), t.ctypes.data, t.shape[1])
    if rc != abi.OK:
        raise ValueError(lib.vine_last_error().decode(errors="replace"))
    return t


def _number(name, v):
    return named_draw.number("ENV_PARAMS.%s" % name, v, finite=False)       # (an infinite end is the table checks' to refuse)


def build_table(spec, vcfg, seed, num_envs, env_id_offset=0, lib=None):
    """The table float32 [VP_COUNT, num_envs] of the envs with global ids ``env_id_offset .. env_id_offset + num_envs - 1``
    (see the module's docstring for ``spec``).  ``vcfg``: the handle's ``abi.VineConfig``.  Raises ``ConfigError`` for an
    unknown name or a malformed entry and ``ValueError`` for a value ``vine_env_params_check`` refuses."""
    if lib is None:
        from .. import native
        lib = native.load()
    return draw_table(spec, config_row(lib, vcfg), seed, num_envs, env_id_offset, check=lambda t: check_table(lib, vcfg, t))


def spec_forms(spec):
    """``{name: v / [lo, hi] / {"values": [..]}}`` of a spec, in its order (``named_draw.form``: the spec as plain numbers
    and lists, what the episode file stores as JSON); raises ``ConfigError`` for an unknown name or a malformed entry."""
    spec = spec or {}
    if not hasattr(spec, "keys"):
        raise ConfigError("ENV_PARAMS must be a mapping of parameter names, not %r" % (spec,))
    for name in spec.keys():
        if name not in abi.ENV_PARAM_ROWS and name not in abi.ENV_INERTIA_NAMES:
            raise ConfigError("ENV_PARAMS: unknown parameter %r (known: %s)" % (
                name, ", ".join(abi.ENV_PARAM_NAMES + abi.ENV_INERTIA_NAMES)))
    forms = {name: named_draw.form("ENV_PARAMS.%s" % name, spec[name], finite=False) for name in spec.keys()}
    for name in INTEGER:
        f = forms.get(name)
        if isinstance(f, list) and (f[0] != np.floor(f[0]) or f[1] != np.floor(f[1])):
            raise ConfigError("ENV_PARAMS.%s: an integer parameter takes an integer range, not [%g, %g]" % (name, f[0], f[1]))
    return forms


def set_rows(table, base, name, v):
    """Write the per-env values ``v`` (float64 [N]) of ``name`` into ``table``: the value itself, or for an FPAM vector the
    factor on the configuration's five constants ``base``."""
    first, count = abi.ENV_PARAM_ROWS[name]
    if count == 1:
        table[first] = v.astype(np.float32)
    else:
        table[first:first + count] = (base[first:first + count, None].astype(np.float64) * v[None, :]).astype(np.float32)


def set_inertia_rows(table, base, draws):
    """Write the PRIMARY rows of the inertia ``table`` [VI_COUNT, N] from the configuration's row ``base`` and the per-env
    values ``draws`` (name -> float64 [N]; an absent name keeps the configuration's): the cart's mass itself; link i's mass
    and inertia = the configuration's * LINK_MASS (* TIP_LINK_MASS for link 4), formed in float64 and rounded once.  The
    derived rows are left for ``derive_inertia``."""
    n = table.shape[1]
    base = np.asarray(base, dtype=np.float64)
    table[abi.VI_CART_MASS] = (draws["CART_MASS"] if "CART_MASS" in draws else np.full(n, base[abi.VI_CART_MASS])).astype(np.float32)
    link = np.asarray(draws.get("LINK_MASS", np.ones(n)), dtype=np.float64)
    tip = np.asarray(draws.get("TIP_LINK_MASS", np.ones(n)), dtype=np.float64)
    for i in range(abi.NUM_LINKS):
        f = link * tip if i == abi.NUM_LINKS - 1 else link
        table[abi.VI_LINK_MASS0 + i] = (base[abi.VI_LINK_MASS0 + i] * f).astype(np.float32)
        table[abi.VI_LINK_INERTIA0 + i] = (base[abi.VI_LINK_INERTIA0 + i] * f).astype(np.float32)


def _candidates(forms):
    """What a spec CAN give an env, per name: both ends of a range, every listed value, the number."""
    return {name: named_draw.candidates(f) for name, f in forms.items()}


def draw_inertia_table(spec, base, seed, num_envs, derive, env_id_offset=0, check=None, draws=None):
    """``build_inertia_table`` from the configuration's row ``base`` (float32 [VI_COUNT]).  ``derive(table)`` returns the
    table with its derived rows filled (``derive_inertia`` bound to a library and a configuration); ``check`` and ``draws``
    as in ``draw_table``.  ``None`` when the spec names none of ``abi.ENV_INERTIA_NAMES``."""
    num_envs = int(num_envs)
    if num_envs < 1:
        raise ValueError("ENV_PARAMS: num_envs must be positive")
    forms = spec_forms(spec)
    if not any(name in forms for name in abi.ENV_INERTIA_NAMES):
        return None
    base = np.asarray(base, dtype=np.float32)
    gids = np.arange(num_envs, dtype=np.int64) + int(env_id_offset)
    cand = {name: c for name, c in _candidates(forms).items() if name in abi.ENV_INERTIA_NAMES}
    width = max(len(c) for c in cand.values())
    probe = np.repeat(base[:, None], width, axis=1)
    set_inertia_rows(probe, base, {name: np.asarray([c[i % len(c)] for i in range(width)], dtype=np.float64)
                                   for name, c in cand.items()})
    if check is not None:
        try:
            check(derive(probe))
        except ValueError as e:
            raise ValueError("ENV_PARAMS: %s" % str(e).replace(" of env ", " of candidate ")) from None
    drawn = {name: v for name, v in _draw_episode(forms, seed, gids, 0).items() if name in abi.ENV_INERTIA_NAMES}
    table = np.repeat(base[:, None], num_envs, axis=1)
    set_inertia_rows(table, base, drawn)
    if draws is not None:
        draws.update(drawn)
    table = derive(table)
    if check is None:
        return table
    try:
        return check(table)
    except ValueError as e:
        raise ValueError("ENV_PARAMS: %s" % e) from None


def build_inertia_table(spec, vcfg, seed, num_envs, env_id_offset=0, lib=None):
    """The inertia table float32 [VI_COUNT, num_envs] of the envs with global ids ``env_id_offset ..`` from the names
    ``CART_MASS``, ``LINK_MASS`` and ``TIP_LINK_MASS`` of ``spec`` (the module's docstring), derived rows filled and the whole
    checked through the library; ``None`` when the spec names none of the three.  Raises as ``build_table`` does."""
    if lib is None:
        from .. import native
        lib = native.load()
    return draw_inertia_table(spec, inertia_config_row(lib, vcfg), seed, num_envs, lambda t: derive_inertia(lib, vcfg, t),
                              env_id_offset, check=lambda t: check_inertia_table(lib, vcfg, t))


def draw_table(spec, base, seed, num_envs, env_id_offset=0, check=None, draws=None):
    """``build_table`` from the configuration's row ``base`` (float32 [VP_COUNT]) instead of a handle's config: pure numpy.
    ``check``: called with the probe of what the spec can give an env and with the finished table (``check_table`` bound to
    a library), or ``None``.  ``draws``: a dict that receives, per name, the float64 [N] values (factors for the FPAM
    vectors) the table was formed from."""
    num_envs = int(num_envs)
    if num_envs < 1:
        raise ValueError("ENV_PARAMS: num_envs must be positive")
    forms = spec_forms(spec)
    base = np.asarray(base, dtype=np.float32)
    table = np.repeat(base[:, None], num_envs, axis=1)
    gids = np.arange(num_envs, dtype=np.int64) + int(env_id_offset)
    # what the spec CAN give an env is checked whatever this batch happens to draw: both ends of a range, every value
    # (the names of the inertia table are draw_inertia_table's to place: here they only take part in the mixed radix)
    cand = {name: c for name, c in _candidates(forms).items() if name in abi.ENV_PARAM_ROWS}
    width = max([len(c) for c in cand.values()] + [1])
    probe = np.repeat(base[:, None], width, axis=1)
    for name, c in cand.items():
        first, count = abi.ENV_PARAM_ROWS[name]
        v = np.asarray([c[i % len(c)] for i in range(width)], dtype=np.float64)
        probe[first:first + count] = (v[None, :] * (base[first:first + count, None].astype(np.float64) if count > 1 else 1.0)
                                      ).astype(np.float32)
    if check is not None:
        try:
            check(probe)
        except ValueError as e:
            raise ValueError("ENV_PARAMS: %s" % str(e).replace(" of env ", " of candidate ")) from None
    for name, v in _draw_episode(forms, seed, gids, 0).items():
        if name in abi.ENV_PARAM_ROWS:
            set_rows(table, base, name, v)
        if draws is not None:
            draws[name] = v
    table = np.ascontiguousarray(table, dtype=np.float32)
    if check is None:
        return table
    try:
        return check(table)
    except ValueError as e:
        raise ValueError("ENV_PARAMS: %s" % e) from None


def varying_rows(table):
    """Indices of the rows whose values differ across envs."""
    t = np.asarray(table)
    return [p for p in range(t.shape[0]) if np.any(t[p] != t[p, 0])]


# ---- ENV_PARAMS_PER_EPISODE (include/vine_env_redraw.h): the draw of episode k, and the spec the device redraws from
def per_episode(env_cfg):
    """Is ``ENV_PARAMS_PER_EPISODE`` on in the ``task.env`` mapping?  ``ConfigError`` when it is and ``ENV_PARAMS`` is empty."""
    if not env_cfg.get("ENV_PARAMS_PER_EPISODE", False):
        return False
    if not len(env_cfg.get("ENV_PARAMS") or {}):
        raise ConfigError("task.env.ENV_PARAMS_PER_EPISODE needs a non-empty task.env.ENV_PARAMS: there is no plant to redraw")
    return True


def _draw_episode(forms, seed, gids, episodes):
    """name -> float64 [M], the value of every name of a spec for (global env id, episode) pairs: ``named_draw.draw`` over
    ALL names of the spec, in its order, whichever table a name fills.  Episode 0 is what the tables are set up from."""
    return dict(zip(forms, named_draw.draw(list(forms.items()), seed, gids, episodes, INTEGER, who="draw_columns")))


def draw_columns(spec, base, inertia_base, derive, seed, gids, episodes):
    """The columns of M ``(global env id, episode)`` pairs: ``(params [VP_COUNT, M], inertia [VI_COUNT, M])`` float32, formed
    exactly as ``draw_table`` / ``draw_inertia_table`` form a table (float64 throughout, rounded once); episode 0 is bit for
    bit their table.  ``base`` / ``inertia_base``: the configuration's rows (``config_row`` / ``inertia_config_row``);
    ``derive(table)``: ``derive_inertia`` bound to a library and a configuration.  ``inertia`` is ``None`` when the spec names
    none of ``abi.ENV_INERTIA_NAMES``.  What the device's redraw (include/vine_env_redraw.h) is compared against."""
    forms = spec_forms(spec)
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    episodes = np.broadcast_to(np.asarray(episodes, dtype=np.int64), gids.shape)
    if np.any(gids < 0) or np.any(episodes < 0):
        raise ValueError("draw_columns: env ids and episodes are non-negative")
    return columns_of(forms, _draw_episode(forms, seed, gids, episodes), base, inertia_base, derive, len(gids))


def columns_of(forms, drawn, base, inertia_base, derive, count):
    """The two columns of ``count`` envs from the per-name values ``drawn`` (name -> float64 [count]) of a spec's ``forms``:
    the last step of ``draw_columns``."""
    gids = range(count)
    base = np.asarray(base, dtype=np.float32)
    params = np.repeat(base[:, None], len(gids), axis=1)
    for name, v in drawn.items():
        if name in abi.ENV_PARAM_ROWS:
            set_rows(params, base, name, v)
    params = np.ascontiguousarray(params, dtype=np.float32)
    if not any(name in forms for name in abi.ENV_INERTIA_NAMES):
        return params, None
    ibase = np.asarray(inertia_base, dtype=np.float32)
    inertia = np.repeat(ibase[:, None], len(gids), axis=1)
    set_inertia_rows(inertia, ibase, {name: v for name, v in drawn.items() if name in abi.ENV_INERTIA_NAMES})
    return params, derive(inertia)


def build_columns(spec, vcfg, gids, episodes, lib=None, seed=None):
    """``draw_columns`` with the rows, the derivation and the seed of a handle's ``abi.VineConfig``."""
    if lib is None:
        from .. import native
        lib = native.load()
    return draw_columns(spec, config_row(lib, vcfg), inertia_config_row(lib, vcfg), lambda t: derive_inertia(lib, vcfg, t),
                        int(vcfg.seed) if seed is None else seed, gids, episodes)


def redraw_names(spec):
    """``(abi.VineEnvRedrawName * VR_NAMES, values float64 [V])`` of a spec (``named_draw.pack``), every name in its slot of
    ``abi.ENV_REDRAW_NAMES``; a name the spec does not hold stays ABSENT."""
    return named_draw.pack(list(spec_forms(spec).items()), abi.VR_NAMES, abi.ENV_REDRAW_NAMES.index)


def redraw_spec(lib, vcfg, spec, device_values=None):
    """``vine_env_redraw_spec``: the checked ``abi.VineEnvRedrawSpec`` of a spec.  ``device_values``: address of the float64
    device array holding ``redraw_names(spec)[1]`` (needed when the spec has a ``values`` entry).  Raises ``ConfigError`` for
    a malformed spec and ``ValueError`` for one whose ends or listed values the table checks refuse."""
    names, values = redraw_names(spec)
    out = abi.VineEnvRedrawSpec()
    rc = lib.vine_env_redraw_spec(C.byref(vcfg), names, values.ctypes.data if len(values) else None,
                                  device_values if len(values) else None, len(values), C.byref(out))
    if rc != abi.OK:
        raise ValueError("ENV_PARAMS: %s" % lib.vine_last_error().decode(errors="replace"))
    return out


# ---- ENV_PARAMS_ADR (include/vine_env_adr.h): the ranges widen on the device as the policy masters them
ADR_DEFAULTS = {"BOUNDARY_FRACTION": 0.25, "QUEUE": 256, "WIDEN_AT": 0.8, "NARROW_AT": 0.4, "HISTORY_CAPACITY": 1024}
_ADR = "task.env.ENV_PARAMS_ADR"


def adr_config(env_cfg, multi_gpu=False):
    """The checked ``task.env.ENV_PARAMS_ADR`` of the ``task.env`` mapping as plain numbers, ``None`` when it is empty (off):
    ``{"NAMES": {NAME: {"START": [lo, hi], "STEP": s}}`` (in slot order), ``"BOUNDARY_FRACTION"``, ``"QUEUE"``, ``"WIDEN_AT"``,
    ``"NARROW_AT"``, ``"HISTORY_CAPACITY"}``.  ``ConfigError``, naming the key, for everything include/vine_env_adr.h refuses
    and for what only the configuration knows: ADR without ``ENV_PARAMS_PER_EPISODE``, ADR under ``multi_gpu``."""
    adr = env_cfg.get("ENV_PARAMS_ADR") or {}
    if not hasattr(adr, "keys"):
        raise ConfigError("%s must be a mapping, not %r" % (_ADR, adr))
    if not len(adr):
        return None
    unknown = sorted(set(adr.keys()) - set(ADR_DEFAULTS) - {"NAMES"})
    if unknown:
        raise ConfigError("%s: unknown key(s) %s" % (_ADR, ", ".join(unknown)))
    if not env_cfg.get("ENV_PARAMS_PER_EPISODE", False):
        raise ConfigError("%s needs task.env.ENV_PARAMS_PER_EPISODE: the ranges are those an env's plant is redrawn from" % _ADR)
    if multi_gpu:
        raise ConfigError("%s with multi_gpu=True: every rank would grow its own ranges" % _ADR)
    forms = spec_forms(env_cfg.get("ENV_PARAMS") or {})
    names = adr.get("NAMES") or {}
    if not hasattr(names, "keys") or not len(names):
        raise ConfigError("%s.NAMES must map at least one name of ENV_PARAMS to {START: [lo, hi], STEP: s}" % _ADR)
    out = {"NAMES": {}}
    for name in abi.ENV_REDRAW_NAMES:
        if name not in names:
            continue
        entry, where = names[name], "%s.NAMES.%s" % (_ADR, name)
        form = forms.get(name)
        if not isinstance(form, list):
            raise ConfigError("%s: the name must be a [lo, hi] range in task.env.ENV_PARAMS, its limits" % where)
        if not hasattr(entry, "keys") or sorted(entry.keys()) != ["START", "STEP"]:
            raise ConfigError("%s must hold START and STEP" % where)
        start = entry["START"]
        if not isinstance(start, (list, tuple)) or len(start) != 2:
            raise ConfigError("%s.START is [lo, hi], not %r" % (where, start))
        lo, hi, step = _number(where + ".START", start[0]), _number(where + ".START", start[1]), _number(where + ".STEP", entry["STEP"])
        if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
            raise ConfigError("%s.START: lo > hi in [%g, %g]" % (where, lo, hi))
        if lo < form[0] or hi > form[1]:
            raise ConfigError("%s.START [%g, %g] lies outside the limits [%g, %g]" % (where, lo, hi, form[0], form[1]))
        if not np.isfinite(step) or not step > 0.0:
            raise ConfigError("%s.STEP must be positive, not %g" % (where, step))
        if name == "ACTION_DELAY" and (lo != np.floor(lo) or hi != np.floor(hi) or step != np.floor(step)):
            raise ConfigError("%s: an integer parameter takes an integer START and STEP" % where)
        out["NAMES"][name] = {"START": [lo, hi], "STEP": step}
    stray = sorted(set(names.keys()) - set(out["NAMES"]))
    if stray:
        raise ConfigError("%s.NAMES.%s: unknown parameter (known: %s)" % (_ADR, stray[0], ", ".join(abi.ENV_REDRAW_NAMES)))
    for key, default in ADR_DEFAULTS.items():
        out[key] = _number("%s.%s" % (_ADR, key), adr.get(key, default))
    if not 0.0 <= out["BOUNDARY_FRACTION"] < 1.0:
        raise ConfigError("%s.BOUNDARY_FRACTION must lie in [0, 1), not %g" % (_ADR, out["BOUNDARY_FRACTION"]))
    for key in ("QUEUE", "HISTORY_CAPACITY"):
        if out[key] != np.floor(out[key]) or out[key] < 1:
            raise ConfigError("%s.%s must be an integer >= 1, not %g" % (_ADR, key, out[key]))
        out[key] = int(out[key])
    if not (np.isfinite(out["WIDEN_AT"]) and np.isfinite(out["NARROW_AT"])) or out["NARROW_AT"] >= out["WIDEN_AT"]:
        raise ConfigError("%s.NARROW_AT (%g) must be below WIDEN_AT (%g)" % (_ADR, out["NARROW_AT"], out["WIDEN_AT"]))
    return out


def adr_start_spec(spec, adr):
    """``spec`` with the range of every name under ADR replaced by its START: what episode 0 is drawn from."""
    out = {name: spec[name] for name in spec.keys()}
    for name, a in adr["NAMES"].items():
        out[name] = [a["START"][0], a["START"][1]]
    return out


def adr_max_widen(spec, adr):
    """int64 [VR_NAMES, 2]: the steps between START and the limit per boundary, ``ceil((start_lo - limit_lo) / step)`` and
    ``ceil((limit_hi - start_hi) / step)``, one more where the rounded quotient would leave the last step short of the limit;
    0 for a name that is not under ADR."""
    forms = spec_forms(spec)
    out = np.zeros((abi.VR_NAMES, 2), dtype=np.int64)
    for name, a in adr["NAMES"].items():
        s = abi.ENV_REDRAW_NAMES.index(name)
        lo, hi, step = np.float64(a["START"][0]), np.float64(a["START"][1]), np.float64(a["STEP"])
        m_lo, m_hi = np.ceil((lo - forms[name][0]) / step), np.ceil((forms[name][1] - hi) / step)
        out[s, 0] = int(m_lo) + (1 if lo - m_lo * step > forms[name][0] else 0)      # (the last step arrives AT the limit, not
        out[s, 1] = int(m_hi) + (1 if hi + m_hi * step < forms[name][1] else 0)      # an ulp inside it)
    return out


def adr_ranges(spec, adr, widen):
    """``{NAME: (lo, hi)}`` in force under ``widen`` (int [VR_NAMES, 2]): ``lo = max(limit_lo, start_lo - widen_lo * step)``,
    ``hi = min(limit_hi, start_hi + widen_hi * step)``, one multiply and one add in float64, as the device forms them."""
    forms = spec_forms(spec)
    widen = np.asarray(widen, dtype=np.int64).reshape(abi.VR_NAMES, 2)
    out = {}
    for name, a in adr["NAMES"].items():
        s = abi.ENV_REDRAW_NAMES.index(name)
        step = np.float64(a["STEP"])
        lo = max(np.float64(forms[name][0]), np.float64(a["START"][0]) - np.float64(widen[s, 0]) * step)
        hi = min(np.float64(forms[name][1]), np.float64(a["START"][1]) + np.float64(widen[s, 1]) * step)
        out[name] = (float(lo), float(hi))
    return out


def adr_draw(spec, adr, seed, gids, episodes, widen):
    """What launch 2 draws for ``(global env id, episode >= 1)`` pairs under ``widen``: ``(forms, drawn, probe)`` with
    ``drawn`` name -> float64 [M] (a probing episode's name set to exactly its boundary) and ``probe`` int64 [M], the
    boundary ``2 * slot + side`` or -1."""
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    k = np.broadcast_to(np.asarray(episodes, dtype=np.int64), gids.shape)
    forms = dict(spec_forms(spec))
    ranges = adr_ranges(spec, adr, widen)
    for name, (lo, hi) in ranges.items():
        forms[name] = [lo, hi]
    drawn = _draw_episode(forms, seed, gids, k)
    slots = [abi.ENV_REDRAW_NAMES.index(name) for name in adr["NAMES"]]
    count = 2 * len(slots)
    u_p = uniform01_episode(seed, "ADR_PROBE", gids, k)
    u_w = uniform01_episode(seed, "ADR_WHICH", gids, k)
    j = np.minimum(np.floor(u_w * float(count)).astype(np.int64), count - 1)
    probe = np.where(u_p < adr["BOUNDARY_FRACTION"], 2 * np.asarray(slots, dtype=np.int64)[j >> 1] + (j & 1), -1)
    for name, (lo, hi) in ranges.items():
        s = abi.ENV_REDRAW_NAMES.index(name)
        drawn[name] = np.where(probe == 2 * s, lo, np.where(probe == 2 * s + 1, hi, drawn[name]))
    return forms, drawn, probe


def adr_decide(adr, max_widen, widen, counts, step_index, history, consumed=None, slots=abi.ENV_REDRAW_NAMES):
    """Launch 1 on the host, in place: judge every boundary with ``counts.n >= QUEUE``, clear its counts (adding them to
    ``consumed`` when given), append one row ``[step index, boundary, new widen, 0]`` to the list ``history`` per boundary
    that changed, in boundary order.  ``slots``: the names in slot order (``adr["NAMES"]`` is in that order too); the default
    is the plant's, utils/env_draw_adr.py passes the nine draw names."""
    for name in adr["NAMES"]:
        s = slots.index(name)
        for side in (0, 1):
            n, r = int(counts[s, side, 0]), int(counts[s, side, 1])
            if n < adr["QUEUE"]:
                continue
            w = int(widen[s, side])
            if float(r) >= adr["WIDEN_AT"] * float(n):
                w = min(w + 1, int(max_widen[s, side]))
            elif float(r) <= adr["NARROW_AT"] * float(n):
                w = max(w - 1, 0)
            if w != widen[s, side]:
                widen[s, side] = w
                history.append([int(step_index), 2 * s + side, w, 0])
            if consumed is not None:
                consumed[s, side] += counts[s, side]
            counts[s, side] = 0


def adr_replay(spec, adr, seed, gids, resets, reached_flags, vcfg, lib=None, step_index=None, widen0=None):
    """Both launches of ``vine_env_adr_scheduled`` on the host, step by step, in float64 and integers.  ``spec``: the
    ENV_PARAMS mapping (the limits); ``adr``: ``adr_config``'s result; ``gids`` [N]: global env ids; ``resets`` and
    ``reached_flags`` [T, N]: the step's reset buffer and ``reward matrix[:, 2] != 0`` as the launches behind step t see them;
    ``vcfg``: the handle's ``abi.VineConfig`` (base rows and the derivation); ``step_index`` [T]: what the history rows carry
    (default ``0 .. T - 1``: the launches ride behind steps 0, 1, ...); ``widen0`` [VR_NAMES, 2]: the ``widen`` in force
    before the first step (default zeros; a run resumed from a checkpoint starts from the checkpoint's).  Returns one dict per step, the state BEHIND that
    step's launches: ``widen`` [VR_NAMES, 2], ``counts`` [VR_NAMES, 2, 2], ``probe``, ``reached``, ``episode_index`` [N],
    ``params`` [VP_COUNT, N], ``inertia`` [VI_COUNT, N] or ``None``, ``history`` [H, 4] (every row so far), ``cursor``,
    ``delay_changed`` (bool [N]: the envs whose delay ring that step's launch zeroed) and ``consumed`` [VR_NAMES, 2, 2] (the
    counts decisions have cleared so far).  Episode 0 is ``build_table`` /
    ``build_inertia_table`` of ``adr_start_spec``."""
    if lib is None:
        from .. import native
        lib = native.load()
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    resets = np.asarray(resets).reshape(-1, len(gids)) != 0
    flags = np.asarray(reached_flags).reshape(-1, len(gids)) != 0
    steps = np.arange(len(resets)) if step_index is None else np.asarray(step_index, dtype=np.int64)
    base, ibase = config_row(lib, vcfg), inertia_config_row(lib, vcfg)
    derive = lambda t: derive_inertia(lib, vcfg, t)      # noqa: E731
    params, inertia = draw_columns(adr_start_spec(spec, adr), base, ibase, derive, seed, gids, 0)
    max_widen = adr_max_widen(spec, adr)
    widen = np.zeros((abi.VR_NAMES, 2), dtype=np.int64) if widen0 is None else np.array(widen0, dtype=np.int64).reshape(abi.VR_NAMES, 2)
    counts = np.zeros((abi.VR_NAMES, 2, 2), dtype=np.int64)
    reached, probe = np.zeros(len(gids), dtype=np.int64), np.full(len(gids), -1, dtype=np.int64)
    episode = np.zeros(len(gids), dtype=np.int64)
    history, out, consumed = [], [], np.zeros_like(counts)
    for t in range(len(resets)):
        adr_decide(adr, max_widen, widen, counts, steps[t], history, consumed)
        reached |= flags[t]
        f = np.flatnonzero(resets[t])
        changed = np.zeros(len(gids), dtype=bool)
        if len(f):
            probing = f[probe[f] >= 0]
            np.add.at(counts, (probe[probing] >> 1, probe[probing] & 1, 0), 1)
            np.add.at(counts, (probe[probing] >> 1, probe[probing] & 1, 1), reached[probing])
            reached[f] = 0
            episode[f] += 1
            forms, drawn, probe[f] = adr_draw(spec, adr, seed, gids[f], episode[f], widen)
            p, i = columns_of(forms, drawn, base, ibase, derive, len(f))
            changed[f] = params[abi.VP_ACTION_DELAY, f] != p[abi.VP_ACTION_DELAY]
            params = params.copy()
            params[:, f] = p
            if i is not None:
                inertia = inertia.copy()
                inertia[:, f] = i
        out.append({"widen": widen.copy(), "counts": counts.copy(), "probe": probe.copy(), "reached": reached.copy(),
                    "episode_index": episode.copy(), "params": params, "inertia": inertia,
                    "history": np.asarray(history, dtype=np.int64).reshape(-1, 4), "cursor": len(history),
                    "delay_changed": changed, "consumed": consumed.copy()})
    return out


def adr_widen_at(history, steps, widen0=None, num_slots=abi.VR_NAMES):
    """int64 [M, VR_NAMES, 2]: the ``widen`` launch 2 read behind each step of ``steps`` [M], from ``widen0`` [VR_NAMES, 2]
    (what was in force before the first step: zeros, or a restored checkpoint's) and the complete ``history`` [H, 4] (a row
    of step s is in force for that step's own redraw: decide runs first).  ``num_slots``: the number of names when it is not
    the plant's ``VR_NAMES`` (utils/env_draw_adr.py: nine)."""
    history = np.asarray(history, dtype=np.int64).reshape(-1, 4)
    steps = np.asarray(steps, dtype=np.int64).reshape(-1)
    out = np.zeros((len(steps), num_slots, 2), dtype=np.int64)
    if widen0 is not None:
        out[:] = np.asarray(widen0, dtype=np.int64).reshape(1, num_slots, 2)
    for s, b, w, _ in history:                       # in the order written: a later row of a boundary overrides
        out[steps >= s, b >> 1, b & 1] = w
    return out


def adr_episode_columns(spec, adr, seed, gids, episodes, drawn_at, history, vcfg=None, lib=None, base=None, inertia_base=None,
                        derive=None, widen0=None):
    """The plant and the probe of M episodes, without a device: ``(params [VP_COUNT, M], inertia [VI_COUNT, M] or None, probe
    [M])``, params and inertia as float64 so that an unknown plant can be NaN.  ``drawn_at`` [M]: the index of the step whose
    launch drew the episode (the step that ended the same env's previous episode), -1 where it is unknown (then NaN and
    probe -2); episode 0 is START's table and probes nothing; ``widen0``: as for ``adr_widen_at``."""
    if base is None:
        if lib is None:
            from .. import native
            lib = native.load()
        base, inertia_base = config_row(lib, vcfg), inertia_config_row(lib, vcfg)
        derive = lambda t: derive_inertia(lib, vcfg, t)      # noqa: E731
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    k = np.asarray(episodes, dtype=np.int64).reshape(-1)
    at = np.asarray(drawn_at, dtype=np.int64).reshape(-1)
    has_inertia = any(name in spec_forms(spec) for name in abi.ENV_INERTIA_NAMES)
    params = np.full((abi.VP_COUNT, len(gids)), np.nan)
    inertia = np.full((abi.VI_COUNT, len(gids)), np.nan) if has_inertia else None
    probe = np.full(len(gids), -2, dtype=np.int64)
    first = np.flatnonzero(k == 0)
    if len(first):
        p, i = draw_columns(adr_start_spec(spec, adr), base, inertia_base, derive, seed, gids[first], 0)
        params[:, first], probe[first] = p, -1
        if has_inertia:
            inertia[:, first] = i
    later = np.flatnonzero((k > 0) & (at >= 0))
    if len(later):
        widen = adr_widen_at(history, at[later], widen0)
        states, inverse = np.unique(widen.reshape(len(later), -1), axis=0, return_inverse=True)
        for j, w in enumerate(states):
            rows = later[np.reshape(inverse, -1) == j]
            forms, drawn, pr = adr_draw(spec, adr, seed, gids[rows], k[rows], w.reshape(abi.VR_NAMES, 2))
            p, i = columns_of(forms, drawn, base, inertia_base, derive, len(rows))
            params[:, rows], probe[rows] = p, pr
            if has_inertia:
                inertia[:, rows] = i
    return params, inertia, probe


def adr_names(adr):
    """``abi.VineEnvAdrName * VR_NAMES`` of ``adr_config``'s result."""
    names = (abi.VineEnvAdrName * abi.VR_NAMES)()
    for name, a in adr["NAMES"].items():
        nm = names[abi.ENV_REDRAW_NAMES.index(name)]
        nm.on, nm.start_lo, nm.start_hi, nm.step = 1, a["START"][0], a["START"][1], a["STEP"]
    return names


def adr_spec(lib, vcfg, spec, adr, device_values=None):
    """``vine_env_adr_spec``: the checked ``abi.VineEnvAdrSpec`` of the ENV_PARAMS mapping ``spec`` (the limits) and
    ``adr_config``'s result.  Raises ``ValueError`` with the library's text for what it refuses."""
    rspec = redraw_spec(lib, vcfg, spec, device_values)
    out = abi.VineEnvAdrSpec()
    rc = lib.vine_env_adr_spec(C.byref(vcfg), C.byref(rspec), adr_names(adr), float(adr["BOUNDARY_FRACTION"]), int(adr["QUEUE"]),
                               float(adr["WIDEN_AT"]), float(adr["NARROW_AT"]), int(adr["HISTORY_CAPACITY"]), C.byref(out))
    if rc != abi.OK:
        raise ValueError("ENV_PARAMS_ADR: %s" % lib.vine_last_error().decode(errors="replace"))
    return out
