"""ENV_DRAW_ADR on the host side: the configuration, the numpy statement of the two launches behind every step
(``draw_adr_replay``: what every GPU test compares against, bit for bit, in float64 and integers), the join of the episode
log (``draw_adr_episode_params``) and the step observer (``EnvDrawAdr``).  The semantics are stated once, in
include/vine_env_draw_adr.h.

``task.env.ENV_DRAW_ADR`` (``{}``: off) maps

  ``NAMES``              ``{DRAW NAME: {START: [lo, hi], STEP: s}}`` over the draw names of ``ENV_SENSOR``, ``ENV_PUSH`` and
                         ``ENV_TARGET`` (``NAMES`` below: nine, in slot order).  The name's ``[lo, hi]`` in its own observer's
                         mapping becomes the limits; the range starts at START and one decision moves one boundary by one STEP
  ``BOUNDARY_FRACTION``, ``QUEUE``, ``WIDEN_AT``, ``NARROW_AT``, ``HISTORY_CAPACITY``
                         as for ``ENV_PARAMS_ADR`` (``env_params.ADR_DEFAULTS``)

The decide rule, the ``widen`` in force behind a step and the step that drew an episode are ``env_params.adr_decide``,
``env_params.adr_widen_at`` and ``episodes.drawn_at``: ENV_PARAMS_ADR's own statements, over these nine slots."""
import ctypes as C

import numpy as np

from .. import abi, native
from . import env_params, env_push, env_sensor, env_target, named_draw
from .config import ConfigError
from .observers import StepObserver

_KEY = "task.env.ENV_DRAW_ADR"
NAMES = tuple(abi.ENV_DRAW_ADR_NAMES)                    # the nine draw names, in slot order
INTEGER = tuple(abi.ENV_DRAW_ADR_INTEGER)                # the draw names whose range is over the integers
GROUPS = ("ENV_SENSOR", "ENV_PUSH", "ENV_TARGET")        # by abi.VDA_SENSOR / _PUSH / _TARGET
_MODULES = (env_sensor, env_push, env_target)
DEFAULTS = env_params.ADR_DEFAULTS
assert NAMES == env_sensor.DRAW_NAMES + env_push.DRAW_NAMES + env_target.DRAW_NAMES


def place_of(name):
    """``(group, row, own name)`` of a draw name: whose table its row lies in, which row, and its key in that observer's
    mapping."""
    for group, module in enumerate(_MODULES):
        if name in module.DRAW_NAMES:
            row = module.DRAW_NAMES.index(name)
            return group, row, module.NAMES[row]
    raise KeyError(name)


# ---- configuration
def draw_adr_config(env_cfg, sensor_cfg, push_cfg, target_cfg, multi_gpu=False):
    """The checked ``task.env.ENV_DRAW_ADR`` of the ``task.env`` mapping as plain numbers, ``None`` when it is empty (off):
    ``{"NAMES": {DRAW NAME: {"START": [lo, hi], "STEP": s}}`` (in slot order), ``"LIMITS": {DRAW NAME: [lo, hi]}``,
    ``"BOUNDARY_FRACTION"``, ``"QUEUE"``, ``"WIDEN_AT"``, ``"NARROW_AT"``, ``"HISTORY_CAPACITY"}``.  ``sensor_cfg`` / ``push_cfg``
    / ``target_cfg``: the checked mappings of the three observers (``sensor_config`` ..), ``None`` for one that is off.
    ``ConfigError``, naming the key, for everything include/vine_env_draw_adr.h refuses and for ``multi_gpu``."""
    adr = env_cfg.get("ENV_DRAW_ADR") or {}
    if not hasattr(adr, "keys"):
        raise ConfigError("%s must be a mapping, not %r" % (_KEY, adr))
    if not len(adr):
        return None
    unknown = sorted(str(k) for k in set(adr.keys()) - set(DEFAULTS) - {"NAMES"})
    if unknown:
        raise ConfigError("%s: unknown key(s) %s" % (_KEY, ", ".join(unknown)))
    if multi_gpu:
        raise ConfigError("%s with multi_gpu=True: every rank would grow its own ranges" % _KEY)
    names = adr.get("NAMES") or {}
    if not hasattr(names, "keys") or not len(names):
        raise ConfigError("%s.NAMES must map at least one draw name of ENV_SENSOR, ENV_PUSH or ENV_TARGET to {START: [lo, hi], "
                          "STEP: s}" % _KEY)
    observers = (sensor_cfg, push_cfg, target_cfg)
    out = {"NAMES": {}, "LIMITS": {}}
    for name in NAMES:
        if name not in names:
            continue
        entry, where = names[name], "%s.NAMES.%s" % (_KEY, name)
        group, _, own = place_of(name)
        if observers[group] is None:
            raise ConfigError("%s needs task.env.%s: the name is one of its draws, and it is off" % (where, GROUPS[group]))
        if not observers[group]["PER_EPISODE"]:
            raise ConfigError("%s needs task.env.%s.PER_EPISODE: the range is the one the name is redrawn from" % (where, GROUPS[group]))
        form = observers[group][own]
        if not isinstance(form, list):
            raise ConfigError("%s: the name must be a [lo, hi] range in task.env.%s.%s, its limits" % (where, GROUPS[group], own))
        if not hasattr(entry, "keys") or sorted(entry.keys()) != ["START", "STEP"]:
            raise ConfigError("%s must hold START and STEP" % where)
        start = entry["START"]
        if not isinstance(start, (list, tuple)) or len(start) != 2:
            raise ConfigError("%s.START is [lo, hi], not %r" % (where, start))
        lo, hi = (named_draw.number(where + ".START", v, finite=False) for v in start)
        step = named_draw.number(where + ".STEP", entry["STEP"], finite=False)
        if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
            raise ConfigError("%s.START: lo > hi in [%g, %g]" % (where, lo, hi))
        if lo < form[0] or hi > form[1]:
            raise ConfigError("%s.START [%g, %g] lies outside the limits [%g, %g]" % (where, lo, hi, form[0], form[1]))
        if not np.isfinite(step) or not step > 0.0:
            raise ConfigError("%s.STEP must be positive, not %g" % (where, step))
        if name in INTEGER and (lo != np.floor(lo) or hi != np.floor(hi) or step != np.floor(step)):
            raise ConfigError("%s: an integer parameter takes an integer START and STEP" % where)
        if max(lo - form[0], form[1] - hi) / step > 2.0 ** 30:
            raise ConfigError("%s: more than 2^30 STEPs between START and a limit" % where)
        out["NAMES"][name] = {"START": [lo, hi], "STEP": step}
        out["LIMITS"][name] = [float(form[0]), float(form[1])]
    stray = sorted(str(k) for k in set(names.keys()) - set(out["NAMES"]))
    if stray:
        raise ConfigError("%s.NAMES.%s: unknown draw name (known: %s)" % (_KEY, stray[0], ", ".join(NAMES)))
    for key, default in DEFAULTS.items():
        out[key] = named_draw.number("%s.%s" % (_KEY, key), adr.get(key, default), finite=False)
    if not 0.0 <= out["BOUNDARY_FRACTION"] < 1.0:
        raise ConfigError("%s.BOUNDARY_FRACTION must lie in [0, 1), not %g" % (_KEY, out["BOUNDARY_FRACTION"]))
    for key in ("QUEUE", "HISTORY_CAPACITY"):
        if out[key] != np.floor(out[key]) or out[key] < 1:
            raise ConfigError("%s.%s must be an integer >= 1, not %g" % (_KEY, key, out[key]))
        out[key] = int(out[key])
    if not (np.isfinite(out["WIDEN_AT"]) and np.isfinite(out["NARROW_AT"])) or out["NARROW_AT"] >= out["WIDEN_AT"]:
        raise ConfigError("%s.NARROW_AT (%g) must be below WIDEN_AT (%g)" % (_KEY, out["NARROW_AT"], out["WIDEN_AT"]))
    return out


def draw_adr_names(adr):
    """``abi.VineEnvAdrName * VDA_NAMES`` of ``draw_adr_config``'s result."""
    names = (abi.VineEnvAdrName * abi.VDA_NAMES)()
    for name, a in adr["NAMES"].items():
        nm = names[NAMES.index(name)]
        nm.on, nm.start_lo, nm.start_hi, nm.step = 1, a["START"][0], a["START"][1], a["STEP"]
    return names


def draw_adr_spec(lib, vcfg, adr, sensor_spec=None, push_spec=None, target_spec=None):
    """``vine_env_draw_adr_spec``: the checked ``abi.VineEnvDrawAdrSpec`` of ``draw_adr_config``'s result and the three
    observers' checked specs (``None``: the observer is off).  ``ValueError`` with the library's text for a refusal."""
    out = abi.VineEnvDrawAdrSpec()
    rc = lib.vine_env_draw_adr_spec(C.byref(vcfg), *[C.byref(s) if s is not None else None for s in (sensor_spec, push_spec, target_spec)],
                                    draw_adr_names(adr), float(adr["BOUNDARY_FRACTION"]), int(adr["QUEUE"]), float(adr["WIDEN_AT"]),
                                    float(adr["NARROW_AT"]), int(adr["HISTORY_CAPACITY"]), C.byref(out))
    if rc != abi.OK:
        raise ValueError("ENV_DRAW_ADR: %s" % lib.vine_last_error().decode(errors="replace"))
    return out


# ---- the ranges
def draw_adr_max_widen(adr):
    """int64 [9, 2]: the steps between START and the limit per boundary, as ``env_params.adr_max_widen`` forms them (one more
    where the rounded quotient would leave the last step short of the limit); 0 for a name that is not under ADR."""
    out = np.zeros((len(NAMES), 2), dtype=np.int64)
    for name, a in adr["NAMES"].items():
        s, limits = NAMES.index(name), adr["LIMITS"][name]
        lo, hi, step = np.float64(a["START"][0]), np.float64(a["START"][1]), np.float64(a["STEP"])
        m_lo, m_hi = np.ceil((lo - limits[0]) / step), np.ceil((limits[1] - hi) / step)
        out[s, 0] = int(m_lo) + (1 if lo - m_lo * step > limits[0] else 0)
        out[s, 1] = int(m_hi) + (1 if hi + m_hi * step < limits[1] else 0)
    return out


def draw_adr_ranges(adr, widen):
    """``{DRAW NAME: (lo, hi)}`` in force under ``widen`` (int [9, 2]): ``lo = max(limit_lo, start_lo - widen_lo * step)``,
    ``hi = min(limit_hi, start_hi + widen_hi * step)``, one multiply and one add in float64, as the device forms them."""
    widen = np.asarray(widen, dtype=np.int64).reshape(len(NAMES), 2)
    out = {}
    for name, a in adr["NAMES"].items():
        s, limits, step = NAMES.index(name), adr["LIMITS"][name], np.float64(a["STEP"])
        lo = max(np.float64(limits[0]), np.float64(a["START"][0]) - np.float64(widen[s, 0]) * step)
        hi = min(np.float64(limits[1]), np.float64(a["START"][1]) + np.float64(widen[s, 1]) * step)
        out[name] = (float(lo), float(hi))
    return out


def draw_adr_draw(adr, seed, gids, episodes, widen):
    """What the redraw launch draws for ``(global env id, episode >= 1)`` pairs under ``widen``: ``(drawn, probe)`` with
    ``drawn`` draw name -> float64 [M] for the names under ADR (a probing episode's name set to exactly its boundary) and
    ``probe`` int64 [M], the boundary ``2 * slot + side`` or -1.  Episode 0 probes nothing."""
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    k = np.broadcast_to(np.asarray(episodes, dtype=np.int64), gids.shape)
    ranges = draw_adr_ranges(adr, widen)
    forms = [(name, [lo, hi]) for name, (lo, hi) in ranges.items()]
    values = named_draw.draw(forms, seed, gids, k, INTEGER, who="draw_adr_draw")
    slots = np.asarray([NAMES.index(name) for name in adr["NAMES"]], dtype=np.int64)
    count = 2 * len(slots)
    u_p = named_draw.uniform01_episode(seed, "DRAW_ADR_PROBE", gids, k)
    u_w = named_draw.uniform01_episode(seed, "DRAW_ADR_WHICH", gids, k)
    j = np.minimum(np.floor(u_w * float(count)).astype(np.int64), count - 1)
    probe = np.where((u_p < adr["BOUNDARY_FRACTION"]) & (k > 0), 2 * slots[j >> 1] + (j & 1), -1)
    drawn = {}
    for i, (name, (lo, hi)) in enumerate(ranges.items()):
        s = NAMES.index(name)
        drawn[name] = np.where(probe == 2 * s, lo, np.where(probe == 2 * s + 1, hi, values[i]))
    return drawn, probe


def start_ranges(adr):
    """``{DRAW NAME: [lo, hi]}``: START of every name under ADR, what episode 0 is drawn from."""
    return {name: list(a["START"]) for name, a in adr["NAMES"].items()}


def start_rows(adr, seed, gids):
    """``{DRAW NAME: float32 [N]}``: episode 0's draw from START, the rows the tables of the names under ADR begin with."""
    forms = [(name, list(a["START"])) for name, a in adr["NAMES"].items()]
    values = named_draw.draw(forms, seed, gids, 0, INTEGER, who="start_rows").astype(np.float32)
    return {name: values[i] for i, (name, _) in enumerate(forms)}


# ---- the two launches, in numpy
def draw_adr_replay(adr, seed, gids, resets, reached_flags, tables, observers=(None, None, None), step_index=None, widen0=None):
    """Both launches of ``vine_env_draw_adr_scheduled`` on the host, step by step, in float64 and integers, together with the
    per-episode tails of the three observers in front of them.  ``adr``: ``draw_adr_config``'s result; ``gids`` [N]: global env
    ids; ``resets`` and ``reached_flags`` [T, N]: the step's reset buffer and ``reward matrix[:, 2] != 0`` as the launches behind
    step t see them; ``tables``: three float32 arrays ``[rows, N]`` (or ``None``), the sensor's, the push's and the target's
    tables before the first step, the START rows already in them (``start_rows``); ``observers``: the three observers' checked
    mappings, ``None`` for one whose tail is not replayed (it is off, or the launches run alone); ``step_index`` [T]: what the
    history rows carry (default ``0 .. T - 1``); ``widen0`` [9, 2]: the ``widen`` in force before the first step.  Returns one
    dict per step, the state BEHIND that step's launches: ``widen`` [9, 2], ``counts`` [9, 2, 2], ``probe``, ``reached``,
    ``episode_index`` [N], ``tables`` (three arrays or ``None``), ``history`` [H, 4] (every row so far), ``cursor`` and
    ``consumed`` [9, 2, 2] (the counts decisions have cleared so far)."""
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    n = len(gids)
    resets = np.asarray(resets).reshape(-1, n) != 0
    flags = np.asarray(reached_flags).reshape(-1, n) != 0
    steps = np.arange(len(resets)) if step_index is None else np.asarray(step_index, dtype=np.int64)
    tables = [None if t is None else np.array(t, dtype=np.float32) for t in tables]
    max_widen = draw_adr_max_widen(adr)
    widen = np.zeros((len(NAMES), 2), dtype=np.int64) if widen0 is None else np.array(widen0, dtype=np.int64).reshape(len(NAMES), 2)
    counts = np.zeros((len(NAMES), 2, 2), dtype=np.int64)
    reached, probe = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    episode = np.zeros(n, dtype=np.int64)
    history, out, consumed = [], [], np.zeros_like(counts)
    for t in range(len(resets)):
        env_params.adr_decide(adr, max_widen, widen, counts, steps[t], history, consumed, slots=NAMES)
        reached |= flags[t]
        f = np.flatnonzero(resets[t])
        if len(f):
            probing = f[probe[f] >= 0]
            np.add.at(counts, (probe[probing] >> 1, probe[probing] & 1, 0), 1)
            np.add.at(counts, (probe[probing] >> 1, probe[probing] & 1, 1), reached[probing])
            reached[f] = 0
            episode[f] += 1
            tables = [None if tb is None else tb.copy() for tb in tables]
            for module, spec, tb in zip(_MODULES, observers, tables):      # the observers' own tails: every row, from the limits
                if spec is not None and spec["PER_EPISODE"] and tb is not None:
                    tb[:, f] = named_draw.draw(named_draw.named(module.NAMES, module.DRAW_NAMES, spec), seed, gids[f], episode[f],
                                               INTEGER).astype(np.float32)
            drawn, probe[f] = draw_adr_draw(adr, seed, gids[f], episode[f], widen)
            for name, v in drawn.items():
                group, row, _ = place_of(name)
                tables[group][row, f] = v.astype(np.float32)
        out.append({"widen": widen.copy(), "counts": counts.copy(), "probe": probe.copy(), "reached": reached.copy(),
                    "episode_index": episode.copy(), "tables": tables,
                    "history": np.asarray(history, dtype=np.int64).reshape(-1, 4), "cursor": len(history),
                    "consumed": consumed.copy()})
    return out


# ---- the episode log's columns
def draw_adr_episode_params(adr, seed, gids, episodes, drawn_at, history, widen0=None):
    """The ``param_<NAME>`` value and the probe of M episodes, without a device: ``({DRAW NAME: float64 [M]}, probe int64
    [M])`` for the names under ADR.  ``drawn_at`` [M]: the index of the step whose launch drew the episode
    (``episodes.drawn_at``), -1 where it is unknown (then NaN and probe -2); episode 0 is START's draw and probes nothing
    (-1); ``history`` [H, 4]: complete; ``widen0``: as for ``env_params.adr_widen_at``."""
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    k = np.asarray(episodes, dtype=np.int64).reshape(-1)
    at = np.asarray(drawn_at, dtype=np.int64).reshape(-1)
    params = {name: np.full(len(gids), np.nan) for name in adr["NAMES"]}
    probe = np.full(len(gids), -2, dtype=np.int64)
    first = np.flatnonzero(k == 0)
    if len(first):
        for name, v in start_rows(adr, seed, gids[first]).items():
            params[name][first] = v
        probe[first] = -1
    later = np.flatnonzero((k > 0) & (at >= 0))
    if len(later):
        widen = env_params.adr_widen_at(history, at[later], widen0, num_slots=len(NAMES))
        states, inverse = np.unique(widen.reshape(len(later), -1), axis=0, return_inverse=True)
        for j, w in enumerate(states):
            rows = later[np.reshape(inverse, -1) == j]
            drawn, probe[rows] = draw_adr_draw(adr, seed, gids[rows], k[rows], w.reshape(len(NAMES), 2))
            for name, v in drawn.items():
                params[name][rows] = v.astype(np.float32)
    return params, probe


class EnvDrawAdr(StepObserver):
    """A step observer (the protocol: utils/observers.py) behind the target, the sensor and the push, whose rows it replaces
    for the envs the step has just flagged, and in front of the redraw / ``EnvAdr``."""

    def __init__(self, lib, handle, vcfg, adr, reset, sensor, push, target, device, logger=None):
        """``adr``: ``draw_adr_config``'s result; ``reset``: the step's buffer; ``sensor`` / ``push`` / ``target``: the
        ``EnvSensor``, ``EnvPush`` and ``EnvTarget`` of the same handle (``None``: off).  The rows of the names under ADR in
        their tables are overwritten with episode 0's draw from START.  A reward matrix must be bound to ``handle`` before the
        first step."""
        import logging
        import torch
        super().__init__()
        self.logger = logger or logging.getLogger(__name__)
        self.lib, self.handle, self.vcfg, self.device = lib, handle, vcfg, device
        self.adr, self.reset = adr, reset
        self.seed, self.env_id_offset = int(vcfg.seed), int(vcfg.env_id_offset)
        self.group_observers = (sensor, push, target)
        self.aspec = draw_adr_spec(lib, vcfg, adr, getattr(sensor, "sspec", None), getattr(push, "pspec", None),
                                   getattr(target, "tspec", None))
        n = int(reset.shape[0])
        self.num_envs = n
        gids = np.arange(n, dtype=np.int64) + self.env_id_offset
        for name, row in start_rows(adr, self.seed, gids).items():      # episode 0 is the host's, from START
            group, r, _ = place_of(name)
            self.group_observers[group].table[r].copy_(torch.as_tensor(row, device=device))
        self.tables = (C.c_void_p * abi.VDA_GROUPS)(*[o.table.data_ptr() if o is not None else None for o in self.group_observers])
        self._ints = torch.zeros(abi.VDA_NAMES * 6, dtype=torch.int32, device=device)      # widen, then counts: one copy reads both
        self.widen = self._ints[:abi.VDA_NAMES * 2].view(abi.VDA_NAMES, 2)
        self.counts = self._ints[abi.VDA_NAMES * 2:].view(abi.VDA_NAMES, 2, 2)
        self.widen0 = np.zeros((abi.VDA_NAMES, 2), dtype=np.int64)      # what was in force before the first step (a restored checkpoint's)
        self.reached = torch.zeros(n, dtype=torch.int32, device=device)
        self.probe = torch.full((n,), -1, dtype=torch.int32, device=device)
        self.episode_index = torch.zeros(n, dtype=torch.int32, device=device)
        self.capacity = int(adr["HISTORY_CAPACITY"])
        self.history = torch.zeros((self.capacity, abi.ENV_DRAW_ADR_HISTORY_WORDS), dtype=torch.int32, device=device)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=device)
        self.history_rows = np.zeros((0, abi.ENV_DRAW_ADR_HISTORY_WORDS), dtype=np.int64)      # every row harvested so far
        self.history_harvested = 0       # the cursor at the last harvest
        self.history_dropped = 0
        self._scalars = torch.zeros(abi.VDA_NAMES * 6, dtype=torch.int32).pin_memory()      # widen, then counts

    # -- the observer protocol ---------------------------------------------------------------------------------------------
    def enqueue(self, stream, actions=None):
        native.check(self.lib.vine_env_draw_adr_scheduled(
            self.handle, self.aspec, self.reset.data_ptr(), self.tables, None, self.widen.data_ptr(), self.counts.data_ptr(),
            self.reached.data_ptr(), self.probe.data_ptr(), self.episode_index.data_ptr(), self.history.data_ptr(),
            self.cursor.data_ptr(), stream), self.lib)

    def live_tensors(self):
        """A rolled-back pass has moved all of it; the tables it wrote are the three observers' live tensors.  The history
        ring is not among them: what the pass appends lies past the restored cursor, where later rows overwrite it."""
        return [self._ints, self.reached, self.probe, self.episode_index, self.cursor]

    def reset_envs(self, env_ids):
        """The envs were reset from outside the step: they keep their values and their episode ordinal, and that episode is
        no longer counted at a boundary."""
        self.reached[env_ids] = 0
        self.probe[env_ids] = -1

    # -- the history -------------------------------------------------------------------------------------------------------
    def harvest_history(self):
        """Copy the history rows appended since the last harvest (synchronises).  Returns the complete history [H, 4]."""
        import torch
        if torch.cuda.is_current_stream_capturing():
            return self.history_rows
        cursor = int(self.cursor.item())
        lost = max(0, cursor - self.history_harvested - self.capacity)
        if lost:
            self.history_dropped += lost
            self.logger.warning(f"ENV_DRAW_ADR: {lost} history rows were overwritten before they were harvested "
                                f"({self.history_dropped} in all): raise ENV_DRAW_ADR.HISTORY_CAPACITY")
        first = max(self.history_harvested, cursor - self.capacity)
        self.history_harvested = cursor
        if cursor > first:
            a, b = first % self.capacity, (cursor - 1) % self.capacity + 1
            rows = self.history[a:b] if a < b else torch.cat([self.history[a:], self.history[:b]])
            self.history_rows = np.concatenate([self.history_rows, rows.cpu().numpy().astype(np.int64)])
        return self.history_rows

    # -- which values ------------------------------------------------------------------------------------------------------
    def episode_params(self, envs, episodes, drawn_at):
        """``draw_adr_episode_params`` of local env indices ``envs``, from the history harvested so far; no device involved."""
        gids = np.asarray(envs, dtype=np.int64) + self.env_id_offset
        return draw_adr_episode_params(self.adr, self.seed, gids, episodes, drawn_at, self.history_rows, self.widen0)

    # -- what a trainer logs -----------------------------------------------------------------------------------------------
    def scalars(self):
        """``{"draw_adr/<NAME>_lo": .., "draw_adr/<NAME>_hi": .., "draw_adr/probing_reach_rate": ..}`` at this point of the
        current stream: one non-blocking copy of ``widen`` and ``counts`` into pinned memory and a wait for it, where the
        caller synchronises anyway.  The rate is that of the probing episodes now in the queues (absent while they are empty)."""
        import torch
        done = torch.cuda.Event()
        self._scalars.copy_(self._ints, non_blocking=True)
        done.record(torch.cuda.current_stream(self.device))
        done.synchronize()
        return scalars_of(self.adr, self._scalars.numpy())

    def state_dict(self):
        """What a checkpoint keeps: ``widen`` (synchronises)."""
        return {"widen": self.widen.cpu().numpy().astype(np.int64), "names": list(self.adr["NAMES"])}

    def load_state_dict(self, state):
        import torch
        widen = check_state(self.adr, state)
        if self.history_harvested or int(self.cursor.item()):
            raise RuntimeError("ENV_DRAW_ADR: a checkpoint's widen is restored before the first step, not into a run under way")
        self.widen.copy_(torch.as_tensor(widen, dtype=torch.int32))
        self.widen0 = widen.copy()           # the episode log's join starts from it: this run's history has no row for it


def scalars_of(adr, ints):
    """``EnvDrawAdr.scalars`` of a host copy of ``widen`` followed by ``counts`` (int [9 * 6])."""
    ints = np.asarray(ints).reshape(-1)
    widen = ints[:abi.VDA_NAMES * 2].reshape(abi.VDA_NAMES, 2)
    counts = ints[abi.VDA_NAMES * 2:].reshape(abi.VDA_NAMES, 2, 2)
    out = {}
    for name, (lo, hi) in draw_adr_ranges(adr, widen).items():
        out[f"draw_adr/{name}_lo"], out[f"draw_adr/{name}_hi"] = lo, hi
    if counts[..., 0].sum() > 0:
        out["draw_adr/probing_reach_rate"] = float(counts[..., 1].sum()) / float(counts[..., 0].sum())
    return out


def check_state(adr, state):
    """The ``widen`` int64 [9, 2] of a checkpoint's ``draw_adr`` entry; ``ValueError`` for one that does not fit ``adr``."""
    widen = np.asarray(state["widen"], dtype=np.int64)
    if widen.size != abi.VDA_NAMES * 2 or list(state.get("names", adr["NAMES"])) != list(adr["NAMES"]) or np.any(widen < 0) or \
            np.any(widen.reshape(abi.VDA_NAMES, 2) > draw_adr_max_widen(adr)):
        raise ValueError("ENV_DRAW_ADR: the checkpoint's widen does not fit this configuration's NAMES, START, STEP and limits")
    return widen.reshape(abi.VDA_NAMES, 2)
