"""ENV_SENSOR on the host side: the configuration, the draw of an env's three sensor values, the numpy statement of the
launch behind every step (``sensor_replay``: what every GPU test compares against, bit for bit) and the step observer
(``EnvSensor``).  The semantics are stated once, in include/vine_env_sensor.h.

``task.env.ENV_SENSOR`` (``{}``: off) maps

  ``DELAY``        whole control steps of sensing latency, integers 0 .. ``abi.SENSOR_MAX_DELAY``
  ``HOLD``         probability per step that no new frame arrives and the previous one stands, [0, 1)
  ``NOISE_STD``    amplitude of per-frame noise on the observation as the step wrote it, >= 0
                   each a number, ``[lo, hi]`` (for ``DELAY`` over the integers, both ends included) or ``{values: [...]}``
  ``COLUMNS``      ``all`` or a list of observation column indices the model applies to
  ``PER_EPISODE``  False: every env's three values are drawn once and held; True: redrawn on the device at every reset

What env ``g`` gets in episode ``k`` is the named draw (utils/named_draw.py) under the names ``SENSOR_DELAY``, ``SENSOR_HOLD``
and ``SENSOR_NOISE_STD``, keyed by the GLOBAL env id: a rank's shard draws what the whole batch would."""
import ctypes as C

import numpy as np

from .. import abi, native
from . import named_draw
from .config import ConfigError
from .named_draw import candidates, philox4x32_10
from .observers import FirstFrameObserver

_KEY = "task.env.ENV_SENSOR"
NAMES = tuple(abi.ENV_SENSOR_NAMES)                  # the table's rows, the order of the mixed radix
DRAW_NAMES = tuple("SENSOR_" + n for n in NAMES)     # the names the draw is keyed by, and of the log's param_ columns
INTEGER = ("SENSOR_DELAY",)                          # the draw names whose range is over the integers
SLOTS = abi.SENSOR_SLOTS
# the scale of the eight-uniform deviate, 1 / sqrt(32 * (65536^2 - 1) / 12), in float64
NOISE_SCALE = np.float64(1.0) / np.sqrt(np.float64(32.0) * (np.float64(65536.0) * np.float64(65536.0) - np.float64(1.0)) / np.float64(12.0))


# ---- configuration
def _check_values(name, form):
    where = "%s.%s" % (_KEY, name)
    for v in candidates(form):
        if name == "DELAY" and (v != np.floor(v) or not 0 <= v <= abi.SENSOR_MAX_DELAY):
            raise ConfigError("%s: %g is not an integer in 0 .. %d" % (where, v, abi.SENSOR_MAX_DELAY))
        if name == "HOLD" and not (v >= 0.0 and np.float32(v) < np.float32(1.0)):
            raise ConfigError("%s: %g lies outside [0, 1)" % (where, v))
        if name == "NOISE_STD" and not v >= 0.0:
            raise ConfigError("%s: %g is negative" % (where, v))


def sensor_config(env_cfg, num_obs):
    """The checked ``task.env.ENV_SENSOR`` of the ``task.env`` mapping as plain numbers and lists, ``None`` when it is empty
    (off): ``{"DELAY", "HOLD", "NOISE_STD"`` (a number, ``[lo, hi]`` or ``{"values": [..]}``), ``"COLUMNS"`` (ascending list of
    column indices), ``"PER_EPISODE"}``.  ``ConfigError``, naming the key, for everything include/vine_env_sensor.h refuses."""
    cfg = env_cfg.get("ENV_SENSOR") or {}
    if not hasattr(cfg, "keys"):
        raise ConfigError("%s must be a mapping, not %r" % (_KEY, cfg))
    if not len(cfg):
        return None
    unknown = sorted(set(cfg.keys()) - set(NAMES) - {"COLUMNS", "PER_EPISODE"})
    if unknown:
        raise ConfigError("%s: unknown key(s) %s" % (_KEY, ", ".join(str(k) for k in unknown)))
    out = {}
    for name in NAMES:
        out[name] = named_draw.form("%s.%s" % (_KEY, name), cfg.get(name, 0))
        _check_values(name, out[name])
    columns = cfg.get("COLUMNS", "all")
    num_obs = int(num_obs)
    if isinstance(columns, str):
        if columns != "all":
            raise ConfigError("%s.COLUMNS is 'all' or a list of column indices, not %r" % (_KEY, columns))
        columns = list(range(num_obs))
    elif not isinstance(columns, (list, tuple)) or len(columns) == 0:
        raise ConfigError("%s.COLUMNS is 'all' or a non-empty list of column indices, not %r" % (_KEY, columns))
    seen = set()
    for j in columns:
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)):
            raise ConfigError("%s.COLUMNS: %r is not a column index" % (_KEY, j))
        if not 0 <= j < num_obs:
            raise ConfigError("%s.COLUMNS: column %d lies outside [0, %d)" % (_KEY, j, num_obs))
        if j in seen:
            raise ConfigError("%s.COLUMNS: column %d is listed twice" % (_KEY, j))
        seen.add(int(j))
    out["COLUMNS"] = sorted(seen)
    out["PER_EPISODE"] = named_draw.flag("%s.PER_EPISODE" % _KEY, cfg.get("PER_EPISODE", False))
    if not out["PER_EPISODE"] and all(max(candidates(out[n])) == 0.0 for n in NAMES):
        raise ConfigError("%s: DELAY, HOLD and NOISE_STD are all constant zero: nothing to do" % _KEY)
    return out


def column_mask(spec):
    return int(sum(1 << int(j) for j in spec["COLUMNS"]))


def varying_names(spec):
    """The names of ``NAMES`` whose value can differ between envs or episodes."""
    return named_draw.varying(NAMES, spec)


# ---- the draw
def draw_sensor(spec, seed, gids, episodes):
    """float64 [3, M]: DELAY, HOLD and NOISE_STD of M ``(global env id, episode)`` pairs: ``named_draw.draw``, the host's
    statement of ``redraw_value`` (csrc/vine_named_draw.h)."""
    return named_draw.draw(named_draw.named(NAMES, DRAW_NAMES, spec), seed, gids, episodes, INTEGER, who="draw_sensor")


def sensor_names(spec):
    """``(abi.VineEnvRedrawName * VSN_NAMES, values float64 [V])`` of a spec."""
    return named_draw.pack(named_draw.named(NAMES, DRAW_NAMES, spec))


def sensor_spec(lib, vcfg, spec, device_values=None):
    """``vine_env_sensor_spec``: the checked ``abi.VineEnvSensorSpec``; ``ValueError`` with the library's text for a refusal."""
    names, values = sensor_names(spec)
    out = abi.VineEnvSensorSpec()
    rc = lib.vine_env_sensor_spec(C.byref(vcfg), names, values.ctypes.data if len(values) else None,
                                  device_values if len(values) else None, len(values), column_mask(spec),
                                  int(spec["PER_EPISODE"]), C.byref(out))
    if rc != abi.OK:
        raise ValueError("ENV_SENSOR: %s" % lib.vine_last_error().decode(errors="replace"))
    return out


# ---- the launch, in numpy
def noise_deviate(seed, gids, step, columns):
    """float32 [M, C]: the deviate z of global envs ``gids`` [M] in ``columns`` [C] behind step ``step``: ``2 * S - 524280``
    with S the sum of the eight 16-bit halves of the Philox call (exact in float32)."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)
    g = (np.asarray(gids, dtype=np.int64).reshape(-1, 1) & 0xFFFFFFFF)
    w = philox4x32_10(g, step & 0xFFFFFFFF, abi.SENSOR_RNG_NOISE | (((step >> 32) << 8) & 0xFFFFFFFF),
                      np.asarray(columns, dtype=np.int64).reshape(1, -1), seed & 0xFFFFFFFF, seed >> 32)
    total = sum((x & np.uint32(0xFFFF)).astype(np.int64) + (x >> np.uint32(16)).astype(np.int64) for x in w)
    return (2 * total - 524280).astype(np.float32)


def hold_uniform(seed, gids, step):
    """float32 [M]: u = (w >> 8) * 2^-24 of the hold stream behind step ``step``."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)
    g = np.asarray(gids, dtype=np.int64).reshape(-1) & 0xFFFFFFFF
    w = philox4x32_10(g, step & 0xFFFFFFFF, abi.SENSOR_RNG_HOLD | (((step >> 32) << 8) & 0xFFFFFFFF), 0, seed & 0xFFFFFFFF, seed >> 32)
    return (w[0] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def sensor_replay(spec, seed, gids, steps, raw_obs, progress, resets, external_resets=None, clip=np.inf, table=None):
    """The launch behind T steps, on the host.  ``spec``: ``sensor_config``'s result; ``gids`` [N]: global env ids; ``steps``
    [T]: the index of the step each launch rides behind; ``raw_obs`` [T, N, num_obs] float32: what the step wrote;
    ``progress`` and ``resets`` [T, N]: the step's buffers as the launch sees them; ``external_resets``: ``None`` or a sequence
    [T] of env-index lists reset from outside BEFORE step t (``EnvSensor.reset_envs``); ``clip``: clipObservations; ``table``:
    the float32 [3, N] table in force before the first step (default: episode 0's draw).  Returns one dict per step, the
    state BEHIND that step's launch: ``obs`` [N, num_obs] (delivered), ``ring`` [SLOTS, N, num_obs], ``table`` [3, N],
    ``fresh`` [N] uint8, ``episode_index`` [N], ``held`` [N] bool, ``first`` [N] bool."""
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    n = len(gids)
    raw = np.asarray(raw_obs, dtype=np.float32)
    num_obs = raw.shape[2]
    progress = np.asarray(progress).reshape(len(raw), n)
    resets = np.asarray(resets).reshape(len(raw), n) != 0
    mask = np.zeros(num_obs, dtype=bool)
    mask[list(spec["COLUMNS"])] = True
    cols = np.flatnonzero(mask)
    clip = np.float32(clip)
    table = (draw_sensor(spec, seed, gids, 0).astype(np.float32) if table is None else np.array(table, dtype=np.float32).reshape(3, n))
    ring = np.zeros((SLOTS, n, num_obs), dtype=np.float32)
    fresh = np.ones(n, dtype=np.uint8)
    episode = np.zeros(n, dtype=np.int64)
    out = []
    for t in range(len(raw)):
        if external_resets is not None and len(external_resets[t]):
            fresh[np.asarray(external_resets[t], dtype=np.int64)] = 1
        s = int(steps[t])
        d, p, std = table[0].astype(np.int64), table[1], table[2]
        frame = raw[t].copy()
        noisy = np.flatnonzero(std != 0)
        if len(noisy):
            c = (std[noisy].astype(np.float64) * NOISE_SCALE).astype(np.float32)
            z = noise_deviate(seed, gids[noisy], s, cols)
            x = raw[t][np.ix_(noisy, cols)] + z * c[:, None]                 # float32: one multiply, one add
            frame[np.ix_(noisy, cols)] = np.minimum(np.maximum(x, -clip), clip)
        first = (progress[t] == 0) | (fresh != 0)
        held = ~first & (hold_uniform(seed, gids, s) < p)
        cur, prev = s % SLOTS, (s - 1) % SLOTS
        pushed = np.where(held[:, None], ring[prev], frame)
        ring = ring.copy()
        ring[cur] = pushed
        ring[:, first] = frame[first][None]
        delivered = ring[(s - d) % SLOTS, np.arange(n)]
        delivered[first] = frame[first]
        obs = raw[t].copy()
        obs[:, mask] = delivered[:, mask]
        fresh = np.zeros(n, dtype=np.uint8)
        if spec["PER_EPISODE"]:
            f = np.flatnonzero(resets[t])
            if len(f):
                episode = episode.copy()
                episode[f] += 1
                table = table.copy()
                table[:, f] = draw_sensor(spec, seed, gids[f], episode[f]).astype(np.float32)
        out.append({"obs": obs, "ring": ring, "table": table, "fresh": fresh.copy(), "episode_index": episode.copy(),
                    "held": held, "first": first})
    return out


# ---- the episode log's columns
def episode_params(spec, seed, gids, episodes):
    """``{"SENSOR_<NAME>": float32 [M]}`` of the names that vary: ``named_draw.episode_params``."""
    return named_draw.episode_params(NAMES, DRAW_NAMES, spec, seed, gids, episodes, INTEGER)


class EnvSensor(FirstFrameObserver):
    """A step observer (the protocol: utils/observers.py) that asks for the observation buffer of the step it rides behind
    (``wants_obs``) and rewrites it in place.  In launch order it stands in front of ``EnvRedraw`` / ``EnvAdr``.  The ring's
    slots follow the device's count; a frame never leaves its episode."""

    wants_obs = True
    NAMES, DRAW_NAMES, INTEGER = NAMES, DRAW_NAMES, INTEGER

    def __init__(self, lib, handle, vcfg, spec, reset, progress, num_envs, num_obs, device):
        """``spec``: ``sensor_config``'s result; ``reset`` / ``progress``: the step's buffers."""
        import torch
        super().__init__(lib, handle, vcfg, spec, num_envs, device)
        self.num_obs = int(num_obs)
        self.reset, self.progress = reset, progress
        self.sspec = sensor_spec(lib, vcfg, spec, self.values_ptr)
        if self.sspec.num_obs != self.num_obs:
            raise ValueError("ENV_SENSOR: the configuration has %d observation columns, the task %d" % (self.sspec.num_obs, self.num_obs))
        self.ring = torch.zeros((SLOTS, self.num_envs, self.num_obs), dtype=torch.float32, device=device)

    def enqueue(self, stream, actions=None, obs=None):
        if obs is None:
            raise ValueError("EnvSensor.enqueue needs the observation buffer of the step it rides behind (obs=...)")
        native.check(self.lib.vine_env_sensor_scheduled(
            self.handle, self.sspec, int(obs), self.reset.data_ptr(), self.progress.data_ptr(), self.table.data_ptr(),
            self.ring.data_ptr(), self.fresh.data_ptr(), self.episode_index.data_ptr(), stream), self.lib)

    def live_tensors(self):
        """A rolled-back pass has pushed frames, cleared ``fresh`` and, per episode, redrawn values and counted episodes."""
        return [self.ring, self.table, self.fresh, self.episode_index]
