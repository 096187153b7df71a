"""ENV_TARGET on the host side: the configuration, the draw of an env's four target values, the numpy statement of the launch
behind every step (``target_replay``: what every GPU test compares against, bit for bit) and the step observer
(``EnvTarget``).  The semantics are stated once, in include/vine_env_target.h.

``task.env.ENV_TARGET`` (``{}``: off) maps

  ``VEL_ALONG``    the target's velocity in m/s, signed, along its path: +y in free space, the depth axis of the shelf or the
                   pipe with an obstacle (positive: deeper)
  ``VEL_ACROSS``   in free space the velocity along +z; constant zero with an obstacle
  ``SPAN_ALONG``   half-length in m of the path about where the reset put the target, >= 0; the target turns round at its ends
  ``SPAN_ACROSS``  likewise along +z
                   each a number, ``[lo, hi]`` or ``{values: [...]}``
  ``PER_EPISODE``  False: every env's four values are drawn once and held; True: redrawn on the device at every reset

What env ``g`` gets in episode ``k`` is the named draw (utils/named_draw.py) under the names ``TARGET_VEL_ALONG`` .. ``TARGET_SPAN_ACROSS``,
keyed by the GLOBAL env id: a rank's shard draws what the whole batch would."""
import ctypes as C

import numpy as np

from .. import abi, native
from . import named_draw
from .config import ConfigError
from .named_draw import candidates
from .observers import FirstFrameObserver

_KEY = "task.env.ENV_TARGET"
NAMES = tuple(abi.ENV_TARGET_NAMES)                  # the table's rows, the order of the mixed radix
DRAW_NAMES = tuple("TARGET_" + n for n in NAMES)     # the names the draw is keyed by, and of the log's param_ columns
MODES = ("free space", "shelf", "pipe")              # by abi.TARGET_FREE / _SHELF / _PIPE


# ---- configuration
def control_period(sim_dt, control_freq_inv):
    """float32 ``dt * controlFrequencyInv`` as the step kernels form it."""
    return np.float32(sim_dt) * np.float32(int(control_freq_inv))


def mode_of(env_cfg):
    """``abi.TARGET_*`` of the ``task.env`` mapping's obstacle keys; ``ConfigError`` for both obstacles at once."""
    shelf, pipe = bool(env_cfg.get("CREATE_SHELF", False)), bool(env_cfg.get("CREATE_PIPE", False))
    if shelf and pipe:
        raise ConfigError("%s: CREATE_SHELF together with CREATE_PIPE: the depth is the pipe's, the shelf would not follow the "
                          "target" % _KEY)
    return abi.TARGET_PIPE if pipe else abi.TARGET_SHELF if shelf else abi.TARGET_FREE


def target_config(env_cfg, cdt):
    """The checked ``task.env.ENV_TARGET`` of the ``task.env`` mapping as plain numbers and lists, ``None`` when it is empty
    (off): ``{"VEL_ALONG", "VEL_ACROSS", "SPAN_ALONG", "SPAN_ACROSS"`` (a number, ``[lo, hi]`` or ``{"values": [..]}``),
    ``"PER_EPISODE"``, ``"MODE"`` (``abi.TARGET_*``, from the obstacle keys)``}``.  ``cdt``: ``control_period`` of the
    configuration.  ``ConfigError``, naming the key, for everything include/vine_env_target.h refuses."""
    cfg = env_cfg.get("ENV_TARGET") or {}
    if not hasattr(cfg, "keys"):
        raise ConfigError("%s must be a mapping, not %r" % (_KEY, cfg))
    if not len(cfg):
        return None
    unknown = sorted(set(cfg.keys()) - set(NAMES) - {"PER_EPISODE"})
    if unknown:
        raise ConfigError("%s: unknown key(s) %s" % (_KEY, ", ".join(str(k) for k in unknown)))
    out = {}
    for name in NAMES:
        out[name] = named_draw.form("%s.%s" % (_KEY, name), cfg.get(name, 0))
        for v in candidates(out[name]):
            if name.startswith("SPAN") and not v >= 0.0:
                raise ConfigError("%s.%s: %g is negative" % (_KEY, name, v))
            if abs(v) > float(np.finfo(np.float32).max):
                raise ConfigError("%s.%s: %g does not fit a float32" % (_KEY, name, v))
    out["PER_EPISODE"] = named_draw.flag("%s.PER_EPISODE" % _KEY, cfg.get("PER_EPISODE", False))
    out["MODE"] = int(mode_of(env_cfg))
    if float(env_cfg.get("VELOCITY_SUCCESS_REWARD_WEIGHT", 0)) != 0.0:
        raise ConfigError("%s: task.env.VELOCITY_SUCCESS_REWARD_WEIGHT must be 0: the step's term assumes a resting target" % _KEY)
    largest = {n: max(abs(np.float32(v)) for v in candidates(out[n])) for n in NAMES}
    if out["MODE"] != abi.TARGET_FREE:
        for name in ("VEL_ACROSS", "SPAN_ACROSS"):
            if largest[name] != 0.0:
                raise ConfigError("%s.%s must be constant zero with an obstacle (%s): the target moves along its depth axis only"
                                  % (_KEY, name, MODES[out["MODE"]]))
    cdt = np.float32(cdt)
    if not (np.isfinite(cdt) and cdt > 0):
        raise ConfigError("%s: the control period must be positive, not %r" % (_KEY, cdt))
    for axis in ("ALONG", "ACROSS"):
        if largest["VEL_" + axis] == 0.0:
            continue
        room = min(np.float32(v) for v in candidates(out["SPAN_" + axis]))
        if np.float32(largest["VEL_" + axis]) * cdt > np.float32(2.0) * room or not room > 0.0:
            raise ConfigError("%s.VEL_%s: max|VEL| * cdt = %g exceeds 2 * min SPAN_%s = %g: one reflection would not keep the "
                              "target on its path" % (_KEY, axis, np.float32(largest["VEL_" + axis]) * cdt, axis, 2.0 * room))
    if largest["VEL_ALONG"] == 0.0 and largest["VEL_ACROSS"] == 0.0 and not out["PER_EPISODE"]:
        raise ConfigError("%s: VEL_ALONG and VEL_ACROSS are both constant zero: nothing to do" % _KEY)
    return out


def varying_names(spec):
    """The names of ``NAMES`` whose value can differ between envs or episodes."""
    return named_draw.varying(NAMES, spec)


# ---- the draw
def draw_target(spec, seed, gids, episodes):
    """float64 [4, M]: the four values of M ``(global env id, episode)`` pairs: ``named_draw.draw``, the host's statement of
    ``redraw_value`` (csrc/vine_named_draw.h)."""
    return named_draw.draw(named_draw.named(NAMES, DRAW_NAMES, spec), seed, gids, episodes, who="draw_target")


def target_names(spec):
    """``(abi.VineEnvRedrawName * VTG_NAMES, values float64 [V])`` of a spec."""
    return named_draw.pack(named_draw.named(NAMES, DRAW_NAMES, spec))


def target_spec(lib, vcfg, spec, device_values=None):
    """``vine_env_target_spec``: the checked ``abi.VineEnvTargetSpec``; ``ValueError`` with the library's text for a refusal."""
    names, values = target_names(spec)
    out = abi.VineEnvTargetSpec()
    rc = lib.vine_env_target_spec(C.byref(vcfg), names, values.ctypes.data if len(values) else None,
                                  device_values if len(values) else None, len(values), int(spec["PER_EPISODE"]), C.byref(out))
    if rc != abi.OK:
        raise ValueError("ENV_TARGET: %s" % lib.vine_last_error().decode(errors="replace"))
    return out


# ---- the launch, in numpy
def layout_of(tspec):
    """What ``target_replay`` needs of a checked ``abi.VineEnvTargetSpec``: ``{"mode", "vel_column" (-1: none), "inv_obs_scale"
    float32 [2], "clip" float32, "cdt" float32}``."""
    return {"mode": int(tspec.mode), "vel_column": int(tspec.vel_column),
            "inv_obs_scale": np.asarray(list(tspec.inv_obs_scale), dtype=np.float32),
            "clip": np.float32(tspec.clip_observations), "cdt": np.float32(tspec.cdt)}


def _advance(off, vel, span, cdt):
    """One control step along an axis, reflected at its ends: float32 ``(off, vel, reflected)``."""
    n = off + vel * cdt                                             # float32: one multiply, one add
    over, under = n > span, n < -span
    n = np.where(over, span - (n - span), np.where(under, -span - (n + span), n))
    return n.astype(np.float32), np.where(over | under, -vel, vel).astype(np.float32), over | under


advance = _advance                    # the one statement of the path step, for utils/mpc_track.py plan_replay too


def target_replay(spec, seed, gids, layout, state, obs, progress, resets, axis=None, external_resets=None, table=None):
    """The launch behind T steps, on the host, in float32, bit for bit.  ``spec``: ``target_config``'s result; ``gids`` [N]:
    global env ids; ``layout``: ``layout_of``'s result (or the same keys by hand); ``state`` [T, VF_COUNT, N] float32: the state
    block as each launch finds it; ``obs`` [T, N, num_obs] float32: what the step wrote; ``progress`` and ``resets`` [T, N]: the
    step's buffers as the launch sees them; ``axis``: ``None`` (float64 ``cos`` / ``sin`` of the stored angle, rounded once) or
    [T, 2, N] float32, the device's AXIS rows behind each launch -- ``sincosf`` is the one statement numpy does not reproduce
    in every bit, and an env's axis is read from ``axis[t]`` at the launch that takes it; ``external_resets``: ``None`` or a
    sequence [T] of env-index lists reset from outside BEFORE step t (``EnvTarget.reset_envs``); ``table``: the float32 [4, N]
    table in force before the first step (default: episode 0's draw).  Returns one dict per step, what lies BEHIND that step's
    launch: ``state`` [VF_COUNT, N], ``obs`` [N, num_obs], ``table`` [4, N], ``motion`` [VTM_COUNT, N], ``fresh`` [N] uint8,
    ``episode_index`` [N], ``first``, ``moving`` and ``reflected`` [N] bool."""
    f = abi
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    n = len(gids)
    state = np.asarray(state, dtype=np.float32)
    obs = np.asarray(obs, dtype=np.float32)
    progress = np.asarray(progress).reshape(len(state), n)
    resets = np.asarray(resets).reshape(len(state), n) != 0
    mode, col = int(layout["mode"]), int(layout["vel_column"])
    inv = np.asarray(layout["inv_obs_scale"], dtype=np.float32)
    clip, cdt = np.float32(layout["clip"]), np.float32(layout["cdt"])
    table = (draw_target(spec, seed, gids, 0).astype(np.float32) if table is None
             else np.array(table, dtype=np.float32).reshape(len(NAMES), n))
    motion = np.zeros((f.VTM_COUNT, n), dtype=np.float32)
    fresh = np.ones(n, dtype=np.uint8)
    episode = np.zeros(n, dtype=np.int64)
    out = []
    for t in range(len(state)):
        if external_resets is not None and len(external_resets[t]):
            fresh[np.asarray(external_resets[t], dtype=np.int64)] = 1
        st, ob = state[t].copy(), obs[t].copy()
        motion = motion.copy()
        first = (progress[t] == 0) | (fresh != 0)
        i = np.flatnonzero(first)
        motion[f.VTM_ANCHOR_Y, i], motion[f.VTM_ANCHOR_Z, i] = st[f.VF_TARGET_Y, i], st[f.VF_TARGET_Z, i]
        motion[f.VTM_DEPTH0, i] = st[f.VF_OBJ_DEPTH, i] if mode != f.TARGET_FREE else np.float32(0)
        if mode == f.TARGET_PIPE:
            if axis is None:
                angle = st[f.VF_OBJ_ANGLE, i].astype(np.float64)
                motion[f.VTM_AXIS_C, i], motion[f.VTM_AXIS_S, i] = np.cos(angle), np.sin(angle)
            else:
                motion[f.VTM_AXIS_C, i], motion[f.VTM_AXIS_S, i] = np.asarray(axis[t], dtype=np.float32)[:, i]
        else:
            motion[f.VTM_AXIS_C, i], motion[f.VTM_AXIS_S, i] = np.float32(1), np.float32(0)
        motion[f.VTM_OFF_ALONG, i] = motion[f.VTM_OFF_ACROSS, i] = np.float32(0)
        motion[f.VTM_VEL_ALONG, i], motion[f.VTM_VEL_ACROSS, i] = table[f.VTG_VEL_ALONG, i], table[f.VTG_VEL_ACROSS, i]
        fresh = np.zeros(n, dtype=np.uint8)

        ay, az, d0, c, s, oa, oc, va, vc = (motion[r].copy() for r in range(f.VTM_COUNT))
        moving = (va != 0) | (vc != 0)
        m = np.flatnonzero(moving)
        if col >= 0 and len(m):
            if mode == f.TARGET_FREE:
                wy, wz = va, vc
            elif mode == f.TARGET_SHELF:
                wy, wz = -va, np.zeros(n, dtype=np.float32)
            else:
                wy, wz = (-va) * c, (-va) * s
            for j, w in ((0, wy), (1, wz)):
                x = ob[m, col + j] + w[m] * inv[j]                  # float32: one multiply, one add
                ob[m, col + j] = np.minimum(np.maximum(x, -clip), clip)
        oa_n, va_n, reflected = _advance(oa, va, table[f.VTG_SPAN_ALONG], cdt)
        if mode == f.TARGET_FREE:
            oc_n, vc_n, reflected_across = _advance(oc, vc, table[f.VTG_SPAN_ACROSS], cdt)
            reflected = reflected | reflected_across
        else:
            oc_n, vc_n = oc, vc
        for row, new in ((f.VTM_OFF_ALONG, oa_n), (f.VTM_OFF_ACROSS, oc_n), (f.VTM_VEL_ALONG, va_n), (f.VTM_VEL_ACROSS, vc_n)):
            motion[row, m] = new[m]
        oa, oc = motion[f.VTM_OFF_ALONG], motion[f.VTM_OFF_ACROSS]
        if mode == f.TARGET_FREE:
            st[f.VF_TARGET_Y, m], st[f.VF_TARGET_Z, m] = (ay + oa)[m], (az + oc)[m]
        elif mode == f.TARGET_SHELF:
            st[f.VF_TARGET_Y, m], st[f.VF_OBJ_DEPTH, m] = (ay - oa)[m], (d0 + oa)[m]
        else:
            st[f.VF_TARGET_Y, m], st[f.VF_TARGET_Z, m] = (ay - oa * c)[m], (az - oa * s)[m]
            st[f.VF_OBJ_DEPTH, m] = (d0 + oa)[m]
        if spec["PER_EPISODE"]:
            r = np.flatnonzero(resets[t])
            if len(r):
                episode = episode.copy()
                episode[r] += 1
                table = table.copy()
                table[:, r] = draw_target(spec, seed, gids[r], episode[r]).astype(np.float32)
        out.append({"state": st, "obs": ob, "table": table, "motion": motion, "fresh": fresh.copy(),
                    "episode_index": episode.copy(), "first": first, "moving": moving, "reflected": reflected & moving})
    return out


# ---- the episode log's columns
def episode_params(spec, seed, gids, episodes):
    """``{"TARGET_<NAME>": float32 [M]}`` of the names that vary: ``named_draw.episode_params``."""
    return named_draw.episode_params(NAMES, DRAW_NAMES, spec, seed, gids, episodes)


class EnvTarget(FirstFrameObserver):
    """A step observer (the protocol: utils/observers.py) that moves each env's target in the state block the step reads and
    adds the target's velocity to the observation the step has just written (``wants_obs``).  In launch order it stands
    behind the video, the recorder and the episode log and in front of ``EnvSensor``.  The path is a function of the env's
    own state, not of the step count."""

    wants_obs = True
    NAMES, DRAW_NAMES = NAMES, DRAW_NAMES

    def __init__(self, lib, handle, vcfg, spec, reset, progress, num_envs, num_obs, device):
        """``spec``: ``target_config``'s result; ``reset`` / ``progress``: the step's buffers."""
        import torch
        super().__init__(lib, handle, vcfg, spec, num_envs, device)
        self.num_obs = int(num_obs)
        self.reset, self.progress = reset, progress
        self.tspec = target_spec(lib, vcfg, spec, self.values_ptr)
        if self.tspec.num_obs != self.num_obs:
            raise ValueError("ENV_TARGET: the configuration has %d observation columns, the task %d" % (self.tspec.num_obs, self.num_obs))
        if self.tspec.mode != spec["MODE"]:
            raise ValueError("ENV_TARGET: the configuration's obstacle flags give mode %d, the spec %d" % (self.tspec.mode, spec["MODE"]))
        self.motion = torch.zeros((abi.VTM_COUNT, self.num_envs), dtype=torch.float32, device=device)
        self.anchor = self.motion[abi.VTM_ANCHOR_Y:abi.VTM_ANCHOR_Z + 1]       # views of the one block the launch takes
        self.depth0 = self.motion[abi.VTM_DEPTH0]
        self.axis = self.motion[abi.VTM_AXIS_C:abi.VTM_AXIS_S + 1]
        self.off = self.motion[abi.VTM_OFF_ALONG:abi.VTM_OFF_ACROSS + 1]
        self.vel = self.motion[abi.VTM_VEL_ALONG:abi.VTM_VEL_ACROSS + 1]

    def enqueue(self, stream, actions=None, obs=None):
        if obs is None:
            raise ValueError("EnvTarget.enqueue needs the observation buffer of the step it rides behind (obs=...)")
        native.check(self.lib.vine_env_target_scheduled(
            self.handle, self.tspec, int(obs), self.reset.data_ptr(), self.progress.data_ptr(), self.table.data_ptr(),
            self.motion.data_ptr(), self.fresh.data_ptr(), self.episode_index.data_ptr(), stream), self.lib)

    def live_tensors(self):
        """A rolled-back pass has moved offsets, flipped velocities, taken anchors, cleared ``fresh`` and, per episode, redrawn
        values and counted episodes: ``motion`` holds ``anchor``, ``depth0``, ``axis``, ``off`` and ``vel``.  The target it wrote
        is in the state block, which is the env's own live tensor."""
        return [self.motion, self.table, self.fresh, self.episode_index]
