"""MPC_TRACK on the host side: the predictive controller's samples see their plant's target move over the horizon.  The
semantics are stated once, in include/vine_mpc_track.h.  What is left for the host: the ``track=`` mapping (``track_config``),
the checked spec (``track_spec``), the numpy statement of the two launches every GPU test compares against, bit for bit
(``plan_replay``, ``node_replay``), and the controller that owns the path table and enqueues the launches
(``TrackingController``).

``track=`` maps

  ``PATH``   ``exact``: the planner knows the path as the plant's ``ENV_TARGET`` observer walks it -- anchor, offset, velocity,
             span, reflections: the upper bound.  ``linear``: it knows the current signed velocity only and extrapolates
             without reflections: what the policy is told through its target-velocity columns.  ``held``: the launches run and
             change nothing (the launches alone, for tests and measurements).

The plant must carry ``task.env.ENV_TARGET``; the model task never does (``mpc.FORCED``): the node moves the samples' targets
instead."""
import ctypes as C

import numpy as np

from .. import abi
from . import env_target, mpc
from .config import ConfigError

_KEY = "track"
PATHS = tuple(abi.MPC_TRACK_PATHS)                   # by abi.TRACK_EXACT / _LINEAR / _HELD


# ---- configuration
def track_config(spec):
    """The checked ``track=`` mapping: ``{"PATH": "exact" | "linear" | "held"}``.  ``ConfigError``, naming the key, for
    anything else."""
    if not hasattr(spec, "keys"):
        raise ConfigError("%s={PATH: exact | linear | held} must be a mapping, not %r" % (_KEY, spec))
    unknown = sorted(str(k) for k in set(spec.keys()) - {"PATH"})
    if unknown:
        raise ConfigError("%s: unknown key(s) %s" % (_KEY, ", ".join(unknown)))
    if "PATH" not in spec:
        raise ConfigError("%s.PATH is missing: one of %s" % (_KEY, ", ".join(PATHS)))
    path = spec["PATH"]
    if not isinstance(path, str) or path not in PATHS:
        raise ConfigError("%s.PATH must be one of %s, not %r" % (_KEY, ", ".join(PATHS), path))
    return {"PATH": path}


def path_kind(path):
    """``abi.TRACK_*`` of a path's name (or of the number itself)."""
    if isinstance(path, str):
        if path not in PATHS:
            raise ConfigError("%s.PATH must be one of %s, not %r" % (_KEY, ", ".join(PATHS), path))
        return PATHS.index(path)
    return int(path)


def track_spec(lib, plant_tspec, mcfg, path):
    """``vine_mpc_track_spec``: the checked ``abi.VineMpcTrackSpec`` of the plant's checked ``abi.VineEnvTargetSpec``, the
    controller's ``abi.VineMpcConfig`` and a path kind; ``ValueError`` with the library's text for a refusal."""
    out = abi.VineMpcTrackSpec()
    rc = lib.vine_mpc_track_spec(C.byref(plant_tspec), C.byref(mcfg), path_kind(path), C.byref(out))
    if rc != abi.OK:
        raise ValueError("MPC_TRACK: %s" % lib.vine_last_error().decode(errors="replace"))
    return out


# ---- the launches, in numpy
def _words(mode, ay, az, d0, c, s, oa, oc, ty, tz, depth):
    """Step 5 of include/vine_env_target.h: float32 ``(TY, TZ, DEPTH)`` of the offsets; a word the mode does not write is the
    caller's."""
    if mode == abi.TARGET_FREE:
        return ay + oa, az + oc, depth
    if mode == abi.TARGET_SHELF:
        return ay - oa, tz, d0 + oa
    return ay - oa * c, az - oa * s, d0 + oa


def plan_replay(mode, path, cdt, horizon, state, motion, table, fresh, plant_reset):
    """``vine_mpc_track_plan`` on the host, in float32, bit for bit.  ``mode``: ``abi.TARGET_*``; ``path``: a name of ``PATHS``
    or ``abi.TRACK_*``; ``cdt``: the plant spec's control period; ``state`` [VF_COUNT, M]: the plant's state block; ``motion``
    [VTM_COUNT, M], ``table`` [VTG_NAMES, M] and ``fresh`` [M]: the plant observer's; ``plant_reset`` [M]: the plant's reset
    buffer.  Returns ``{"path": float32 [M, H, 3], "live": uint8 [M], "reflected": bool [M, H]}`` -- ``reflected[p, k]``: entry k
    of a live plant lies behind a reflection the ``exact`` walk took between entries k - 1 and k."""
    f = abi
    mode, kind, H = int(mode), path_kind(path), int(horizon)
    cdt = np.float32(cdt)
    state = np.asarray(state, dtype=np.float32)
    motion = np.asarray(motion, dtype=np.float32)
    table = np.asarray(table, dtype=np.float32)
    M = state.shape[1]
    ty0, tz0, dp0 = state[f.VF_TARGET_Y].copy(), state[f.VF_TARGET_Z].copy(), state[f.VF_OBJ_DEPTH].copy()
    ay, az, d0, c, s, oa, oc, va, vc = (motion[r].copy() for r in range(f.VTM_COUNT))
    live = ((kind != f.TRACK_HELD) & (np.asarray(plant_reset).reshape(M) == 0) & (np.asarray(fresh).reshape(M) == 0)
            & ((va != 0) | (vc != 0)))
    out = np.empty((M, H, f.MPC_TRACK_WORDS), dtype=np.float32)
    reflected = np.zeros((M, H), dtype=bool)
    np_errors = np.seterr(all="ignore")
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = ty0, tz0, dp0
    for k in range(1, H):                                            # (a plant that is not live may hold anything: its lanes are dropped)
        if kind == f.TRACK_EXACT:
            oa, va, bounced = env_target.advance(oa, va, table[f.VTG_SPAN_ALONG], cdt)
            if mode == f.TARGET_FREE:
                oc, vc, bounced_across = env_target.advance(oc, vc, table[f.VTG_SPAN_ACROSS], cdt)
                bounced = bounced | bounced_across
            reflected[:, k] = bounced & live
        else:
            oa = oa + va * cdt                                       # float32: one multiply, one add
            if mode == f.TARGET_FREE:
                oc = oc + vc * cdt
        ty, tz, depth = _words(mode, ay, az, d0, c, s, oa, oc, ty0, tz0, dp0)
        out[:, k, 0] = np.where(live, ty, ty0)
        out[:, k, 1] = np.where(live, tz, tz0)
        out[:, k, 2] = np.where(live, depth, dp0)
    np.seterr(**np_errors)
    return {"path": out, "live": live.astype(np.uint8), "reflected": reflected}


def node_replay(mode, samples, k, state, alive, path, live):
    """``vine_mpc_track_scheduled`` on the host: the model's state block [VF_COUNT, M * K] behind the launch that finds
    ``k = c - window[0]``, ``alive`` [M * K] as the node of include/vine_mpc.h left it, and the plan's ``path`` [M, H, 3] and
    ``live`` [M].  Returns a new block; the argument is not written."""
    f = abi
    mode, K, k = int(mode), int(samples), int(k)
    out = np.array(state, dtype=np.float32, copy=True)
    path = np.asarray(path, dtype=np.float32)
    H = path.shape[1]
    if k < 1 or k > H - 1:
        return out
    plant = np.arange(out.shape[1]) // K
    e = np.flatnonzero((np.asarray(live).reshape(-1)[plant] != 0) & (np.asarray(alive).reshape(-1) != 0))
    out[f.VF_TARGET_Y, e] = path[plant[e], k, 0]
    if mode != f.TARGET_SHELF:
        out[f.VF_TARGET_Z, e] = path[plant[e], k, 1]
    if mode != f.TARGET_FREE:
        out[f.VF_OBJ_DEPTH, e] = path[plant[e], k, 2]
    return out


# ---- the device
class TrackingController(mpc.Controller):
    """``mpc.Controller`` whose samples follow their plant's moving target.  It owns ``path`` [M, H, 3] and ``live`` [M] and
    builds its spec from the plant's ``ENV_TARGET`` observer (``plant.env_target.tspec``).

    ``control_step()`` = ``plan()``, ``fork()``, H x (``model.step_into`` + ``node()`` + ``track_node()``), ``update()``, the
    plant step: still one linear chain in a captured graph.  ``launches`` gains ``"plan"`` and ``"track"``."""

    def __init__(self, plant_task, model_task, samples, track, horizon=mpc.DEFAULTS["horizon"], lam=mpc.DEFAULTS["lambda"],
                 sigma=mpc.DEFAULTS["sigma"], seed=mpc.DEFAULTS["seed"], graph=True, graph_steps=1, keep_weights=False):
        import torch
        self.track = track_config(track)
        observer = getattr(plant_task, "env_target", None)
        if observer is None:
            raise ConfigError("mpc: track= needs a plant with task.env.ENV_TARGET: there is no path to follow")
        super().__init__(plant_task, model_task, samples, horizon, lam, sigma, seed, graph=graph, graph_steps=graph_steps,
                         keep_weights=keep_weights)
        self.observer = observer
        self.kspec = track_spec(self.lib, observer.tspec, self.mcfg, self.track["PATH"])
        self.path = torch.zeros((self.M, self.H, abi.MPC_TRACK_WORDS), dtype=torch.float32, device=self.device)
        self.live = torch.zeros(self.M, dtype=torch.uint8, device=self.device)
        self.launches.update({"plan": 0, "track": 0})

    def tensors(self):
        return super().tensors() + [self.path, self.live]

    def plan(self):
        from .. import native
        p, o = self.plant, self.observer
        native.check(self.lib.vine_mpc_track_plan(
            p._handle, self.kspec, p.reset_buf.data_ptr(), o.fresh.data_ptr(), o.table.data_ptr(), o.motion.data_ptr(),
            self.path.data_ptr(), self.live.data_ptr(), self._stream()), self.lib)
        self.launches["plan"] += 1

    def track_node(self):
        from .. import native
        native.check(self.lib.vine_mpc_track_scheduled(
            self.model._handle, self.kspec, self.window.data_ptr(), self.alive.data_ptr(), self.path.data_ptr(),
            self.live.data_ptr(), self._stream()), self.lib)
        self.launches["track"] += 1

    def model_step(self):
        """One model step, the scoring node behind it and the target's next entry behind that."""
        super().model_step()
        self.track_node()

    def control_step(self):
        self.plan()
        super().control_step()


# ---- a run
class Play(mpc.PlayVariant):
    """``track=`` of ``mpc.play``."""
    report_params = True       # the plant's varying param_TARGET_* columns

    def check(self, run):
        self.spec = track_config(self.spec)

    def controller(self, run):
        import torch
        self.lived = torch.zeros((), dtype=torch.int64, device=run.plant.device)
        return TrackingController(run.plant, run.model, run.samples, self.spec, *run.planner, graph=run.graph)

    def banner(self, run):
        print("mpc: the samples' targets follow the %s path of their plant's ENV_TARGET" % self.spec["PATH"], flush=True)

    def stepped(self, ctl):
        self.lived += ctl.live.sum()

    def result(self, run, out):
        out["track"] = {"PATH": self.spec["PATH"], "live_fraction": float(self.lived) / max(1, run.steps * run.M)}
        print("mpc: tracked along the %s path on %.4g of the (plant, control step) pairs" % (
            self.spec["PATH"], out["track"]["live_fraction"]), flush=True)
