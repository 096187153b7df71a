"""MPC_OBSERVE on the host side: the predictive controller's sensing path.  The controller receives the state of each plant
some control steps late, with noise and dropped frames (``vine_mpc_observe_measure``), puts a model copy of the plant -- the
*predictor* task, M envs -- onto that measurement (``vine_mpc_observe_pin``), replays the actions it has sent since then
(``catchup`` predictor steps with ``vine_mpc_observe_catchup`` behind each) and forks its samples from the predicted "now".
The semantics are stated once, in include/vine_mpc_observe.h.  What is left for the host: the configuration
(``observe_config``, ``draw_observe``, ``observe_cconfig``), the numpy statements every GPU test compares against
(``measure_replay``, ``pin_replay``, ``catchup_schedule``) and the controller (``ObservingController``).

``observe=`` of ``mpc.play`` / ``mpc.py`` maps

  ``DELAY``        whole control steps of sensing latency, integers 0 .. ``abi.MAX_DELAY``
  ``HOLD``         probability per step that no new frame arrives and the previous one stands, [0, 1)
  ``NOISE_Q``      amplitude of per-frame noise on the six joint positions, >= 0
  ``NOISE_QD``     ... on the six joint velocities, >= 0
                   each a number, ``[lo, hi]`` (for ``DELAY`` over the integers, both ends included) or ``{values: [...]}``,
                   drawn once per plant with the sensor's draw under the keys ``OBSERVE_<NAME>``
  ``COMPENSATE``   True (default): the delivered frame is predicted forward through the model; False: it is planned from as is
  ``CATCHUP``      predictor steps per control step, the largest ``DELAY`` (default) .. ``abi.MAX_DELAY``"""
import copy

import numpy as np

from .. import abi
from . import env_sensor, named_draw
from .config import ConfigError
from .mpc import DEFAULTS as MPC_DEFAULTS
from .mpc import Controller, PlayVariant, make_task

_KEY = "mpc: observe"
NAMES = tuple(abi.MPC_OBSERVE_NAMES)                  # the table's rows, the order of the mixed radix
DRAW_NAMES = tuple("OBSERVE_" + n for n in NAMES)     # the names the draw is keyed by
INTEGER = ("OBSERVE_DELAY",)                          # the draw names whose range is over the integers
SLOTS, LOG = abi.MPC_OBSERVE_SLOTS, abi.MPC_OBSERVE_LOG
NOISE_SCALE = env_sensor.NOISE_SCALE
RING = slice(abi.VF_FIFO0, abi.VF_PIPE_Y)             # the fields of a column no frame holds
NOT_RING = np.array([f for f in range(abi.VF_COUNT) if not abi.VF_FIFO0 <= f < abi.VF_PIPE_Y])


# ---------------------------------------------------------------------------------------------------------- configuration
def _check_values(name, form):
    where = "%s.%s" % (_KEY, name)
    for v in named_draw.candidates(form):
        if name == "DELAY" and (v != np.floor(v) or not 0 <= v <= abi.MAX_DELAY):
            raise ConfigError("%s: %g is not an integer in 0 .. %d" % (where, v, abi.MAX_DELAY))
        if name == "HOLD" and not (v >= 0.0 and np.float32(v) < np.float32(1.0)):
            raise ConfigError("%s: %g lies outside [0, 1)" % (where, v))
        if name in ("NOISE_Q", "NOISE_QD") and not (v >= 0.0 and v <= float(np.finfo(np.float32).max)):
            raise ConfigError("%s: %g is negative (or does not fit a float32)" % (where, v))


def observe_config(spec):
    """The checked ``observe=`` mapping as plain numbers and lists: ``{"DELAY", "HOLD", "NOISE_Q", "NOISE_QD"`` (a number,
    ``[lo, hi]`` or ``{"values": [..]}``), ``"COMPENSATE"`` (bool), ``"CATCHUP"`` (int)``}``.  ``ConfigError``, naming the key,
    for every bad key or value -- a ``CATCHUP`` below the largest ``DELAY`` among them."""
    if not hasattr(spec, "keys"):
        raise ConfigError("%s={NAME: value, ...} must be a mapping, not %r" % (_KEY, spec))
    unknown = sorted(str(k) for k in set(spec.keys()) - set(NAMES) - {"COMPENSATE", "CATCHUP"})
    if unknown:
        raise ConfigError("%s: unknown key(s) %s" % (_KEY, ", ".join(unknown)))
    out = {}
    for name in NAMES:
        out[name] = named_draw.form("%s.%s" % (_KEY, name), spec.get(name, 0))
        _check_values(name, out[name])
    out["COMPENSATE"] = named_draw.flag("%s.COMPENSATE" % _KEY, spec.get("COMPENSATE", True))
    largest = int(max(named_draw.candidates(out["DELAY"])))
    catchup = spec.get("CATCHUP", largest)
    if isinstance(catchup, bool) or not isinstance(catchup, (int, np.integer)) or not 0 <= catchup <= abi.MAX_DELAY:
        raise ConfigError("%s.CATCHUP must be an integer in 0 .. %d, not %r" % (_KEY, abi.MAX_DELAY, catchup))
    if catchup < largest:
        raise ConfigError("%s.CATCHUP = %d lies below the largest DELAY, %d: the last frames could not be caught up with"
                          % (_KEY, catchup, largest))
    out["CATCHUP"] = int(catchup)
    return out


def draw_observe(spec, seed, gids):
    """float64 [4, M]: DELAY, HOLD, NOISE_Q and NOISE_QD of the plants with global ids ``gids``: episode 0 of
    ``named_draw.draw`` under the names ``OBSERVE_<NAME>``."""
    return named_draw.draw(named_draw.named(NAMES, DRAW_NAMES, spec), seed, gids, 0, INTEGER, who="draw_observe")


def observe_cconfig(num_plants, catchup=0, compensate=True, seed=0, table=None):
    """The checked ``abi.VineMpcObserveConfig``: what include/vine_mpc_observe.h refuses is refused here with a ``ConfigError``
    naming the key (``plants``, ``catchup``, ``compensate``, ``seed``), and -- the host's own -- a ``catchup`` below the
    largest ``DELAY`` of ``table`` ([4, M]) where one is given."""
    c = abi.VineMpcObserveConfig()
    c.abi_version = abi.MPC_OBSERVE_ABI_VERSION
    if isinstance(num_plants, bool) or not isinstance(num_plants, (int, np.integer)) or num_plants < 1:
        raise ConfigError("%s: plants must be an integer >= 1, not %r" % (_KEY, num_plants))
    c.num_plants = int(num_plants)
    if isinstance(catchup, bool) or not isinstance(catchup, (int, np.integer)) or not 0 <= catchup <= abi.MAX_DELAY:
        raise ConfigError("%s: catchup must be an integer in 0 .. %d, not %r" % (_KEY, abi.MAX_DELAY, catchup))
    c.catchup = int(catchup)
    if not isinstance(compensate, (bool, np.bool_)):
        raise ConfigError("%s: compensate must be a bool, not %r" % (_KEY, compensate))
    c.compensate = int(bool(compensate))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed <= 0xFFFFFFFFFFFFFFFF:
        raise ConfigError("%s: seed must be an integer in 0 .. 2^64 - 1, not %r" % (_KEY, seed))
    c.seed = int(seed)
    if table is not None:
        table = np.asarray(table)
        if table.shape != (len(NAMES), c.num_plants):
            raise ConfigError("%s: the table must be [%d, %d], not %s" % (_KEY, len(NAMES), c.num_plants, table.shape))
        largest = int(table[abi.VMO_DELAY].max())
        if c.catchup < largest:
            raise ConfigError("%s: catchup = %d lies below the table's largest DELAY, %d" % (_KEY, c.catchup, largest))
    return c


# ---------------------------------------------------------------------------------------------------- the launches, in numpy
def noise_deviate(seed, gids, step, fields):
    """float32 [M, F]: the deviate z of plants ``gids`` [M] in the counter words ``fields`` [F] (0 .. 5: q; 6 .. 11: qd) behind
    step ``step``: ``2 * S - 524280`` with S the sum of the eight 16-bit halves of the Philox call (exact in float32)."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)
    g = (np.asarray(gids, dtype=np.int64).reshape(-1, 1) & 0xFFFFFFFF)
    w = named_draw.philox4x32_10(g, step & 0xFFFFFFFF, abi.MPC_OBSERVE_RNG_NOISE | (((step >> 32) << 8) & 0xFFFFFFFF),
                                 np.asarray(fields, dtype=np.int64).reshape(1, -1), seed & 0xFFFFFFFF, seed >> 32)
    total = sum((x & np.uint32(0xFFFF)).astype(np.int64) + (x >> np.uint32(16)).astype(np.int64) for x in w)
    return (2 * total - 524280).astype(np.float32)


def hold_uniform(seed, gids, step):
    """float32 [M]: u = (w >> 8) * 2^-24 of the hold stream behind step ``step``."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)
    g = np.asarray(gids, dtype=np.int64).reshape(-1) & 0xFFFFFFFF
    w = named_draw.philox4x32_10(g, step & 0xFFFFFFFF, abi.MPC_OBSERVE_RNG_HOLD | (((step >> 32) << 8) & 0xFFFFFFFF), 0,
                                 seed & 0xFFFFFFFF, seed >> 32)
    return (w[0] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def fk64(q, qd, link_length, joint1_z, phi0):
    """float64 [M, 4]: tip y, z, vy, vz of joint states ``q``, ``qd`` [M, 6] -- ``tip_fk_joint`` of csrc/vine_task_shared.h in
    double."""
    q, qd = np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64)
    phi = np.float64(phi0) + np.cumsum(q[:, 1:], axis=1)
    w = np.cumsum(qd[:, 1:], axis=1)
    L = np.float64(link_length)
    return np.stack([q[:, 0] - L * np.sin(phi).sum(1), np.float64(joint1_z) + L * np.cos(phi).sum(1),
                     qd[:, 0] - L * (w * np.cos(phi)).sum(1), -L * (w * np.sin(phi)).sum(1)], axis=1)


def noisy_frame(table, seed, step, column, tip):
    """The frame of one step: ``column`` [VF_COUNT, M] float32 with, for the plants with a non-zero noise value, the twelve
    joint fields moved by the sensor's noise (one float32 multiply, one float32 add) and the fields a joint state determines
    formed anew, as ``vine_sysid_pin`` forms them.  ``tip(q, qd, plants)`` -> [len(plants), 4]: the tip of those joint states."""
    table = np.asarray(table, dtype=np.float32)
    frame = np.array(column, dtype=np.float32)
    f = abi
    for row, first, word0 in ((abi.VMO_NOISE_Q, f.VF_Q0, 0), (abi.VMO_NOISE_QD, f.VF_QD0, 6)):
        on = np.flatnonzero(table[row] != 0)
        if len(on):
            c = (table[row][on].astype(np.float64) * NOISE_SCALE).astype(np.float32)
            z = noise_deviate(seed, on, step, np.arange(word0, word0 + 6))
            frame[first:first + 6, on] = frame[first:first + 6, on] + (z * c[:, None]).T          # float32 throughout
    noisy = np.flatnonzero((table[abi.VMO_NOISE_Q] != 0) | (table[abi.VMO_NOISE_QD] != 0))
    if len(noisy):
        if tip is None:
            raise ValueError("noisy_frame: a non-zero noise value needs tip(q, qd, plants), the tip of a joint state")
        q, qd = frame[f.VF_Q0:f.VF_Q0 + 6, noisy].T, frame[f.VF_QD0:f.VF_QD0 + 6, noisy].T
        t = np.asarray(tip(q, qd, noisy), dtype=np.float32).reshape(len(noisy), 4)
        frame[f.VF_TIP_Y:f.VF_TIP_VZ + 1, noisy] = t.T
        frame[f.VF_CART_Y, noisy], frame[f.VF_CART_VY, noisy] = q[:, 0], qd[:, 0]
        frame[f.VF_PREV_Q0:f.VF_PREV_Q0 + 6, noisy] = q.T
        frame[f.VF_PREV_TIP_Y, noisy], frame[f.VF_PREV_TIP_Z, noisy] = t[:, 0], t[:, 1]
        frame[f.VF_PREV_CART_VEL, noisy] = qd[:, 0]
    return frame


def measure_replay(table, seed, steps, columns, progress, plant_actions, tip=None, external_resets=None, state=None):
    """``vine_mpc_observe_measure`` behind T plant steps, on the host.  ``table`` [4, M] float32; ``steps`` [T]: the index of
    the step each launch rides behind; ``columns`` [T, VF_COUNT, M] float32: the plants' state block behind each step;
    ``progress`` [T, M]: the plant's progress buffer; ``plant_actions`` [T, M, 2]: what each step consumed; ``tip``: see
    ``noisy_frame`` (needed only where a noise value is non-zero; the device's is float32 ``tip_fk_joint``, which numpy does
    not reproduce to the bit -- a bit-for-bit comparison hands in the device's own tips and holds those to their own checks);
    ``external_resets``: ``None`` or a sequence [T] of plant-index lists reset from outside BEFORE step t
    (``ObservingController.reset_plants``); ``state``: ``{"snap", "act_log", "age", "fresh"}`` in force before the first step
    (default: zeros, ``fresh`` ones).  Returns one dict per step, the state BEHIND that step's launch: ``snap`` [SLOTS,
    VF_COUNT, M] (the ring fields of a slot are never written), ``act_log`` [M, LOG, 2], ``age`` [M] int32, ``fresh`` [M]
    uint8, ``held`` and ``first`` [M] bool, ``frame`` [VF_COUNT, M]."""
    table = np.asarray(table, dtype=np.float32)
    M = table.shape[1]
    cols = np.asarray(columns, dtype=np.float32)
    progress = np.asarray(progress).reshape(len(cols), M)
    acts = np.asarray(plant_actions, dtype=np.float32).reshape(len(cols), M, 2)
    state = state or {}
    snap = np.array(state.get("snap", np.zeros((SLOTS, abi.VF_COUNT, M))), dtype=np.float32)
    act_log = np.array(state.get("act_log", np.zeros((M, LOG, 2))), dtype=np.float32)
    age = np.array(state.get("age", np.zeros(M)), dtype=np.int32)
    fresh = np.array(state.get("fresh", np.ones(M)), dtype=np.uint8)
    out = []
    for t in range(len(cols)):
        if external_resets is not None and len(external_resets[t]):
            ids = np.asarray(external_resets[t], dtype=np.int64)
            fresh[ids] = 1
            act_log[ids] = 0.0
        s = int(steps[t])
        frame = noisy_frame(table, seed, s, cols[t], tip)
        first = (progress[t] == 0) | (fresh != 0)
        held = ~first & (hold_uniform(seed, np.arange(M), s) < table[abi.VMO_HOLD])
        cur, prev = s % SLOTS, (s - 1) % SLOTS
        snap = snap.copy()
        pushed = np.where(held[None, :], snap[prev], frame)
        snap[cur][NOT_RING] = pushed[NOT_RING]
        snap[:, NOT_RING[:, None], np.flatnonzero(first)[None, :]] = frame[NOT_RING][:, first][None]
        age = np.where(first, 0, np.minimum(age + 1, abi.MAX_DELAY)).astype(np.int32)
        fresh = np.zeros(M, dtype=np.uint8)
        act_log = np.concatenate([acts[t][:, None], act_log[:, :-1]], axis=1)
        out.append({"snap": snap, "act_log": act_log, "age": age.copy(), "fresh": fresh.copy(), "held": held, "first": first,
                    "frame": frame})
    return out


def catchup_schedule(catchup, d):
    """The C predictor steps of one control step for a plant with lag ``d`` (0 .. C): one dict per i = 0 .. C -- i = 0 the pin,
    i >= 1 the node behind the i-th step -- with ``pinned`` (the plant is put onto the delivered frame: the pin, and every
    step that did not count), ``real`` (the step just run was one of the plant's d) and ``action`` (the index into ``act_log``
    of the next step's action; ``None``: (0, 0); ``"none"`` behind the last step: nothing is written)."""
    C, d = int(catchup), int(d)
    if not 0 <= d <= C:
        raise ValueError("catchup_schedule: needs 0 <= d <= catchup, not d = %d, catchup = %d" % (d, C))
    out = []
    for i in range(C + 1):
        pinned = i <= C - d
        action = "none" if i == C else (C - i - 1 if i >= C - d else None)
        out.append({"i": i, "pinned": pinned, "real": i >= 1 and not pinned, "action": action})
    return out


def pin_replay(table, state, plant_column, plant_progress, plant_steps, catchup, compensate, step_index=0):
    """``vine_mpc_observe_pin`` (``step_index`` 0) or the catch-up node behind the predictor's ``step_index``-th step, on the
    host.  ``table`` [4, M]; ``state``: ``{"snap", "act_log", "age", "fresh"}`` as ``measure_replay`` returns them;
    ``plant_column`` [VF_COUNT, M] and ``plant_progress`` [M]: the plant's block and progress now; ``plant_steps``: the plant
    handle's steps completed.  Returns a dict: ``lag`` [M] (d), ``behind`` [M] (dd: how old the delivered frame is),
    ``pinned`` [M] bool (the lanes that were put onto their frame; for the others only ``reset`` is written), ``column``
    [VF_COUNT, M] (the delivered frame; the ring fields hold nothing), ``progress`` [M], ``ring_history`` [M, MAX_DELAY, 2]
    (the actions whose commands the predictor's ring is rebuilt from: entry k - 1 goes to slot (c - k) mod a, as
    ``vine_mpc_fork`` places ``history``), ``actions`` [M, 2] and ``writes_action`` (False behind the last step)."""
    table = np.asarray(table, dtype=np.float32)
    M, C, i = table.shape[1], int(catchup), int(step_index)
    snap, act_log = np.asarray(state["snap"], dtype=np.float32), np.asarray(state["act_log"], dtype=np.float32)
    age, fresh = np.asarray(state["age"]).astype(np.int64), np.asarray(state["fresh"])
    known = (fresh != 0) | (int(plant_steps) == 0)
    delay = np.clip(table[abi.VMO_DELAY].astype(np.int64), 0, abi.MAX_DELAY)
    dd = np.where(known, 0, np.minimum(delay, np.clip(age, 0, abi.MAX_DELAY)))
    d = np.minimum(dd, C) if compensate else np.zeros(M, dtype=np.int64)
    s = int(plant_steps) - 1
    column = np.where(known[None, :], np.asarray(plant_column, dtype=np.float32), snap[(s - dd) % SLOTS, :, np.arange(M)].T)
    column[RING] = 0.0
    pinned = i <= C - d
    hist = np.stack([act_log[p, d[p]:d[p] + abi.MAX_DELAY] for p in range(M)])
    actions = np.zeros((M, 2), dtype=np.float32)
    if i < C:
        use = i >= C - d
        actions[use] = act_log[np.flatnonzero(use), C - i - 1]
    return {"lag": d.astype(np.int32), "behind": dd, "pinned": pinned, "column": column,
            "progress": np.asarray(plant_progress).astype(np.int64) - dd, "ring_history": hist, "actions": actions,
            "writes_action": i < C}


# ------------------------------------------------------------------------------------------------------------ the device
class ObservingController(Controller):
    """A ``Controller`` that sees its plants through the sensing path of include/vine_mpc_observe.h.  It owns the predictor
    task (``predictor_task``: ``model_config(cfg, M, 1, ...)``, the model's plant with one env per real plant; closed by
    ``close()``) and the buffers.

    ``control_step()`` = ``pin()``, C x (``predictor.step_into`` + ``catchup(i)``), ``vine_mpc_fork`` from the predictor, the
    unchanged horizon and update, the plant step, ``measure()``."""

    def __init__(self, plant_task, model_task, predictor_task, samples, observe, horizon=MPC_DEFAULTS["horizon"],
                 lam=MPC_DEFAULTS["lambda"], sigma=MPC_DEFAULTS["sigma"], seed=MPC_DEFAULTS["seed"], graph=True, graph_steps=1,
                 keep_weights=False):
        import torch
        super().__init__(plant_task, model_task, samples, horizon, lam, sigma, seed, graph=graph, graph_steps=graph_steps,
                         keep_weights=keep_weights)
        self.predictor = predictor_task
        self.tasks += (predictor_task,)
        self.fork_source = predictor_task            # the samples start where the controller believes the plant to be
        if int(predictor_task.num_envs) != self.M:
            raise ConfigError("%s: the predictor task has %d envs, not plants = %d" % (_KEY, int(predictor_task.num_envs), self.M))
        if predictor_task.device != self.device:
            raise ConfigError("%s: the predictor task sits on %s, the plant on %s" % (_KEY, predictor_task.device, self.device))
        self.spec = observe_config(observe)
        self.C = self.spec["CATCHUP"]
        self.table_host = draw_observe(self.spec, seed, np.arange(self.M)).astype(np.float32)
        self.ocfg = observe_cconfig(self.M, self.C, self.spec["COMPENSATE"], seed, self.table_host)
        M, dev, f32 = self.M, self.device, torch.float32
        self.table = torch.as_tensor(self.table_host, device=dev).contiguous()
        self.snap = torch.zeros((SLOTS, abi.VF_COUNT, M), dtype=f32, device=dev)
        self.act_log = torch.zeros((M, LOG, 2), dtype=f32, device=dev)
        self.age = torch.zeros(M, dtype=torch.int32, device=dev)
        self.fresh = torch.ones(M, dtype=torch.uint8, device=dev)
        self.lag = torch.zeros(M, dtype=torch.int32, device=dev)
        self.predictor_actions = torch.zeros((M, abi.NUM_ACTIONS), dtype=f32, device=dev)
        self.predictor_obs = torch.zeros((M, predictor_task.num_obs), dtype=f32, device=dev)
        self.use_graph = self.use_graph and bool(getattr(predictor_task, "graph_capturable", False))
        self.launches.update({"pin": 0, "catchup": 0, "predictor_step": 0, "measure": 0})

    def tensors(self):
        return super().tensors() + [self.snap, self.act_log, self.age, self.fresh, self.lag, self.predictor_actions,
                                    self.predictor_obs]

    # -- the three launches ----------------------------------------------------------------------------------------------
    def _pin_args(self):
        r = self.predictor
        return [self.table.data_ptr(), self.plant.progress_buf.data_ptr(), self.snap.data_ptr(), self.act_log.data_ptr(),
                self.age.data_ptr(), self.fresh.data_ptr(), self.predictor_actions.data_ptr(), r.rew_buf.data_ptr(),
                r.reset_buf.data_ptr(), r.progress_buf.data_ptr(), self.lag.data_ptr(), self._stream()]

    def pin(self):
        from .. import native
        native.check(self.lib.vine_mpc_observe_pin(self.plant._handle, self.predictor._handle, self.ocfg, *self._pin_args()),
                     self.lib)
        self.launches["pin"] += 1

    def catchup(self, i):
        from .. import native
        native.check(self.lib.vine_mpc_observe_catchup(self.plant._handle, self.predictor._handle, self.ocfg, int(i),
                                                       *self._pin_args()), self.lib)
        self.launches["catchup"] += 1

    def measure(self):
        from .. import native
        native.check(self.lib.vine_mpc_observe_measure(
            self.plant._handle, self.ocfg, self.table.data_ptr(), self.plant.progress_buf.data_ptr(),
            self.plant_actions.data_ptr(), self.snap.data_ptr(), self.act_log.data_ptr(), self.age.data_ptr(),
            self.fresh.data_ptr(), self._stream()), self.lib)
        self.launches["measure"] += 1

    def predict(self):
        """The pin and the catch-up: behind it the predictor stands where the controller believes the plant to be."""
        self.pin()
        for i in range(1, self.C + 1):
            self.predictor.step_into(self.predictor_actions, self.predictor_obs)
            self.launches["predictor_step"] += 1
            self.catchup(i)

    def control_step(self):
        """One control step, eagerly (or into a capture)."""
        self.predict()
        super().control_step()
        self.measure()

    # -- from outside the step -------------------------------------------------------------------------------------------
    def set_model_params(self, values):
        """``Controller.set_model_params``, and each plant's value into the predictor's bound table, not repeated."""
        super().set_model_params(values)
        self.predictor.set_env_params({k: np.asarray(v, dtype=np.float64) for k, v in values.items()})

    def clear_rows(self, ids):
        """The next frame of each is its episode's first, and its action log starts anew."""
        super().clear_rows(ids)
        self.fresh[ids] = 1
        self.act_log[ids] = 0.0

    def close(self):
        self.predictor.close()


# ------------------------------------------------------------------------------------------------------------------ a run
class Play(PlayVariant):
    """``observe=`` of ``mpc.play``."""

    def check(self, run):
        self.checked = observe_config(self.spec)

    def make(self, run):
        pcfg = copy.deepcopy(run.mcfg)                   # the model's plant once more, one env per real plant
        pcfg["env"]["numEnvs"] = run.M
        run.predictor = make_task(pcfg, run.device)

    def controller(self, run):
        return ObservingController(run.plant, run.model, run.predictor, run.samples, self.spec, *run.planner, graph=run.graph)

    def banner(self, run):
        ctl = run.ctl
        print("mpc: observing through DELAY %s, HOLD %s, NOISE_Q %s, NOISE_QD %s; %d catch-up steps, %s" % (
            ctl.spec["DELAY"], ctl.spec["HOLD"], ctl.spec["NOISE_Q"], ctl.spec["NOISE_QD"], ctl.C,
            "compensated" if ctl.spec["COMPENSATE"] else "not compensated"), flush=True)

    def result(self, run, out):
        ctl = run.ctl
        out["observe"] = {"names": list(NAMES), "table": ctl.table_host.copy(), "catchup": ctl.C,
                          "compensate": ctl.spec["COMPENSATE"], "lag": float(ctl.lag.double().mean())}
