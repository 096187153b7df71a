"""MPC_FILTER on the host side: a fixed-gain corrector (a Luenberger observer, alpha-beta style) over the frames of the
predictive controller's sensing path.  Per plant an estimate of the whole state-block column is advanced once per control step
by one step of the predictor (``vine_mpc_filter_pin``) and pulled towards the frame of that step by two gains
(``vine_mpc_filter_correct``); the unchanged pin and catch-up of MPC_OBSERVE then deliver that estimate instead of the raw
frame.  The semantics are stated once, in include/vine_mpc_filter.h.  What is left for the host: the configuration
(``filter_config``, ``draw_gains``, ``largest_reach``), the numpy statements every GPU test compares against
(``filter_pin_replay``, ``filter_correct_replay``) and the controller (``FilteringController``).

``filter=`` of ``mpc.play`` / ``mpc.py`` maps

  ``GAIN_Q``       the gain on the six joint-position innovations, [0, 1]; 1: the frame itself, 0: the model alone
  ``GAIN_QD``      ... on the six joint-velocity innovations, [0, 1]
                   each a number (default ``DEFAULT_GAIN``), ``[lo, hi]`` or ``{values: [...]}``, drawn once per plant with the
                   sensor's draw under the keys ``FILTER_<NAME>``"""
import numpy as np

from .. import abi
from . import env_params, named_draw
from .config import ConfigError
from .mpc import DEFAULTS as MPC_DEFAULTS
from .mpc import PlayVariant
from .mpc_observe import LOG, NOT_RING, RING, SLOTS, ObservingController, hold_uniform

_KEY = "mpc: filter"
NAMES = tuple(abi.MPC_FILTER_NAMES)                   # the table's rows, the order of the mixed radix
DRAW_NAMES = tuple("FILTER_" + n for n in NAMES)      # the names the draw is keyed by
DEFAULT_GAIN = 0.3
JOINTS = np.arange(abi.VF_Q0, abi.VF_Q0 + 12)         # six q, six qd
# what a joint state determines ("Derived fields" of include/vine_mpc_observe.h)
DERIVED = np.array([abi.VF_TIP_Y, abi.VF_TIP_Z, abi.VF_TIP_VY, abi.VF_TIP_VZ, abi.VF_CART_Y, abi.VF_CART_VY]
                   + list(range(abi.VF_PREV_Q0, abi.VF_PREV_Q0 + 6)) + [abi.VF_PREV_TIP_Y, abi.VF_PREV_TIP_Z, abi.VF_PREV_CART_VEL])


# ---------------------------------------------------------------------------------------------------------- configuration
def filter_config(spec):
    """The checked ``filter=`` mapping as plain numbers and lists: ``{"GAIN_Q", "GAIN_QD"}``, each a number, ``[lo, hi]`` or
    ``{"values": [..]}`` inside [0, 1].  ``ConfigError``, naming the key, for every bad key or value."""
    if not hasattr(spec, "keys"):
        raise ConfigError("%s={NAME: value, ...} must be a mapping, not %r" % (_KEY, spec))
    unknown = sorted(str(k) for k in set(spec.keys()) - set(NAMES))
    if unknown:
        raise ConfigError("%s: unknown key(s) %s" % (_KEY, ", ".join(unknown)))
    out = {}
    for name in NAMES:
        where = "%s.%s" % (_KEY, name)
        out[name] = named_draw.form(where, spec.get(name, DEFAULT_GAIN))
        for v in named_draw.candidates(out[name]):
            if not 0.0 <= v <= 1.0:
                raise ConfigError("%s: %g lies outside [0, 1]" % (where, v))
    return out


def draw_gains(spec, seed, gids):
    """float64 [2, M]: GAIN_Q and GAIN_QD of the plants with global ids ``gids``: episode 0 of ``named_draw.draw`` under the
    names ``FILTER_<NAME>``."""
    return named_draw.draw(named_draw.named(NAMES, DRAW_NAMES, spec), seed, gids, 0, who="draw_gains")


def check_gains(gain, num_plants):
    """``gain`` as float32 [2, M]; a ``ConfigError`` for another shape or a value outside [0, 1]."""
    gain = np.asarray(gain, dtype=np.float32)
    if gain.shape != (len(NAMES), int(num_plants)):
        raise ConfigError("%s: the gain table must be [%d, %d], not %s" % (_KEY, len(NAMES), int(num_plants), gain.shape))
    if not np.all((gain >= 0.0) & (gain <= 1.0)):
        raise ConfigError("%s: a gain lies outside [0, 1]" % _KEY)
    return gain


def largest_reach(observe_spec, action_delay):
    """The deepest entry of ``act_log`` the filter's pin can read: the largest ``DELAY`` of the checked ``observe=`` spec plus
    the model's largest ``ACTION_DELAY``.  A ``ConfigError`` naming both when it lies beyond the log's last entry."""
    delay = int(max(named_draw.candidates(observe_spec["DELAY"])))
    reach = delay + int(action_delay)
    if reach > LOG - 1:
        raise ConfigError("%s: the largest observe.DELAY, %d, plus the model's largest ACTION_DELAY, %d, exceeds %d: the action "
                          "log does not reach that far back" % (_KEY, delay, int(action_delay), LOG - 1))
    return reach


def model_action_delay(env_cfg, model_params=None):
    """The largest ``ACTION_DELAY`` a model env can have: the ``task.env`` mapping's own, or the largest candidate of a
    ``model_params`` spec that names it."""
    entry = (model_params or {}).get("ACTION_DELAY")
    if entry is None:
        return int(env_cfg.get("ACTION_DELAY", 0))
    return int(max(named_draw.candidates(env_params.spec_forms({"ACTION_DELAY": entry})["ACTION_DELAY"])))


# ---------------------------------------------------------------------------------------------------- the launches, in numpy
def _frame_step(table, state, plant_steps):
    """known [M], dd [M] and e [M] of include/vine_mpc_filter.h, NOTATION."""
    table = np.asarray(table, dtype=np.float32)
    age, fresh = np.asarray(state["age"]).astype(np.int64), np.asarray(state["fresh"])
    known = (fresh != 0) | (int(plant_steps) == 0)
    delay = np.clip(table[abi.VMO_DELAY].astype(np.int64), 0, abi.MAX_DELAY)
    dd = np.where(known, 0, np.minimum(delay, np.clip(age, 0, abi.MAX_DELAY)))
    return known, dd, int(plant_steps) - 1 - dd


def filter_pin_replay(table, state, est, est_index, plant_column, plant_progress, plant_steps):
    """``vine_mpc_filter_pin`` on the host.  ``table`` [4, M]: the observe table; ``state``: ``{"act_log", "age", "fresh"}`` as
    ``mpc_observe.measure_replay`` returns them; ``est`` [SLOTS, VF_COUNT, M], ``est_index`` [M]; ``plant_column`` [VF_COUNT, M]
    and ``plant_progress`` [M]: the plant's block and progress now; ``plant_steps``: the plant handle's steps completed.
    Returns a dict: ``advancing`` [M] bool, ``behind`` [M] (dd), ``e`` [M], ``column`` [VF_COUNT, M] (what every plant's
    predictor column is put on; the ring fields hold nothing), ``progress`` [M] (written for the advancing only),
    ``ring_history`` [M, MAX_DELAY, 2] (the actions the advancing plants' ring is rebuilt from: entry k - 1 goes to slot
    (c - k) mod a; entries beyond the log's end read (0, 0)) and ``actions`` [M, 2]."""
    est, est_index = np.asarray(est, dtype=np.float32), np.asarray(est_index).astype(np.int64)
    act_log = np.asarray(state["act_log"], dtype=np.float32)
    M = est.shape[2]
    known, dd, e = _frame_step(table, state, plant_steps)
    advancing = ~known & (np.asarray(state["age"]) != 0) & (est_index >= 0) & (est_index == e - 1)
    same = ~advancing & ~known & (est_index >= 0) & (est_index == e)
    column = np.array(plant_column, dtype=np.float32)
    lanes = np.arange(M)
    column[:, advancing] = est[(e - 1) % SLOTS, :, lanes].T[:, advancing]
    column[:, same] = est[e % SLOTS, :, lanes].T[:, same]
    column[RING] = 0.0
    padded = np.concatenate([act_log, np.zeros((M, abi.MAX_DELAY + 1, 2), dtype=np.float32)], axis=1)
    hist = np.stack([padded[p, dd[p] + 1:dd[p] + 1 + abi.MAX_DELAY] for p in range(M)])
    actions = np.zeros((M, 2), dtype=np.float32)
    actions[advancing] = act_log[lanes, dd][advancing]
    return {"advancing": advancing, "behind": dd, "e": e, "column": column,
            "progress": np.asarray(plant_progress).astype(np.int64) - dd - 1, "ring_history": hist, "actions": actions}


CASES = ("known", "first", "same", "held", "unit", "still", "blend", "other")


def filter_correct_replay(table, gain, seed, state, est, est_index, innov, predictor_column, plant_steps, tip=None):
    """``vine_mpc_filter_correct`` on the host.  ``table`` [4, M], ``gain`` [2, M]; ``seed``: the observe config's; ``state``:
    ``{"snap", "age", "fresh"}``; ``est``, ``est_index``, ``innov`` [2, M]: the filter's state in front of the launch;
    ``predictor_column`` [VF_COUNT, M]: the predictor's block behind its step (as ``pin_replay`` takes the plant's);
    ``tip(q, qd, plants)`` -> [len(plants), 4]: the tip of those joint states (needed only where an estimate is blended; the
    device's is float32 ``tip_fk_joint``, which numpy does not reproduce to the bit -- a bit-for-bit comparison hands in the
    device's own tips).  Returns a dict: ``est``, ``est_index``, ``innov`` behind the launch and ``case`` [M]: one of ``CASES``
    per plant -- a., b., c. of the header, d. as ``held`` / ``unit`` (both gains 1) / ``still`` (every innovation zero) /
    ``blend``, and e. as ``other``."""
    table, gain = np.asarray(table, dtype=np.float32), np.asarray(gain, dtype=np.float32)
    snap = np.asarray(state["snap"], dtype=np.float32)
    est, est_index = np.array(est, dtype=np.float32), np.array(est_index).astype(np.int64)
    innov = np.array(innov, dtype=np.float32)
    xminus = np.asarray(predictor_column, dtype=np.float32)
    M = est.shape[2]
    known, dd, e = _frame_step(table, state, plant_steps)
    age = np.asarray(state["age"])
    case = np.empty(M, dtype=object)
    f = abi
    for p in range(M):
        ep = int(e[p])
        if known[p]:
            case[p], est_index[p] = "known", -1
            continue
        y = snap[ep % SLOTS, :, p]
        if age[p] == 0:
            case[p] = "first"
            est[:, NOT_RING, p] = y[NOT_RING][None]
            est_index[p], innov[:, p] = ep, 0.0
            continue
        if est_index[p] == ep:
            case[p] = "same"
            continue
        advancing = est_index[p] >= 0 and est_index[p] == ep - 1
        est_index[p] = ep
        if not advancing:
            case[p] = "other"
            est[ep % SLOTS, NOT_RING, p] = y[NOT_RING]
            continue
        if hold_uniform(seed, [p], ep)[0] < table[abi.VMO_HOLD, p]:
            case[p] = "held"
            est[ep % SLOTS, NOT_RING, p] = xminus[NOT_RING, p]
            innov[:, p] = 0.0
            continue
        x = xminus[JOINTS, p]
        v = y[JOINTS] - x                                                   # float32 throughout
        for row in (0, 1):
            total = np.float32(0.0)
            for i in range(6):
                total = np.float32(total + np.float32(v[6 * row + i] * v[6 * row + i]))
            innov[row, p] = total
        new = y.copy()
        if gain[abi.VMF_GAIN_Q, p] == 1.0 and gain[abi.VMF_GAIN_QD, p] == 1.0:
            case[p] = "unit"
        elif not np.any(v != 0):
            case[p] = "still"
            new[JOINTS], new[DERIVED] = x, xminus[DERIVED, p]
        else:
            case[p] = "blend"
            g = np.repeat(gain[:, p], 6)
            joint = x + g * v                                               # one float32 multiply, one float32 add
            if tip is None:
                raise ValueError("filter_correct_replay: a blended estimate needs tip(q, qd, plants), the tip of a joint state")
            q, qd = joint[:6], joint[6:]
            t = np.asarray(tip(q[None], qd[None], np.array([p])), dtype=np.float32).reshape(4)
            new[JOINTS] = joint
            new[f.VF_TIP_Y:f.VF_TIP_VZ + 1] = t
            new[f.VF_CART_Y], new[f.VF_CART_VY] = q[0], qd[0]
            new[f.VF_PREV_Q0:f.VF_PREV_Q0 + 6] = q
            new[f.VF_PREV_TIP_Y], new[f.VF_PREV_TIP_Z] = t[0], t[1]
            new[f.VF_PREV_CART_VEL] = qd[0]
        est[ep % SLOTS, NOT_RING, p] = new[NOT_RING]
    return {"est": est, "est_index": est_index, "innov": innov, "case": case}


# ------------------------------------------------------------------------------------------------------------ the device
class FilteringController(ObservingController):
    """An ``ObservingController`` whose pin and catch-up are delivered the filter's estimate instead of the raw frame.  It owns
    ``gain`` [2, M], the estimate ring ``est``, ``est_index`` and the diagnostic ``innov``.

    ``control_step()`` = ``filter_pin()``, one ``predictor.step_into``, ``filter_correct()``, then the observing controller's
    control step with ``est`` in ``snap``'s place: the predictor takes C + 1 steps per control step."""

    def __init__(self, plant_task, model_task, predictor_task, samples, observe, filter, horizon=MPC_DEFAULTS["horizon"],
                 lam=MPC_DEFAULTS["lambda"], sigma=MPC_DEFAULTS["sigma"], seed=MPC_DEFAULTS["seed"], graph=True, graph_steps=1,
                 keep_weights=False):
        import torch
        super().__init__(plant_task, model_task, predictor_task, samples, observe, horizon, lam, sigma, seed, graph=graph,
                         graph_steps=graph_steps, keep_weights=keep_weights)
        self.filter_spec = filter_config(filter)
        self.gain_host = check_gains(draw_gains(self.filter_spec, seed, np.arange(self.M)), self.M)
        M, dev = self.M, self.device
        self.gain = torch.as_tensor(self.gain_host, device=dev).contiguous()
        self.est = torch.zeros((SLOTS, abi.VF_COUNT, M), dtype=torch.float32, device=dev)
        self.est_index = torch.full((M,), -1, dtype=torch.int64, device=dev)
        self.innov = torch.zeros((2, M), dtype=torch.float32, device=dev)
        self.launches.update({"filter_pin": 0, "filter_correct": 0})

    def tensors(self):
        return super().tensors() + [self.est, self.est_index, self.innov]

    def _pin_args(self):
        """The observe pin's and the catch-up node's arguments with the estimate ring in ``snap``'s place."""
        args = super()._pin_args()
        args[2] = self.est.data_ptr()
        return args

    # -- the two launches ------------------------------------------------------------------------------------------------
    def filter_pin(self):
        from .. import native
        r = self.predictor
        native.check(self.lib.vine_mpc_filter_pin(
            self.plant._handle, r._handle, self.ocfg, self.table.data_ptr(), self.plant.progress_buf.data_ptr(),
            self.est.data_ptr(), self.est_index.data_ptr(), self.act_log.data_ptr(), self.age.data_ptr(), self.fresh.data_ptr(),
            self.predictor_actions.data_ptr(), r.rew_buf.data_ptr(), r.reset_buf.data_ptr(), r.progress_buf.data_ptr(),
            self._stream()), self.lib)
        self.launches["filter_pin"] += 1

    def filter_correct(self):
        from .. import native
        native.check(self.lib.vine_mpc_filter_correct(
            self.plant._handle, self.predictor._handle, self.ocfg, self.table.data_ptr(), self.gain.data_ptr(),
            self.snap.data_ptr(), self.age.data_ptr(), self.fresh.data_ptr(), self.est.data_ptr(), self.est_index.data_ptr(),
            self.innov.data_ptr(), self._stream()), self.lib)
        self.launches["filter_correct"] += 1

    def advance(self):
        """The estimate of every plant moved on to the step its delivered frame belongs to."""
        self.filter_pin()
        self.predictor.step_into(self.predictor_actions, self.predictor_obs)
        self.launches["predictor_step"] += 1
        self.filter_correct()

    def predict(self):
        """The filter's step, then the pin and the catch-up from the estimate."""
        self.advance()
        super().predict()

    def clear_rows(self, ids):
        """The estimate of each is forgotten."""
        super().clear_rows(ids)
        self.est_index[ids] = -1


# ------------------------------------------------------------------------------------------------------------------ a run
class Play(PlayVariant):
    """``filter=`` of ``mpc.play``; ``observe=`` is given with it and has been checked."""

    def check(self, run):
        filter_config(self.spec)
        if run.model_params:
            env_params.spec_forms(run.model_params)
        largest_reach(run.given["observe"].checked, model_action_delay(run.cfg["env"], run.model_params))

    def controller(self, run):
        return FilteringController(run.plant, run.model, run.predictor, run.samples, run.given["observe"].spec, self.spec,
                                   *run.planner, graph=run.graph)

    def banner(self, run):
        print("mpc: filtering with GAIN_Q %s, GAIN_QD %s" % (run.ctl.filter_spec["GAIN_Q"], run.ctl.filter_spec["GAIN_QD"]),
              flush=True)

    def result(self, run, out):
        out["filter"] = {"names": list(NAMES), "gain": run.ctl.gain_host.copy(),
                         "innov": run.ctl.innov.double().mean(dim=1).cpu().numpy()}
        print("mpc: mean lag %.3g, mean innovation (sum of squares) q %.4g, qd %.4g" % (
            out["observe"]["lag"], out["filter"]["innov"][0], out["filter"]["innov"][1]), flush=True)

    def report_rows(self, run, rows):
        for slot, name in enumerate(DRAW_NAMES):             # a gain that varies over the plants is a parameter of the report
            if len(np.unique(run.ctl.gain_host[slot])) > 1:
                rows["param_" + name] = run.ctl.gain_host[slot][rows["env"]]
