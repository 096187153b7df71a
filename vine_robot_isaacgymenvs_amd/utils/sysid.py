"""SYSID on the host side: which plant produced a recorded trajectory?

A log of ONE env (a MAT file of ``RECORD_TRAJECTORIES``, or of the real robot in the same layout) is scored against every
env of a batch whose ``ENV_PARAMS`` table holds the candidate plants: ``vine_sysid_pin`` puts all of them onto a row of the
log, and behind every step ``vine_sysid_scheduled`` (include/vine_sysid.h) adds each env's squared distance from the log's
next row to a float64 sum on the device and hands the step the log's next action.  What is left for the host is cheap and
rare: reading the file (``load_log``), choosing where windows may start (``windows``), and a cross-entropy search over
the table (``cem``), one table upload and one read of N sums per iteration.  ``fit`` ties them together; ``sysid.py`` at
the repository root is its command line."""
import copy
import json
import logging
import os
import time

import numpy as np

from .. import abi
from . import env_params
from .config import ConfigError

REQUIRED_KEYS = ("cart_pos", "Q", "cart_vel", "Qd", "action", "smoothed_u_fpam", "reset", "progress")
DEFAULT_WEIGHTS = (1.0,) * abi.NUM_DOFS + (0.0,) * (abi.SYSID_FIELDS - abi.NUM_DOFS)
_GOLDEN = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------------------------------------------------ the log
def load_log(path, weights=None):
    """A MAT file of ``RECORD_TRAJECTORIES`` as the ``[T, abi.RECORD_FIELDS]`` float32 table of its rows (``VRF_*`` layout):
    the inverse of ``trajectory.trajectory_arrays``.  ``REQUIRED_KEYS`` must be there -- a log without ``action`` is refused
    by name: a log of the real robot must carry the commanded actions.  ``tip_pos`` / ``tip_vel`` may be missing when the
    ``weights`` of the four tip fields are 0 (their columns are then 0); every other key is optional and 0 when absent."""
    import scipy.io
    mat = scipy.io.loadmat(path)
    for key in REQUIRED_KEYS:
        if key not in mat:
            hint = ": a log must carry the commanded actions (RECORD_TRAJECTORIES writes them)" if key == "action" else ""
            raise ValueError("%s: the log has no '%s'%s" % (path, key, hint))
    w = np.asarray(DEFAULT_WEIGHTS if weights is None else weights, dtype=np.float64)
    f = abi
    T = np.asarray(mat["cart_pos"]).shape[1]
    rows = np.zeros((T, abi.RECORD_FIELDS), dtype=np.float32)

    def put(col, key, count=1, first=0):
        a = np.asarray(mat[key], dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != T or a.shape[0] < first + count:
            raise ValueError("%s: '%s' has shape %s, expected (%d, %d)" % (path, key, a.shape, first + count, T))
        rows[:, col:col + count] = a[first:first + count].T.astype(np.float32)

    put(f.VRF_Q0, "cart_pos")
    put(f.VRF_Q0 + 1, "Q", abi.NUM_LINKS)
    put(f.VRF_QD0, "cart_vel")
    put(f.VRF_QD0 + 1, "Qd", abi.NUM_LINKS)
    put(f.VRF_ACTION0, "action", abi.NUM_ACTIONS)
    put(f.VRF_SMOOTHED_U, "smoothed_u_fpam")
    put(f.VRF_RESET, "reset")
    put(f.VRF_PROGRESS, "progress")
    for key, col, wts in (("tip_pos", f.VRF_TIP_Y, w[f.VRF_TIP_Y:f.VRF_TIP_Z + 1]),
                          ("tip_vel", f.VRF_TIP_VY, w[f.VRF_TIP_VY:f.VRF_TIP_VZ + 1])):
        if key in mat:
            put(col, key, 2, first=1)                 # (3, T) with a zero x row
        elif np.any(wts != 0.0):
            raise ValueError("%s: the log has no '%s' and its fields carry non-zero weights" % (path, key))
    if "moving_target_pos" in mat:
        put(f.VRF_TARGET_Y, "moving_target_pos", 2, first=1)
    for key, col, count in (("reward", f.VRF_REWARD, 1), ("time_out", f.VRF_TIMEOUT, 1), ("obj_info", f.VRF_OBJ_DEPTH, 2),
                            ("contact", f.VRF_CONTACT, 1)):
        if key in mat:
            put(col, key, count)
    return rows


def windows(log, horizon, stride):
    """The start rows r = 0, stride, 2 stride, .. whose window r .. r + horizon stays inside one episode of the log: no
    row r .. r + horizon - 1 has ``reset`` = 1 (the row after it begins another episode), ``progress`` grows by one from
    each row r .. r + horizon - 1 to the next, and r >= VINE_MAX_DELAY -- the pin fills a delay ring from the actions of
    the rows before r -- except that r = 0 is allowed: a log is taken to begin where the ring was empty."""
    log = np.asarray(log)
    T, H, stride = log.shape[0], int(horizon), int(stride)
    if H < 1 or stride < 1:
        raise ValueError("windows: horizon and stride must be positive")
    reset, progress = log[:, abi.VRF_RESET], log[:, abi.VRF_PROGRESS]
    out = []
    for r in range(0, T - H, stride):
        if r != 0 and r < abi.MAX_DELAY:
            continue
        if np.any(reset[r:r + H] != 0):
            continue
        if np.any(np.diff(progress[r:r + H + 1]) != 1):
            continue
        out.append(r)
    return out


# --------------------------------------------------------------------------------------------------------- the device
def sysid_config(lib, num_rows, horizon, weights=None):
    from .. import native
    c = abi.VineSysidConfig()
    native.check(lib.vine_sysid_config_default(c), lib)
    c.num_rows, c.horizon = int(num_rows), int(horizon)
    if weights is not None:
        w = [float(x) for x in weights]
        if len(w) != abi.SYSID_FIELDS:
            raise ValueError("sysid weights: %d values, one per row field 0..%d" % (abi.SYSID_FIELDS, abi.SYSID_FIELDS - 1))
        for i, x in enumerate(w):
            c.weights[i] = x
    return c


class Evaluator:
    """The candidates of ``task`` (a ``Vine5LinkMovingBase`` whose ``ENV_PARAMS`` table holds them) against ``log``
    ([T, RECORD_FIELDS] float32) over windows of ``horizon`` steps.  ``evaluate(starts)`` zeroes ``err``, sets ``alive`` to
    1 and, for each start row, pins every env to it (eagerly) and runs ``horizon`` x (step + scoring node): the pairs are
    captured once as a hipGraph and replayed, or issued eagerly where the task is not capturable (``graph=False`` forces
    that).  Returns ``err`` as float64 [N] with +inf where a candidate left the log's episode."""

    def __init__(self, task, log, horizon, weights=None, graph=True):
        import torch
        self.task, self.lib = task, task._lib
        self.device = task.device
        self.log = torch.as_tensor(np.ascontiguousarray(log, dtype=np.float32), device=self.device).contiguous()
        if self.log.ndim != 2 or self.log.shape[1] != abi.RECORD_FIELDS:
            raise ValueError("sysid log must be [T, %d], not %s" % (abi.RECORD_FIELDS, tuple(self.log.shape)))
        self.horizon = int(horizon)
        self.scfg = sysid_config(self.lib, self.log.shape[0], self.horizon, weights)
        n = task.num_envs
        self.actions = torch.zeros((n, abi.NUM_ACTIONS), dtype=torch.float32, device=self.device)
        self.obs = torch.zeros((n, task.num_obs), dtype=torch.float32, device=self.device)
        self.window = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.err = torch.zeros(n, dtype=torch.float64, device=self.device)
        self.alive = torch.ones(n, dtype=torch.uint8, device=self.device)
        self.use_graph = bool(graph) and bool(getattr(task, "graph_capturable", False)) and not task.observers
        self.graph = None
        self.steps_run = 0

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def pin(self, row):
        from .. import native
        t = self.task
        native.check(self.lib.vine_sysid_pin(t._handle, self.scfg, self.log.data_ptr(), int(row), self.actions.data_ptr(),
                                             t.rew_buf.data_ptr(), t.reset_buf.data_ptr(), t.progress_buf.data_ptr(),
                                             self.window.data_ptr(), self._stream()), self.lib)

    def node(self):
        from .. import native
        t = self.task
        native.check(self.lib.vine_sysid_scheduled(t._handle, self.scfg, self.log.data_ptr(), self.window.data_ptr(),
                                                   self.actions.data_ptr(), t.reset_buf.data_ptr(), self.err.data_ptr(),
                                                   self.alive.data_ptr(), self._stream()), self.lib)

    def step(self):
        """One step on the actions the pin or the node left, and the node behind it."""
        self.task.step_into(self.actions, self.obs)
        self.node()

    def run_window(self):
        import torch
        from ..learning.graph_capture import collector_at_rest
        if not self.use_graph:
            for _ in range(self.horizon):
                self.step()
        else:
            if self.graph is None:
                torch.cuda.synchronize(self.device)
                self.graph = torch.cuda.CUDAGraph()
                with collector_at_rest(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                    for _ in range(self.horizon):
                        self.step()
            self.graph.replay()
        self.steps_run += self.horizon

    def evaluate(self, starts):
        import torch
        self.err.zero_()
        self.alive.fill_(1)
        for r in starts:
            self.pin(r)
            self.run_window()
        torch.cuda.synchronize(self.device)
        err = self.err.cpu().numpy().copy()
        err[self.alive.cpu().numpy() == 0] = np.inf
        return err


FORCED = (
    # (section, key, value): what a candidate batch must be, whatever the configuration says
    ("task", "vine_randomize", False),
    ("randomization_parameters", "OBSERVATION_NOISE_STD", 0.0),
    ("randomization_parameters", "ACTION_NOISE_STD", 0.0),
    ("env", "CREATE_SHELF", False),
    ("env", "CREATE_PIPE", False),
    ("env", "USE_TARGET_REACHED_RESET", False),
    ("env", "USE_TIP_LIMIT_HIT_RESET", False),
    ("env", "USE_NONZERO_CONTACT_FORCE_RESET", False),
    ("env", "CAPTURE_VIDEO", False),
    ("env", "RECORD_TRAJECTORIES", False),
    ("env", "EPISODE_LOG", False),
    ("env", "MAT_FILE", ""),
    ("env", "ENV_PARAMS_PER_EPISODE", False),      # a candidate keeps its plant: the table IS the search's population
    ("env", "ENV_PARAMS_ADR", {}),                 # ... and no range moves
    ("env", "ENV_SENSOR", {}),                     # ... and the fit reads the state as it is: no sensor model
    ("env", "ENV_PUSH", {}),                       # ... and nothing but the recorded commands moves a candidate
    ("env", "ENV_TARGET", {}),                     # ... and no target moves by itself
    ("env", "ENV_DRAW_ADR", {}),                   # ... and no range of those draws moves
)


def candidate_config(cfg, spec, num_envs, horizon, logger=None):
    """A copy of the task config ``cfg`` with what a candidate batch needs forced, each change logged: no randomisation and
    no noise (a candidate is a deterministic plant), free space (obstacle poses are not in a log), none of the three
    optional resets (the log's episode is not the candidates' to end), no observer, ``maxEpisodeLength`` > horizon, and
    ``spec`` as ``ENV_PARAMS`` so that a table is bound."""
    logger = logger or logging.getLogger(__name__)
    cfg = copy.deepcopy(cfg)
    cfg["task"].setdefault("randomization_parameters", {})
    for section, key, value in FORCED:
        node = cfg["task"] if section == "task" else cfg["task"]["randomization_parameters"] if section != "env" else cfg["env"]
        if node.get(key, value) != value:
            logger.info("sysid: %s.%s forced from %r to %r", section, key, node.get(key), value)
        node[key] = value
    if int(cfg["env"]["maxEpisodeLength"]) <= int(horizon) + 1:
        logger.info("sysid: env.maxEpisodeLength forced from %r to %d (> horizon)", cfg["env"]["maxEpisodeLength"], int(horizon) + 2)
        cfg["env"]["maxEpisodeLength"] = int(horizon) + 2
    if int(cfg["env"]["numEnvs"]) != int(num_envs):
        logger.info("sysid: env.numEnvs set to %d candidates", int(num_envs))
        cfg["env"]["numEnvs"] = int(num_envs)
    if not spec:
        raise ConfigError("sysid: the parameter spec is empty")
    cfg["env"]["ENV_PARAMS"] = copy.deepcopy(dict(spec))
    return cfg


def candidate_task(cfg, spec, num_envs, horizon, device="cuda:0", logger=None):
    from ..tasks import isaacgym_task_map
    cfg = candidate_config(cfg, spec, num_envs, horizon, logger)
    return isaacgym_task_map[cfg.get("name", "Vine5LinkMovingBase")](cfg=cfg, rl_device=device, sim_device=device,
                                                                    graphics_device_id=0, headless=True)


# --------------------------------------------------------------------------------------------------------- the search
def _seed_of(seed, iteration):
    return (int(seed) + int(iteration) * _GOLDEN) & 0xFFFFFFFFFFFFFFFF


def cem(evaluate, spec, base_row, num_envs, iterations, seed, elite_fraction=0.1, check=None, log=None, inertia=None):
    """Cross-entropy search over an ``ENV_PARAMS``-style ``spec`` (utils/env_params.py), host only.

    ``evaluate(table)`` takes a float32 table [VP_COUNT, num_envs] and returns one error per column (+inf allowed).
    ``base_row``: the configuration's own row (``env_params.config_row``).  ``check(table)``: called on every table before
    it is evaluated; by default ``vine_env_params_check`` of the product library.

    Iteration 0 is ``env_params.build_table``'s draw for ``seed``.  After every iteration the elites are the
    ``elite_fraction`` of the candidates with the smallest finite errors (two at least).  A ``[lo, hi]`` name is redrawn
    uniformly from the elites' mean +- 2 std, clipped to the initial range, with the table's own hash and the iteration
    mixed into the seed; a ``{values: [...]}`` name and ``ACTION_DELAY`` are redrawn from the elites' empirical values (the
    same hash picks one elite per env); a number stays.  Column 0 carries the best candidate so far, unchanged, from
    iteration 1 on, so the best error never increases.

    A spec that names ``CART_MASS``, ``LINK_MASS`` or ``TIP_LINK_MASS`` needs ``inertia = (base_row, derive, check)``: the
    configuration's own row of the inertia table (``env_params.inertia_config_row``), ``derive(table)`` returning the
    table with its derived rows filled and ``check(table)`` (``env_params.derive_inertia`` / ``check_inertia_table`` bound
    to a library and a configuration).  The inertia table [VI_COUNT, num_envs] is then carried beside the parameter table:
    the three names are drawn and redrawn by the rules above like any ``[lo, hi]`` / ``values`` name, column 0 keeps the
    best candidate's column of BOTH tables, every inertia table is derived and checked, and ``evaluate(table, inertia)``
    gets both.

    Returns ``(best_column, best_error, history)``: float32 [VP_COUNT], float, and one dict per iteration with
    ``best_error`` (so far), ``iteration_best``, ``finite`` (candidates with a finite error), ``ranges`` (name -> [lo, hi]
    drawn from) and ``counts`` (name -> {value: elites}); the last entry also holds the final population as ``table`` and
    ``errors``, and with an inertia table ``inertia`` (the final population's) and ``inertia_best`` (float32 [VI_COUNT])."""
    if check is None:
        from .. import native
        lib = native.load()

        def check(t):
            return env_params.check_table(lib, None, t)
    N, iterations = int(num_envs), int(iterations)
    if iterations < 1:
        raise ValueError("cem: at least one iteration")
    forms = env_params.spec_forms(spec)
    base = np.asarray(base_row, dtype=np.float32)
    masses = [name for name in forms if name in abi.ENV_INERTIA_NAMES]
    if masses and inertia is None:
        raise ValueError("cem: the spec names %s and needs inertia=(base_row, derive, check)" % ", ".join(masses))
    if masses:
        ibase, iderive, icheck = np.asarray(inertia[0], dtype=np.float32), inertia[1], inertia[2]
    itable, best_icol = None, None
    gids = np.arange(N, dtype=np.int64)
    initial = {name: (f[0], f[1]) for name, f in forms.items() if isinstance(f, list) and name != "ACTION_DELAY"}
    ranges = dict(initial)
    discrete = [name for name, f in forms.items() if isinstance(f, dict) or (name == "ACTION_DELAY" and isinstance(f, list))]
    draws = {}
    table = env_params.draw_table(spec, base, seed, N, check=check, draws=draws)
    if masses:
        itable = env_params.draw_inertia_table(spec, ibase, seed, N, iderive, check=icheck)
    best_col, best_draw, best_err = None, None, np.inf
    n_elite = min(N, max(2, int(np.ceil(float(elite_fraction) * N))))
    history = []
    for it in range(iterations):
        if it > 0:
            table = np.repeat(base[:, None], N, axis=1)
            s = _seed_of(seed, it)
            for name, f in forms.items():
                u = env_params.uniform01(s, name, gids)
                if not isinstance(f, (list, dict)):
                    v = np.full(N, f, dtype=np.float64)
                elif name in ranges:
                    lo, hi = ranges[name]
                    v = lo + (hi - lo) * u
                else:
                    pool = elite_values[name]
                    v = pool[np.minimum((u * len(pool)).astype(np.int64), len(pool) - 1)]
                if best_draw is not None:
                    v[0] = best_draw[name]
                draws[name] = v
                if name not in masses:
                    env_params.set_rows(table, base, name, v)
            if best_col is not None:
                table[:, 0] = best_col
            table = np.ascontiguousarray(table, dtype=np.float32)
            check(table)
            if masses:
                itable = np.repeat(ibase[:, None], N, axis=1)
                env_params.set_inertia_rows(itable, ibase, {name: draws[name] for name in masses})
                if best_icol is not None:
                    itable[:, 0] = best_icol
                itable = icheck(iderive(itable))
        err = np.asarray(evaluate(table, itable) if masses else evaluate(table), dtype=np.float64)
        if err.shape != (N,):
            raise ValueError("cem: evaluate returned %s, expected (%d,)" % (err.shape, N))
        err = np.where(np.isnan(err), np.inf, err)
        k = int(np.argmin(err))
        if err[k] < best_err or best_col is None:
            best_err, best_col = float(err[k]), table[:, k].copy()
            best_icol = itable[:, k].copy() if masses else None
            best_draw = {name: float(draws[name][k]) for name in forms}
        order = np.argsort(err, kind="stable")
        elites = order[:n_elite]
        elites = elites[np.isfinite(err[elites])]
        entry = {"iteration": it, "best_error": best_err, "iteration_best": float(err[k]),
                 "finite": int(np.isfinite(err).sum()),
                 "ranges": {name: [float(lo), float(hi)] for name, (lo, hi) in ranges.items()}, "counts": {}}
        elite_values = {}
        for name in discrete:
            pool = draws[name][elites] if len(elites) else draws[name]
            elite_values[name] = pool
            vals, cnt = np.unique(pool, return_counts=True)
            entry["counts"][name] = {float(a): int(b) for a, b in zip(vals, cnt)}
        if len(elites):
            for name in ranges:
                v = draws[name][elites]
                m, sd = float(v.mean()), float(v.std())
                lo0, hi0 = initial[name]
                ranges[name] = (min(max(m - 2.0 * sd, lo0), hi0), max(min(m + 2.0 * sd, hi0), lo0))
        history.append(entry)
        if log is not None:
            log(entry)
    history[-1]["table"], history[-1]["errors"] = table, err
    if masses:
        history[-1]["inertia"], history[-1]["inertia_best"] = itable, best_icol
    return best_col, best_err, history


def _describe(entry):
    parts = ["%s in [%.6g, %.6g]" % (n, lo, hi) for n, (lo, hi) in entry["ranges"].items()]
    parts += ["%s elites %s" % (n, ", ".join("%g x%d" % kv for kv in c.items())) for n, c in entry["counts"].items()]
    return "sysid iteration %d: best error %.9g (this iteration %.9g, %d finite)  %s" % (
        entry["iteration"], entry["best_error"], entry["iteration_best"], entry["finite"], "; ".join(parts))


def fit(cfg, log_path, spec, num_envs=4096, iterations=8, horizon=50, stride=25, seed=0, weights=None, directory=None,
        time_str=None, elite_fraction=0.1, device="cuda:0", logger=None):
    """Fit the parameters of ``spec`` to the log at ``log_path``: ``cfg`` is the task config (the ``task`` block of the
    composed configuration).  Builds the candidate batch (``candidate_config``), scores every ``cem`` table over the log's
    windows (``windows``), prints one line per iteration and the
    fitted values beside the configuration's, and writes ``<directory>/<time_str>_sysid.npz`` with ``best`` (the column),
    ``best_error``, ``env_param_names``, ``history`` (JSON), ``starts``, and the final population ``table`` with its
    ``errors``.  Returns a dict of the same.  Where ``spec`` names ``CART_MASS``, ``LINK_MASS`` or ``TIP_LINK_MASS`` the
    fitted masses and inertias are printed beside the configuration's too, and the dict and the file also hold ``inertia``
    (the final population's inertia table [VI_COUNT, N]), ``inertia_best`` (the best candidate's column) and
    ``env_inertia_names``."""
    logger = logger or logging.getLogger(__name__)
    weights = list(DEFAULT_WEIGHTS if weights is None else weights)
    log = load_log(log_path, weights)
    starts = windows(log, horizon, stride)
    if not starts:
        raise ValueError("sysid: no window of %d steps fits into one episode of %s (%d rows)" % (horizon, log_path, len(log)))
    task = candidate_task(cfg, spec, num_envs, horizon, device=device, logger=logger)
    try:
        ev = Evaluator(task, log, horizon, weights)
        base = env_params.config_row(task._lib, task._vcfg)
        names = list(task.env_param_names)
        seconds = [0.0]

        inames = list(task.env_inertia_names)
        with_masses = any(name in abi.ENV_INERTIA_NAMES for name in spec)
        ibase = env_params.inertia_config_row(task._lib, task._vcfg)

        def evaluate(table, itable=None):
            t0 = time.perf_counter()
            values = {names[p]: table[p] for p in range(abi.VP_COUNT)}
            if itable is not None:               # the eleven primary rows: the task derives the rest again and checks
                values.update({inames[r]: itable[r] for r in range(abi.VI_PRIMARY_COUNT)})
            task.set_env_params(values)                                                  # (checks the tables, then uploads)
            err = ev.evaluate(starts)
            seconds[0] += time.perf_counter() - t0
            return err

        print("sysid: %d candidates x %d windows of %d steps from %s (%d rows), %s" % (
            num_envs, len(starts), horizon, log_path, len(log), "hipGraph replay" if ev.use_graph else "eager steps"), flush=True)
        best, best_err, history = cem(evaluate, spec, base, num_envs, iterations, seed, elite_fraction,
                                      check=lambda t: env_params.check_table(task._lib, task._vcfg, t),
                                      log=lambda entry: print(_describe(entry), flush=True),
                                      inertia=(ibase, lambda t: env_params.derive_inertia(task._lib, task._vcfg, t),
                                               lambda t: env_params.check_inertia_table(task._lib, task._vcfg, t))
                                      if with_masses else None)
        for p in env_params.varying_rows(np.stack([best, base], axis=1)):
            print("sysid: %-26s fitted %-14.9g configuration %.9g" % (names[p], best[p], base[p]), flush=True)
        inertia_best = history[-1].pop("inertia_best", None)
        inertia = history[-1].pop("inertia", None)
        if inertia_best is not None:
            for r in env_params.varying_rows(np.stack([inertia_best, ibase], axis=1)[:abi.VI_PRIMARY_COUNT]):
                print("sysid: %-26s fitted %-14.9g configuration %.9g" % (inames[r], inertia_best[r], ibase[r]), flush=True)
        rate = num_envs * ev.steps_run / max(seconds[0], 1e-9)
        print("sysid: best error %.9g; %d candidate-steps in %.3f s (%.3g candidate-steps/s)" % (
            best_err, num_envs * ev.steps_run, seconds[0], rate), flush=True)
        final = history[-1]
        table, errors = final.pop("table"), final.pop("errors")
        out = {"best": best, "best_error": best_err, "env_param_names": names, "history": history, "starts": starts,
               "table": table, "errors": errors, "candidate_steps_per_second": rate, "path": None}
        more = {}
        if inertia is not None:
            more = {"inertia": inertia, "inertia_best": inertia_best, "env_inertia_names": np.array(inames)}
            out.update(more)
        if directory is not None:
            os.makedirs(directory, exist_ok=True)
            time_str = time_str or time.strftime("%Y-%m-%d_%H-%M-%S")
            path = os.path.join(directory, "%s_sysid.npz" % time_str)
            np.savez(path, best=best, best_error=np.float64(best_err), env_param_names=np.array(names),
                     history=np.array(json.dumps(history)), starts=np.asarray(starts, dtype=np.int64), table=table,
                     errors=errors, **more)
            out["path"] = path
            print("sysid: wrote %s" % path, flush=True)
        return out
    finally:
        task.close()
