"""EPISODE_LOG on the host side: the accumulators, totals and row ring of ``vine_episodes_scheduled``
(include/vine_episodes.h), the harvest, and the ``.npz`` file.

The rows are written on the device by a launch behind every step (any step entry point, both step kernels): one row per
finished episode of every env.  ``EpisodeLog`` is a step observer (the protocol: utils/observers.py).  Its harvest reads
the device cursor and copies the rows appended since the last one; that synchronises, so it runs where the host
synchronises anyway (once per training iteration, at the end of a player's run) and, inside a long run of steps, whenever
the worst case -- every env finishing every step -- could have filled half the ring since the last harvest.  Used through
the task class the ring can therefore never lap unharvested rows; ``dropped`` is kept, logged and stored all the same.

One file per run, ``<dir>/<time_str>_episodes.npz``: the rows sorted by (end step, env) as named columns, the folded
totals, ``dropped`` and the config keys that define the task.  ``load`` / ``report`` / ``binned_rate`` read it back."""
import functools
import logging
import math
import os

import numpy as np
import torch

from .. import abi, native

# the columns of a harvested row, in the order of the device's 16 words (include/vine_episodes.h); integer words as int64
COLUMNS = ("env", "end_step", "length", "return", "reached_ever", "reached_at_end", "first_reach", "final_dist", "min_dist",
           "end_reason", "target_y", "target_z", "obj_depth", "obj_angle")
INT_COLUMNS = ("env", "end_step", "end_reason")
TASK_KEYS = ("SUCCESS_DIST", "MIN_TARGET_DEPTH_IN_OBSTACLE", "MAX_TARGET_DEPTH_IN_OBSTACLE", "MIN_TARGET_Y", "MAX_TARGET_Y",
             "MIN_TARGET_Z", "MAX_TARGET_Z", "RANDOMIZE_TARGETS", "CREATE_SHELF", "CREATE_PIPE", "USE_TARGET_REACHED_RESET",
             "USE_TIP_LIMIT_HIT_RESET", "USE_NONZERO_CONTACT_FORCE_RESET", "maxEpisodeLength")


def episodes_config(lib, capacity):
    c = abi.VineEpisodesConfig()
    native.check(lib.vine_episodes_config_default(c), lib)
    c.capacity = int(capacity)
    return c


def dropped_rows(cursor, harvested, capacity):
    """Rows the writer lapped before they were copied: ``max(0, cursor - harvested - capacity)``."""
    return max(0, int(cursor) - int(harvested) - int(capacity))


def decode_rows(words):
    """``words[R, abi.EPISODES_WORDS]`` of 32-bit words as the device wrote them -> dict of columns (``COLUMNS``), sorted by
    (end step, env).  Float columns keep the device's bits (float32)."""
    w = np.ascontiguousarray(np.asarray(words).reshape(-1, abi.EPISODES_WORDS)).view(np.uint32)
    order = np.lexsort((w[:, abi.VEW_ENV].view(np.int32), w[:, abi.VEW_END_STEP].view(np.int32)))
    w = w[order]
    rows = {}
    for k, name in enumerate(COLUMNS):
        col = np.ascontiguousarray(w[:, k])
        rows[name] = col.view(np.int32).astype(np.int64) if name in INT_COLUMNS else col.view(np.float32).copy()
    return rows


def concat_rows(parts):
    """Several ``decode_rows`` results as one, sorted by (end step, env)."""
    parts = [p for p in parts if len(p["env"])]
    if not parts:
        return {name: np.zeros(0, dtype=np.int64 if name in INT_COLUMNS else np.float32) for name in COLUMNS}
    rows = {name: np.concatenate([p[name] for p in parts]) for name in COLUMNS}
    order = np.lexsort((rows["env"], rows["end_step"]))
    return {name: v[order] for name, v in rows.items()}


def totals_of(rows):
    """The twelve totals of ``vine_step_eval`` (abi.EVAL_*) from rows, summed in float64."""
    t = np.zeros(abi.EVAL_NUM_TOTALS, dtype=np.float64)
    f64 = lambda name: np.asarray(rows[name], dtype=np.float64)       # noqa: E731
    reason = np.asarray(rows["end_reason"], dtype=np.int64)
    t[abi.EVAL_EPISODES] = len(reason)
    t[abi.EVAL_RETURN_SUM] = f64("return").sum()
    t[abi.EVAL_LENGTH_SUM] = f64("length").sum()
    t[abi.EVAL_REACHED_EVER] = f64("reached_ever").sum()
    t[abi.EVAL_REACHED_AT_END] = f64("reached_at_end").sum()
    t[abi.EVAL_FIRST_REACH_SUM] = f64("first_reach").sum()
    t[abi.EVAL_FINAL_DIST_SUM] = f64("final_dist").sum()
    t[abi.EVAL_MIN_DIST_SUM] = f64("min_dist").sum()
    for col, bit in ((abi.EVAL_END_TIMEOUT, abi.EPISODES_END_TIMEOUT), (abi.EVAL_END_RAIL_LIMIT, abi.EPISODES_END_RAIL_LIMIT),
                     (abi.EVAL_END_TIP_LIMIT, abi.EPISODES_END_TIP_LIMIT), (abi.EVAL_END_CONTACT, abi.EPISODES_END_CONTACT)):
        t[col] = np.count_nonzero(reason & bit)
    return t


def report(rows):
    """The twelve ``player.REPORT_KEYS`` from rows: ``player.eval_report`` of the rows' totals."""
    from ..learning.player import eval_report
    return eval_report(totals_of(rows))


def binned_rate(rows, column, bins, of="reached_ever"):
    """The mean of the 0/1 column ``of`` over the episodes whose ``column`` falls into each bin: ``bins`` as for
    ``numpy.histogram`` (a count or the edges).  Returns (rate [B] with nan for an empty bin, count [B], edges [B + 1])."""
    x = np.asarray(rows[column], dtype=np.float64)
    y = np.asarray(rows[of], dtype=np.float64)
    count, edges = np.histogram(x, bins=bins)
    hit, _ = np.histogram(x, bins=edges, weights=y)
    with np.errstate(invalid="ignore", divide="ignore"):
        rate = np.where(count > 0, hit / count, np.nan)
    return rate, count, edges


def varying_params(table, names, inertia=None):
    """``{NAME: values [N]}``: one value per env of every parameter that varies across the envs.  ``table`` ([VP_COUNT, N],
    the bound per-env parameter table; ``names``: one per table row, ``abi.ENV_PARAM_ROW_NAMES``): the row's value, an FPAM
    vector reduced to joint 0's.  ``inertia`` ([VI_COUNT, N] or ``None``, the bound inertia table): ``CART_MASS`` = the
    cart's mass; ``LINK_MASS`` = link 0's mass, where it varies (one factor scales all five); ``TIP_LINK_MASS`` = link 4's
    mass, where its ratio to link 0's varies (the tip was scaled on its own).  All in kg."""
    t = np.asarray(table)
    out = {}
    for name, (first, count) in abi.ENV_PARAM_ROWS.items():
        if any(np.any(t[p] != t[p, 0]) for p in range(first, first + count)):
            assert names[first] == (name if count == 1 else name + "[0]"), (names[first], name)
            out[name] = t[first]
    if inertia is not None:
        m = np.asarray(inertia)
        cart, m0, m4 = m[abi.VI_CART_MASS], m[abi.VI_LINK_MASS0], m[abi.VI_LINK_MASS0 + abi.NUM_LINKS - 1]
        if np.any(cart != cart[0]):
            out["CART_MASS"] = cart
        if np.any(m0 != m0[0]):
            out["LINK_MASS"] = m0
        ratio = m4.astype(np.float64) / m0.astype(np.float64)
        if np.any(np.abs(ratio - ratio[0]) > 4e-7 * np.abs(ratio[0])):      # (beyond the rounding of two float32 masses)
            out["TIP_LINK_MASS"] = m4
    return out


def with_env_params(rows, table, names, inertia=None):
    """``rows`` with one more column per parameter that varies across the envs (``varying_params``): ``param_<NAME>`` = the
    value of the row's env.  ``binned_rate`` works on them like on any column."""
    env = np.asarray(rows["env"], dtype=np.int64)
    out = dict(rows)
    for name, values in varying_params(table, names, inertia).items():
        out["param_" + name] = values[env]
    return out


def episode_ordinals(env, end_step, episode_index):
    """The ordinal of the episode every row of ONE harvest ended, counted BACKWARDS from ``episode_index`` (int [N], the
    device's per-env episode counter copied at the same stream point as the cursor): the m harvested rows of env e, sorted by
    end step, are episodes ``c_e - m .. c_e - 1``.  That also holds where the ring dropped rows, because the survivors are
    each env's newest; counting forwards from the previous harvest would be off by the rows dropped."""
    env = np.asarray(env, dtype=np.int64)
    end = np.asarray(end_step, dtype=np.int64)
    c = np.asarray(episode_index, dtype=np.int64)
    order = np.lexsort((end, env))                                   # by env, then by end step
    e = env[order]
    first = np.r_[0, np.flatnonzero(e[1:] != e[:-1]) + 1] if len(e) else np.zeros(0, dtype=np.int64)
    count = np.diff(np.r_[first, len(e)])
    rank = np.arange(len(e)) - np.repeat(first, count)                # 0 .. m - 1 within the env
    out = np.empty(len(e), dtype=np.int64)
    out[order] = c[e] - np.repeat(count, count) + rank
    return out


def with_episode_params(rows, params, names, inertia=None):
    """``rows`` with ``param_<NAME>`` per parameter that varies across the ROWS: ``params`` [VP_COUNT, R] (``inertia``
    [VI_COUNT, R] or ``None``) hold the column every row's episode ran with (``env_params.draw_columns`` of the rows' env and
    ``episode``), reduced as ``varying_params`` reduces a table.  The rates then bin by episode, not by env."""
    out = dict(rows)
    if len(np.asarray(rows["env"])):
        for name, values in varying_params(params, names, inertia).items():
            out["param_" + name] = values
    return out


def drawn_at(env, episode, end_step):
    """ENV_PARAMS_ADR: the index of the step whose launch drew every row's episode, int64 [R]: the end step of the SAME env's
    row of the episode before it.  -1 for episode 0 (drawn by nobody: START's table) and where that row is not among the
    rows (the ring dropped it): the range in force when the episode was drawn is then unknown."""
    env = np.asarray(env, dtype=np.int64)
    k = np.asarray(episode, dtype=np.int64)
    end = np.asarray(end_step, dtype=np.int64)
    out = np.full(len(env), -1, dtype=np.int64)
    order = np.lexsort((k, env))
    e, ks = env[order], k[order]
    has = np.r_[False, (e[1:] == e[:-1]) & (ks[1:] == ks[:-1] + 1)] if len(e) else np.zeros(0, dtype=bool)
    out[order[has]] = end[order[np.flatnonzero(has) - 1]]
    return out


def with_adr_params(rows, columns):
    """ENV_PARAMS_ADR: ``rows`` (with ``episode``) with ``param_<NAME>`` per parameter that varies across the rows and the
    ``probe`` column (the boundary ``2 * slot + side`` the episode was pinned to, -1: none, -2: unknown).  ``columns(envs,
    episodes, drawn_at)`` -> ``(params, inertia or None, probe)``.  A row whose predecessor was dropped has NaN parameters;
    ``(rows, unknown)`` with ``unknown`` their number."""
    out = dict(rows)
    if not len(np.asarray(rows["env"])):
        out["probe"] = np.zeros(0, dtype=np.int64)
        return out, 0
    at = drawn_at(rows["env"], rows["episode"], rows["end_step"])
    params, inertia, probe = columns(rows["env"], rows["episode"], at)
    out = with_episode_params(rows, params, abi.ENV_PARAM_ROW_NAMES, inertia)
    out["probe"] = probe
    return out, int(np.count_nonzero(probe == -2))


def value_rate(rows, column, of="reached_ever"):
    """The mean of the 0/1 column ``of`` over the episodes of each distinct value of ``column``: (values [V] ascending,
    rate [V], count [V])."""
    x = np.asarray(rows[column], dtype=np.float64)
    y = np.asarray(rows[of], dtype=np.float64)
    values, inverse, count = np.unique(x, return_inverse=True, return_counts=True)
    hit = np.bincount(inverse, weights=y, minlength=len(values))
    return values, hit / np.maximum(count, 1), count


DRAW_OBSERVERS = ("sensor", "push", "target")      # the observers with a table of named draws, in the order their columns join


def with_draw_params(rows, draw_params):
    """``rows`` with the ``param_<DRAW NAME>`` columns of one observer's named draws (ENV_SENSOR: ``param_SENSOR_DELAY`` / ``_HOLD``
    / ``_NOISE_STD``; ENV_PUSH: ``param_PUSH_RATE`` / ``_IMPULSE``; ENV_TARGET: ``param_TARGET_VEL_ALONG`` .. ``_SPAN_ACROSS``) for
    the names that vary.  ``draw_params(envs, episodes)`` -> ``{DRAW NAME: values [R]}`` (``named_draw.episode_params``: held
    values are joined by env, per-episode ones by the row's ``episode``, the join ``param_<NAME>`` uses under
    ENV_PARAMS_PER_EPISODE)."""
    out = dict(rows)
    if len(np.asarray(rows["env"])):
        episodes_ = rows["episode"] if "episode" in rows else np.zeros(len(rows["env"]), dtype=np.int64)
        for name, values in draw_params(rows["env"], episodes_).items():
            out["param_" + name] = values
    return out


def with_draw_adr_params(rows, episode_params):
    """ENV_DRAW_ADR: ``rows`` (with ``episode``) with the ``param_<DRAW NAME>`` column of every name under ADR, from the range
    in force at the step that drew the row's episode (in the place of the observer's own join, which knows the limits only),
    and the ``draw_probe`` column (the boundary ``2 * slot + side`` the episode was pinned to, -1: none, -2: unknown).
    ``episode_params(envs, episodes, drawn_at)`` -> ``({DRAW NAME: values [R]}, probe [R])``
    (``env_draw_adr.draw_adr_episode_params``).  A row whose predecessor was dropped is NaN; ``(rows, unknown)`` with
    ``unknown`` their number."""
    out = dict(rows)
    if not len(np.asarray(rows["env"])):
        out["draw_probe"] = np.zeros(0, dtype=np.int64)
        return out, 0
    params, probe = episode_params(rows["env"], rows["episode"], drawn_at(rows["env"], rows["episode"], rows["end_step"]))
    for name, values in params.items():
        out["param_" + name] = values
    out["draw_probe"] = probe
    return out, int(np.count_nonzero(probe == -2))


def save(path, rows, totals, dropped, task, env_params=None, env_param_names=None, env_inertia=None, env_inertia_names=None,
         redraw=None, adr=None, sensor=None, push=None, target=None, draw_adr=None):
    """Rows as named columns, the folded totals, ``dropped`` and the task's keys (``task_<KEY>``), written beside the path
    and renamed.  With a bound per-env parameter table also ``env_params`` [VP_COUNT, N] and ``env_param_names``, with a
    bound inertia table ``env_inertia`` [VI_COUNT, N] and ``env_inertia_names``.  With ENV_PARAMS_PER_EPISODE (``redraw``: a
    dict of ``spec``, ``seed``, ``env_id_offset``, ``base``, ``inertia_base``, ``geometry``) the rows' ``episode`` column and
    what ``load_env_redraw`` needs to rebuild every episode's column without a device; the two tables are then the plants
    at the moment of writing.  With ENV_PARAMS_ADR also ``adr``: a dict of ``config`` (``env_params.adr_config``'s result),
    ``history`` [H, 4] (complete), ``history_dropped`` and ``widen0`` [VR_NAMES, 2] (the ``widen`` in force before the run's
    first step: zeros, or a restored checkpoint's).  With ENV_SENSOR, ENV_PUSH or ENV_TARGET (``sensor``, ``push``, ``target``: each a
    dict of ``spec``, ``seed`` and ``env_id_offset``) what ``load_env_draw`` needs to rebuild the ``param_SENSOR_*``,
    ``param_PUSH_*`` and ``param_TARGET_*`` columns without a device, and, where the rows carry one, their ``episode`` column.
    With ENV_DRAW_ADR also ``draw_adr``: a dict of ``config`` (``env_draw_adr.draw_adr_config``'s result), ``history`` [H, 4]
    (complete), ``history_dropped``, ``widen0`` [9, 2], ``seed`` and ``env_id_offset``: what ``load_env_draw_adr`` needs."""
    out = {name: np.asarray(rows[name]) for name in COLUMNS}
    for prefix, draw in (("target", target), ("push", push), ("sensor", sensor)):
        if draw is not None:
            import json
            out[prefix + "_spec"] = np.array(json.dumps(draw["spec"]))
            out[prefix + "_seed"] = np.array(int(draw["seed"]), dtype=np.uint64)
            out[prefix + "_env_id_offset"] = np.array(int(draw["env_id_offset"]), dtype=np.int64)
            if "episode" in rows:
                out["episode"] = np.asarray(rows["episode"], dtype=np.int64)
    if draw_adr is not None:
        import json
        out["draw_adr_config"] = np.array(json.dumps(draw_adr["config"]))
        out["draw_adr_history"] = np.asarray(draw_adr["history"], dtype=np.int64).reshape(-1, 4)
        out["draw_adr_history_dropped"] = np.array(int(draw_adr["history_dropped"]), dtype=np.int64)
        out["draw_adr_widen0"] = np.asarray(draw_adr["widen0"], dtype=np.int64).reshape(abi.VDA_NAMES, 2)
        out["draw_adr_seed"] = np.array(int(draw_adr["seed"]), dtype=np.uint64)
        out["draw_adr_env_id_offset"] = np.array(int(draw_adr["env_id_offset"]), dtype=np.int64)
    if adr is not None:
        import json
        out["adr_config"] = np.array(json.dumps(adr["config"]))
        out["adr_history"] = np.asarray(adr["history"], dtype=np.int64).reshape(-1, 4)
        out["adr_history_dropped"] = np.array(int(adr["history_dropped"]), dtype=np.int64)
        out["adr_widen0"] = np.asarray(adr.get("widen0", np.zeros((abi.VR_NAMES, 2))), dtype=np.int64).reshape(abi.VR_NAMES, 2)
    if redraw is not None:
        import json
        out["episode"] = np.asarray(rows["episode"], dtype=np.int64)
        out["redraw_spec"] = np.array(json.dumps(redraw["spec"]))
        out["redraw_seed"] = np.array(int(redraw["seed"]), dtype=np.uint64)
        out["redraw_env_id_offset"] = np.array(int(redraw["env_id_offset"]), dtype=np.int64)
        out["redraw_base"] = np.asarray(redraw["base"], dtype=np.float32)
        out["redraw_inertia_base"] = np.asarray(redraw["inertia_base"], dtype=np.float32)
        out["redraw_geometry"] = np.asarray(redraw["geometry"], dtype=np.float32)      # link_length, link_com, gravity
    if env_params is not None:
        out["env_params"] = np.asarray(env_params, dtype=np.float32)
        out["env_param_names"] = np.array(list(env_param_names))
    if env_inertia is not None:
        out["env_inertia"] = np.asarray(env_inertia, dtype=np.float32)
        out["env_inertia_names"] = np.array(list(env_inertia_names))
    out["totals"] = np.asarray(totals, dtype=np.float64).reshape(-1, abi.EVAL_NUM_TOTALS).sum(axis=0)
    out["dropped"] = np.array(int(dropped), dtype=np.int64)
    for k, v in task.items():
        out["task_" + k] = np.asarray(v)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    part = path + ".part.npz"
    np.savez(part, **out)                  # not compressed: a player's run() ends here, with millions of rows
    os.replace(part, path)
    return path


def load(path):
    """``(rows, totals[12], dropped, task)`` of a file written by ``save``."""
    with np.load(path) as z:
        rows = {name: z[name] for name in COLUMNS}
        task = {k[5:]: z[k][()] for k in z.files if k.startswith("task_")}
        return rows, z["totals"], int(z["dropped"]), task


def load_env_params(path):
    """``(table [VP_COUNT, N], names)`` of a file written with a bound per-env parameter table, else ``(None, None)``."""
    with np.load(path) as z:
        if "env_params" not in z.files:
            return None, None
        return z["env_params"], [str(n) for n in z["env_param_names"]]


def load_env_inertia(path):
    """``(table [VI_COUNT, N], names)`` of a file written with a bound inertia table, else ``(None, None)``."""
    with np.load(path) as z:
        if "env_inertia" not in z.files:
            return None, None
        return z["env_inertia"], [str(n) for n in z["env_inertia_names"]]


def _redraw_of(path):
    """What ``load_env_redraw`` and ``load_env_adr`` read of a file written under ENV_PARAMS_PER_EPISODE, else ``None``."""
    import ctypes as C
    import json
    from . import env_params
    with np.load(path) as z:
        if "redraw_spec" not in z.files:
            return None
        r = {"spec": json.loads(str(z["redraw_spec"][()])), "seed": int(z["redraw_seed"]), "offset": int(z["redraw_env_id_offset"]),
             "base": z["redraw_base"], "inertia_base": z["redraw_inertia_base"], "episode": z["episode"], "adr": None}
        geometry = z["redraw_geometry"]
        if "adr_config" in z.files:
            r.update(adr=json.loads(str(z["adr_config"][()])), history=z["adr_history"], dropped=int(z["adr_history_dropped"]),
                     widen0=z["adr_widen0"] if "adr_widen0" in z.files else None)

    def derive(t):
        lib = native.load()
        vcfg = abi.VineConfig()
        native.check(lib.vine_config_default(C.byref(vcfg)), lib)
        vcfg.link_length, vcfg.link_com, vcfg.gravity = (float(g) for g in geometry)
        return env_params.derive_inertia(lib, vcfg, t)
    r["derive"] = derive
    return r


def load_env_redraw(path):
    """Of a file written under ENV_PARAMS_PER_EPISODE: ``(episode [R], columns)`` with ``columns(envs, episodes)`` ->
    ``(params [VP_COUNT, M], inertia [VI_COUNT, M] or None)``, ``env_params.draw_columns`` rebuilt from the stored spec, seed,
    ``env_id_offset`` and base rows (host code of the library only, no device); else ``(None, None)``.  A file written under
    ENV_PARAMS_ADR gives its ``episode`` too, but its ``columns`` raises: a plant there also depends on the step that drew it,
    and ``load_env_adr`` is its reader."""
    from . import env_params
    r = _redraw_of(path)
    if r is None:
        return None, None

    def columns(envs, episodes_):
        if r["adr"] is not None:
            raise ValueError("%s was written under ENV_PARAMS_ADR: an episode's plant also depends on the range in force when it "
                             "was drawn; read it with load_env_adr or load_rows_with_params" % path)
        return env_params.draw_columns(r["spec"], r["base"], r["inertia_base"], r["derive"], r["seed"],
                                       np.asarray(envs, dtype=np.int64) + r["offset"], episodes_)
    return r["episode"], columns


def load_env_adr(path):
    """Of a file written under ENV_PARAMS_ADR: ``(config, history [H, 4], history_dropped, widen0 [VR_NAMES, 2], columns)`` with
    ``columns(envs, episodes, drawn_at)`` -> ``(params [VP_COUNT, M], inertia [VI_COUNT, M] or None, probe [M])``,
    ``env_params.adr_episode_columns`` rebuilt from what the file stores (float64, NaN and probe -2 where ``drawn_at`` is -1;
    ``drawn_at``: this module's); else ``(None, None, 0, None, None)``."""
    from . import env_params
    r = _redraw_of(path)
    if r is None or r["adr"] is None:
        return None, None, 0, None, None
    widen0 = r["widen0"] if r["widen0"] is not None else np.zeros((abi.VR_NAMES, 2), dtype=np.int64)

    def columns(envs, episodes_, drawn_at_):
        return env_params.adr_episode_columns(r["spec"], r["adr"], r["seed"], np.asarray(envs, dtype=np.int64) + r["offset"], episodes_,
                                              drawn_at_, r["history"], base=r["base"], inertia_base=r["inertia_base"],
                                              derive=r["derive"], widen0=widen0)
    return r["adr"], r["history"], r["dropped"], widen0, columns


def load_env_draw(path, prefix):
    """Of a file written under ENV_SENSOR, ENV_PUSH or ENV_TARGET (``prefix``: one of ``DRAW_OBSERVERS``): ``(spec, episode [R]
    or None, draw_params)`` with ``draw_params(envs, episodes)`` -> the ``episode_params`` of utils/env_<prefix>.py rebuilt
    from the stored spec, seed and ``env_id_offset`` (no device); else ``(None, None, None)``."""
    import importlib
    import json
    module = importlib.import_module(".env_" + prefix, __package__)
    with np.load(path) as z:
        if prefix + "_spec" not in z.files:
            return None, None, None
        spec, seed, offset = json.loads(str(z[prefix + "_spec"][()])), int(z[prefix + "_seed"]), int(z[prefix + "_env_id_offset"])
        episode = z["episode"] if "episode" in z.files else None

    def draw_params(envs, episodes_):
        return module.episode_params(spec, seed, np.asarray(envs, dtype=np.int64) + offset, episodes_)
    return spec, episode, draw_params


def load_env_draw_adr(path):
    """Of a file written under ENV_DRAW_ADR: ``(config, history [H, 4], history_dropped, widen0 [9, 2], episode_params)`` with
    ``episode_params(envs, episodes, drawn_at)`` -> ``({DRAW NAME: values [M]}, probe [M])``,
    ``env_draw_adr.draw_adr_episode_params`` rebuilt from what the file stores (no device; NaN and probe -2 where ``drawn_at``
    is -1); else ``(None, None, 0, None, None)``."""
    import json
    from . import env_draw_adr
    with np.load(path) as z:
        if "draw_adr_config" not in z.files:
            return None, None, 0, None, None
        config, history, widen0 = json.loads(str(z["draw_adr_config"][()])), z["draw_adr_history"], z["draw_adr_widen0"]
        dropped, seed, offset = int(z["draw_adr_history_dropped"]), int(z["draw_adr_seed"]), int(z["draw_adr_env_id_offset"])

    def episode_params(envs, episodes_, drawn_at_):
        return env_draw_adr.draw_adr_episode_params(config, seed, np.asarray(envs, dtype=np.int64) + offset, episodes_, drawn_at_,
                                                    history, widen0)
    return config, history, dropped, widen0, episode_params


# the names the join and the loader had while each of the three observers had its own: files and callers written then still work
with_sensor_params = with_push_params = with_target_params = with_draw_params
load_env_sensor = functools.partial(load_env_draw, prefix="sensor")
load_env_push = functools.partial(load_env_draw, prefix="push")
load_env_target = functools.partial(load_env_draw, prefix="target")


def load_rows_with_params(path):
    """The rows of a file written under ENV_PARAMS_PER_EPISODE with the ``param_<NAME>`` columns of every row's own episode
    (and ``episode``; under ENV_PARAMS_ADR also ``probe``), as ``EpisodeLog.rows_with_params`` gives them; no device.  Under
    ENV_SENSOR, ENV_PUSH and ENV_TARGET also the ``param_SENSOR_*``, ``param_PUSH_*`` and ``param_TARGET_*`` columns; under
    ENV_DRAW_ADR those of the names under ADR from the range in force, and ``draw_probe``."""
    rows = _load_rows_with_plant_params(path)
    for prefix in DRAW_OBSERVERS:
        _, episode, params = load_env_draw(path, prefix)
        if params is None:
            continue
        if episode is not None:
            rows["episode"] = episode
        rows = with_draw_params(rows, params)
    draw_adr_params = load_env_draw_adr(path)[4]
    if draw_adr_params is not None:                  # ENV_DRAW_ADR: the names under ADR from the range in force, and draw_probe
        rows = with_draw_adr_params(rows, draw_adr_params)[0]
    return rows


def _load_rows_with_plant_params(path):
    episode, columns = load_env_redraw(path)
    rows = dict(load(path)[0])
    if episode is None:
        return rows
    rows["episode"] = episode
    adr_columns = load_env_adr(path)[4]
    if adr_columns is not None:
        return with_adr_params(rows, adr_columns)[0]
    params, inertia = columns(rows["env"], episode) if len(episode) else (None, None)
    return with_episode_params(rows, params, abi.ENV_PARAM_ROW_NAMES, inertia)


class EpisodeLog:
    """The device buffers of one env handle's episode log, the host's count of steps since the last harvest, and the
    harvest.  A step observer (the protocol: utils/observers.py); not windowed, so its harvest is its own."""

    def __init__(self, lib, handle, num_envs, capacity, with_table, buffers, device, directory, time_str, task, logger=None):
        """``buffers``: the step's output tensors ``(rew, reset, progress, timeouts)``.  A reward matrix must already be
        bound to ``handle``."""
        self.lib, self.handle, self.device, self.num_envs = lib, handle, device, int(num_envs)
        self.logger = logger or logging.getLogger(__name__)
        self.ecfg = episodes_config(lib, capacity)
        self.capacity = int(capacity)
        nbytes = int(lib.vine_episodes_table_bytes(self.ecfg))
        if nbytes < 0:
            native.check(nbytes, lib)
        rows = int(lib.vine_episodes_rows(handle))
        if rows < 0:
            native.check(rows, lib)
        self.rew, self.reset, self.progress, self.timeouts = buffers
        self.episode = torch.zeros((abi.EVAL_EPISODE_FIELDS, self.num_envs), dtype=torch.float32, device=device)
        self.episode[abi.EVAL_EP_MIN_DIST].fill_(math.inf)
        self.totals = torch.zeros((rows, abi.EVAL_NUM_TOTALS), dtype=torch.float64, device=device)
        self.table = self.cursor = None
        if with_table:
            self.table = torch.zeros((self.capacity, abi.EPISODES_WORDS), dtype=torch.int32, device=device)
            assert self.table.numel() * 4 == nbytes
            self.cursor = torch.zeros(1, dtype=torch.int64, device=device)
        self.path = os.path.join(directory, f"{time_str}_episodes.npz")
        self.task = dict(task)
        self.harvested = 0           # the cursor at the last harvest
        self.dropped = 0
        self.pending = 0             # steps enqueued since the last harvest
        self.parts = []              # harvested rows as the device wrote them, in harvest order
        self._rows = None            # the same decoded and sorted, until the next harvest adds to them
        self.paused = 0
        self.copy_done = None        # (the harvest is synchronous: no copy is ever in flight)
        self.env_params_of, self.env_param_names = None, None      # ENV_PARAMS: set by the task class when a table is bound
        self.env_inertia_of, self.env_inertia_names = None, None   # ENV_INERTIA: likewise
        self.redraw = None           # ENV_PARAMS_PER_EPISODE: the task's ``env_redraw.EnvRedraw``; rows then carry ``episode``
        self.part_counters = []      # ... and every harvested part the device's episode_index at its harvest
        self.unknown_plants = 0      # ENV_PARAMS_ADR: rows of the last rows_with_params() whose plant is unknown (NaN)
        self.sensor = None           # ENV_SENSOR: the task's ``env_sensor.EnvSensor``; under its PER_EPISODE rows carry ``episode``
        self.push = None             # ENV_PUSH: the task's ``env_push.EnvPush``; likewise
        self.target = None           # ENV_TARGET: the task's ``env_target.EnvTarget``; likewise (the three of DRAW_OBSERVERS)
        self.draw_adr = None         # ENV_DRAW_ADR: the task's ``env_draw_adr.EnvDrawAdr``
        self.unknown_draws = 0       # ... and the rows of the last rows_with_params() whose range in force is unknown (NaN)

    def live_tensors(self):
        """What a caller that rolls steps back (the warm-up pass in front of a graph capture) must save and restore.  The
        ring is not among them: rows are harvested first, and what the rolled-back pass appends lies past the restored
        cursor, where later rows overwrite it."""
        self.harvest()
        return [self.episode, self.totals] + ([self.cursor] if self.cursor is not None else [])

    # -- device side -------------------------------------------------------------------------------------------------
    def enqueue(self, stream, actions=None):
        """The accounting of the step just enqueued on ``stream`` (captured with it inside a hipGraph)."""
        native.check(self.lib.vine_episodes_scheduled(
            self.handle, self.ecfg, self.rew.data_ptr(), self.reset.data_ptr(), self.progress.data_ptr(),
            self.timeouts.data_ptr(), self.episode.data_ptr(), self.totals.data_ptr(),
            self.table.data_ptr() if self.table is not None else None,
            self.cursor.data_ptr() if self.cursor is not None else None, stream), self.lib)

    def _counters(self):
        """Who counts the episodes of every env on the device: the redraw, else the first of the sensor, the push and the
        target that is redrawn per episode (all that are on count alike), else nobody."""
        if self.redraw is not None:
            return self.redraw
        for observer in (self.sensor, self.push, self.target):
            if observer is not None and observer.spec["PER_EPISODE"]:
                return observer
        return None

    def reset_envs(self, env_ids):
        """The envs were reset from outside the step: their running episode is discarded without a row."""
        self.episode[:, env_ids] = torch.tensor([0.0, 0.0, math.inf, 0.0], device=self.device).unsqueeze(1)

    # -- host side ---------------------------------------------------------------------------------------------------
    def set_steps(self, steps):
        pass                         # the end step of a row is the device's own count

    def _room(self, n_steps):
        """Could ``n_steps`` more steps, every env finishing in each, pass half the ring?"""
        return self.num_envs * (self.pending + int(n_steps)) > self.capacity // 2

    def before(self, n_steps):
        if self.paused or self.table is None or torch.cuda.is_current_stream_capturing():
            return
        if self.pending and self._room(n_steps):
            self.harvest()

    def advance(self, n_steps):
        if not self.paused:
            self.pending += int(n_steps)

    def harvest(self):
        """Copy the rows appended since the last harvest (synchronises with the device).  Returns their number."""
        self.pending = 0
        if self.table is None or torch.cuda.is_current_stream_capturing():
            return 0
        cursor = int(self.cursor.item())
        lost = dropped_rows(cursor, self.harvested, self.capacity)
        if lost:
            self.dropped += lost
            self.logger.warning(f"EPISODE_LOG: {lost} rows were overwritten before they were harvested "
                                f"({self.dropped} in all): raise EPISODE_LOG_CAPACITY")
        first = max(self.harvested, cursor - self.capacity)
        self.harvested = cursor
        if cursor == first:
            return 0
        a, b = first % self.capacity, (cursor - 1) % self.capacity + 1
        words = self.table[a:b] if a < b else torch.cat([self.table[a:], self.table[:b]])
        self.parts.append(words.cpu().numpy())       # decoded and sorted when somebody asks for rows
        if self._counters() is not None:             # the same stream point as the cursor: nothing was enqueued in between
            self.part_counters.append(self._counters().episodes_now())
            if hasattr(self.redraw, "harvest_history"):      # ENV_PARAMS_ADR: and the moves of the ranges up to here
                self.redraw.harvest_history()
            if self.draw_adr is not None:                    # ENV_DRAW_ADR: likewise
                self.draw_adr.harvest_history()
        self._rows = None
        return cursor - first

    def rows(self):
        """Every harvested row so far, sorted by (end step, env)."""
        if self._rows is None and self._counters() is not None:
            parts = []
            for words, counters in zip(self.parts, self.part_counters):      # ordinals count back from each harvest's counters
                part = decode_rows(words)
                part["episode"] = episode_ordinals(part["env"], part["end_step"], counters)
                parts.append(part)
            if parts:
                rows = {name: np.concatenate([p[name] for p in parts]) for name in COLUMNS + ("episode",)}
            else:
                rows = dict(concat_rows([]), episode=np.zeros(0, dtype=np.int64))
            order = np.lexsort((rows["env"], rows["end_step"]))
            self._rows = {name: v[order] for name, v in rows.items()}
        elif self._rows is None:
            if len(self.parts) > 1:
                self.parts = [np.concatenate(self.parts)]
            self._rows = decode_rows(self.parts[0]) if self.parts else concat_rows([])
        return self._rows

    def rows_with_params(self):
        """``rows()`` with ``param_<NAME>`` columns: under ENV_PARAMS_PER_EPISODE the plant of every row's episode
        (``with_episode_params`` of ``draw_columns(env, episode)``), else the bound table's column of its env.  Under
        ENV_SENSOR also ``param_SENSOR_*``, under ENV_PUSH ``param_PUSH_*``, under ENV_TARGET ``param_TARGET_*``
        (``with_draw_params``); under ENV_DRAW_ADR the names under ADR from the range in force, and ``draw_probe``
        (``with_draw_adr_params``)."""
        out = self._rows_with_plant_params()
        for observer in (self.sensor, self.push, self.target):
            if observer is not None:
                out = with_draw_params(out, observer.episode_params)
        if self.draw_adr is not None:                # ENV_DRAW_ADR: the range in force when the episode was drawn
            self.draw_adr.harvest_history()
            out, self.unknown_draws = with_draw_adr_params(out, self.draw_adr.episode_params)
            if self.unknown_draws:
                self.logger.info(f"EPISODE_LOG: {self.unknown_draws} rows have no known draw range (the row of the episode before "
                                 f"them was dropped)")
        return out

    def _rows_with_plant_params(self):
        rows = self.rows()
        if getattr(self.redraw, "adr", None) is not None:      # ENV_PARAMS_ADR: the range in force when the episode was drawn
            self.redraw.harvest_history()
            out, self.unknown_plants = with_adr_params(rows, self.redraw.episode_columns)
            if self.unknown_plants:
                self.logger.info(f"EPISODE_LOG: {self.unknown_plants} rows have no known plant (the row of the episode before "
                                 f"them was dropped)")
            return out
        if self.redraw is not None:
            params, inertia = self.redraw.columns(rows["env"], rows["episode"]) if len(rows["env"]) else (None, None)
            return with_episode_params(rows, params, self.env_param_names, inertia)
        if self.env_params_of is None:
            return dict(rows)
        inertia = self.env_inertia_of(range(self.num_envs)) if self.env_inertia_of is not None else None
        return with_env_params(rows, self.env_params_of(range(self.num_envs)), self.env_param_names, inertia)

    def folded_totals(self):
        """The twelve totals, folded over the workgroups' rows in float64 on the host (synchronises)."""
        return self.totals.cpu().numpy().sum(axis=0)

    def drain(self):
        """Harvest what is left and (re)write the file."""
        self.harvest()
        table = self.env_params_of(range(self.num_envs)) if self.env_params_of is not None else None
        inertia = self.env_inertia_of(range(self.num_envs)) if self.env_inertia_of is not None else None
        redraw = None
        if self.redraw is not None:
            from . import env_params
            r = self.redraw
            redraw = {"spec": r.spec, "seed": r.seed, "env_id_offset": r.env_id_offset,
                      "base": env_params.config_row(r.lib, r.vcfg), "inertia_base": env_params.inertia_config_row(r.lib, r.vcfg),
                      "geometry": (r.vcfg.link_length, r.vcfg.link_com, r.vcfg.gravity)}
        adr = None
        if getattr(self.redraw, "adr", None) is not None:
            adr = {"config": self.redraw.adr, "history": self.redraw.harvest_history(), "history_dropped": self.redraw.history_dropped,
                   "widen0": self.redraw.widen0}
        sensor, push, target = (None if o is None else {"spec": o.spec, "seed": o.seed, "env_id_offset": o.env_id_offset}
                                for o in (self.sensor, self.push, self.target))
        draw_adr = None
        if self.draw_adr is not None:
            d = self.draw_adr
            draw_adr = {"config": d.adr, "history": d.harvest_history(), "history_dropped": d.history_dropped, "widen0": d.widen0,
                        "seed": d.seed, "env_id_offset": d.env_id_offset}
        save(self.path, self.rows(), self.folded_totals(), self.dropped, self.task, table, self.env_param_names, inertia,
             self.env_inertia_names, redraw, adr, sensor, push, target, draw_adr)
        self.logger.info(f"EPISODE_LOG: {len(self.rows()['env'])} episodes -> {self.path}")

    def close(self):
        pass
