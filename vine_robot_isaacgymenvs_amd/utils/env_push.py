"""ENV_PUSH on the host side: the configuration, the draw of an env's two push values, the numpy statement of the launch
behind every step (``push_replay``: what every GPU test compares against) and the step observer (``EnvPush``).  The semantics
are stated once, in include/vine_env_push.h.

``task.env.ENV_PUSH`` (``{}``: off) maps

  ``RATE``         probability per control step that the env is pushed, [0, 1]
  ``IMPULSE``      largest impulse component in N s, >= 0
                   each a number, ``[lo, hi]`` or ``{values: [...]}``
  ``POINTS``       a non-empty list without duplicates of point indices 0 .. 5: 0 the cart, m the distal end of link m - 1,
                   5 the tip (default ``[5]``)
  ``PER_EPISODE``  False: every env's two values are drawn once and held; True: redrawn on the device at every reset

What env ``g`` gets in episode ``k`` is the named draw (utils/named_draw.py) under the names ``PUSH_RATE`` and
``PUSH_IMPULSE``, keyed by the GLOBAL env id: a rank's shard draws what the whole batch would."""
import ctypes as C

import numpy as np

from .. import abi, native
from . import env_params, named_draw
from .config import ConfigError
from .named_draw import candidates, philox4x32_10
from .observers import TableObserver

_KEY = "task.env.ENV_PUSH"
NAMES = tuple(abi.ENV_PUSH_NAMES)                    # the table's rows, the order of the mixed radix
DRAW_NAMES = tuple("PUSH_" + n for n in NAMES)       # the names the draw is keyed by, and of the log's param_ columns
NL = abi.NUM_LINKS
ND = NL + 1


# ---- configuration
def _check_values(name, form):
    where = "%s.%s" % (_KEY, name)
    for v in candidates(form):
        if name == "RATE" and not 0.0 <= v <= 1.0:
            raise ConfigError("%s: %g lies outside [0, 1]" % (where, v))
        if name == "IMPULSE" and not v >= 0.0:
            raise ConfigError("%s: %g is negative" % (where, v))


def push_config(env_cfg):
    """The checked ``task.env.ENV_PUSH`` of the ``task.env`` mapping as plain numbers and lists, ``None`` when it is empty
    (off): ``{"RATE", "IMPULSE"`` (a number, ``[lo, hi]`` or ``{"values": [..]}``), ``"POINTS"`` (list of point indices, in the
    order given: the draw indexes it), ``"PER_EPISODE"}``.  ``ConfigError``, naming the key, for everything
    include/vine_env_push.h refuses."""
    cfg = env_cfg.get("ENV_PUSH") or {}
    if not hasattr(cfg, "keys"):
        raise ConfigError("%s must be a mapping, not %r" % (_KEY, cfg))
    if not len(cfg):
        return None
    unknown = sorted(set(cfg.keys()) - set(NAMES) - {"POINTS", "PER_EPISODE"})
    if unknown:
        raise ConfigError("%s: unknown key(s) %s" % (_KEY, ", ".join(str(k) for k in unknown)))
    out = {}
    for name in NAMES:
        out[name] = named_draw.form("%s.%s" % (_KEY, name), cfg.get(name, 0))
        _check_values(name, out[name])
    points = cfg.get("POINTS", [abi.PUSH_MAX_POINTS - 1])
    if not isinstance(points, (list, tuple)) or len(points) == 0:
        raise ConfigError("%s.POINTS is a non-empty list of point indices 0 .. %d, not %r" % (_KEY, abi.PUSH_MAX_POINTS - 1, points))
    seen = []
    for m in points:
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
            raise ConfigError("%s.POINTS: %r is not a point index" % (_KEY, m))
        if not 0 <= m < abi.PUSH_MAX_POINTS:
            raise ConfigError("%s.POINTS: point %d lies outside 0 .. %d" % (_KEY, m, abi.PUSH_MAX_POINTS - 1))
        if int(m) in seen:
            raise ConfigError("%s.POINTS: point %d is listed twice" % (_KEY, m))
        seen.append(int(m))
    out["POINTS"] = seen
    out["PER_EPISODE"] = named_draw.flag("%s.PER_EPISODE" % _KEY, cfg.get("PER_EPISODE", False))
    if not out["PER_EPISODE"]:
        for name in NAMES:
            if max(candidates(out[name])) == 0.0:
                raise ConfigError("%s.%s is constant zero: nothing to do" % (_KEY, name))
    return out


def varying_names(spec):
    """The names of ``NAMES`` whose value can differ between envs or episodes."""
    return named_draw.varying(NAMES, spec)


# ---- the draw
def draw_push(spec, seed, gids, episodes):
    """float64 [2, M]: RATE and IMPULSE of M ``(global env id, episode)`` pairs: ``named_draw.draw``, the host's statement of
    ``redraw_value`` (csrc/vine_named_draw.h)."""
    return named_draw.draw(named_draw.named(NAMES, DRAW_NAMES, spec), seed, gids, episodes, who="draw_push")


def push_names(spec):
    """``(abi.VineEnvRedrawName * VPU_NAMES, values float64 [V])`` of a spec."""
    return named_draw.pack(named_draw.named(NAMES, DRAW_NAMES, spec))


def push_spec(lib, vcfg, spec, device_values=None):
    """``vine_env_push_spec``: the checked ``abi.VineEnvPushSpec``; ``ValueError`` with the library's text for a refusal."""
    names, values = push_names(spec)
    points = (C.c_int32 * len(spec["POINTS"]))(*spec["POINTS"])
    out = abi.VineEnvPushSpec()
    rc = lib.vine_env_push_spec(C.byref(vcfg), names, values.ctypes.data if len(values) else None,
                                device_values if len(values) else None, len(values), points, len(spec["POINTS"]),
                                int(spec["PER_EPISODE"]), C.byref(out))
    if rc != abi.OK:
        raise ValueError("ENV_PUSH: %s" % lib.vine_last_error().decode(errors="replace"))
    return out


# ---- the launch, in numpy
def geometry_of(lib, vcfg):
    """What the launch takes from the handle: ``{"L", "s0", "c0"}`` as float32 (vine_create forms s0 and c0 in double and
    rounds once) and ``"composites"`` float32 [20], the configuration's own derived inertia rows."""
    phi0 = np.float64(np.float32(vcfg.phi0))
    return {"L": np.float32(vcfg.link_length), "s0": np.float32(np.sin(phi0)), "c0": np.float32(np.cos(phi0)),
            "composites": env_params.inertia_config_row(lib, vcfg)[abi.VI_MTOT:].copy()}


def push_draw(seed, gids, step, num_points):
    """The Philox call behind step ``step`` for global envs ``gids`` [M]: ``(u float32 [M], a float32 [M, 2], pick int64 [M])``
    with u = (w3 >> 8) * 2^-24, a = (w0 >> 8, w1 >> 8) * 2^-23 - 1 and pick = ((w2 >> 8) * num_points) >> 24."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)
    g = np.asarray(gids, dtype=np.int64).reshape(-1) & 0xFFFFFFFF
    w = philox4x32_10(g, step & 0xFFFFFFFF, abi.PUSH_RNG | (((step >> 32) << 8) & 0xFFFFFFFF), 0, seed & 0xFFFFFFFF, seed >> 32)
    u = (w[3] >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    a = np.stack([(x >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 8388608.0) - np.float32(1.0) for x in w[:2]], axis=1)
    pick = ((w[2] >> np.uint32(8)).astype(np.int64) * int(num_points)) >> 24
    return u, a, pick


def mass_matrix(q, composites, s0, c0, dtype=np.float64):
    """``(M [B, 6, 6], sin phi [B, 5], cos phi [B, 5])`` in ``dtype`` of joint positions ``q`` [B, 6] and composites [B, 20]:
    the matrix of the oracle's ``fd_abs`` without its ``h`` terms, formed product by product as the kernel forms it."""
    q, cm = np.asarray(q, dtype=dtype), np.asarray(composites, dtype=dtype)
    s0, c0 = dtype(s0), dtype(c0)
    th = np.zeros((len(q), NL), dtype=dtype)
    acc = np.zeros(len(q), dtype=dtype)
    for i in range(NL):
        acc = acc + q[:, 1 + i]
        th[:, i] = acc
    sn, cs = np.sin(th), np.cos(th)
    sp, cp = s0 * cs + c0 * sn, c0 * cs - s0 * sn
    b, adiag, aoff = cm[:, 1:1 + NL], cm[:, 1 + 2 * NL:1 + 3 * NL], cm[:, 1 + 3 * NL:]
    M = np.zeros((len(q), ND, ND), dtype=dtype)
    M[:, 0, 0] = cm[:, 0]
    for i in range(NL):
        M[:, i + 1, 0] = M[:, 0, i + 1] = -b[:, i] * cp[:, i]
        for j in range(i + 1):
            a = adiag[:, i] if j == i else aoff[:, i - 1]
            M[:, i + 1, j + 1] = M[:, j + 1, i + 1] = a * (cs[:, i] * cs[:, j] + sn[:, i] * sn[:, j])
    return M, sp, cp


def generalised_impulse(P, point, sp, cp, L, dtype=np.float64):
    """Q [B, 6] in the absolute coordinates of impulses ``P`` [B, 2] at points ``point`` [B]."""
    P, L = np.asarray(P, dtype=dtype), dtype(L)
    Q = np.zeros((len(P), ND), dtype=dtype)
    Q[:, 0] = P[:, 0]
    for i in range(NL):
        Q[:, i + 1] = np.where(i < np.asarray(point), -L * (cp[:, i] * P[:, 0] + sp[:, i] * P[:, 1]), dtype(0))
    return Q


def cholesky_solve(M, Q):
    """D = M^-1 Q, batched, in the dtype of ``M``: G G^T row by row, a forward and a backward substitution, every sum
    subtracting its products in ascending k -- the order of csrc/vine_env_push.hip."""
    A, x = np.array(M), np.array(Q)
    for i in range(ND):
        for j in range(i + 1):
            total = A[:, i, j].copy()
            for k in range(j):
                total = total - A[:, i, k] * A[:, j, k]
            A[:, i, j] = np.sqrt(total) if i == j else total / A[:, j, j]
    for i in range(ND):
        total = x[:, i].copy()
        for k in range(i):
            total = total - A[:, i, k] * x[:, k]
        x[:, i] = total / A[:, i, i]
    for i in range(ND - 1, -1, -1):
        total = x[:, i].copy()
        for k in range(i + 1, ND):
            total = total - A[:, k, i] * x[:, k]
        x[:, i] = total / A[:, i, i]
    return x


def to_relative(D):
    """Absolute (ydot, w_1 .. w_5) to relative generalised velocities."""
    out = np.array(D)
    out[:, 2:] = D[:, 2:] - D[:, 1:-1]
    return out


def impulse_response(q, P, point, composites, geometry, dtype=np.float64):
    """dqd [B, 6] in ``dtype``, relative coordinates: steps 5 and 6 of the header for joint positions ``q`` [B, 6], impulses
    ``P`` [B, 2] at points ``point`` [B] and composites [B, 20]."""
    M, sp, cp = mass_matrix(q, composites, geometry["s0"], geometry["c0"], dtype)
    return to_relative(cholesky_solve(M, generalised_impulse(P, point, sp, cp, geometry["L"], dtype)))


def composites64(vcfg):
    """float64 [20]: MTOT, B, GB, ADIAG, AOFF1..4 of the configuration's masses, formed in double as
    csrc/vine_inertia_composites.h forms them and NOT rounded (``geometry_of`` holds their float32)."""
    m = np.asarray(list(vcfg.link_mass), dtype=np.float64)
    inertia = np.asarray(list(vcfg.link_inertia), dtype=np.float64)
    L, l, g = np.float64(vcfg.link_length), np.float64(vcfg.link_com), np.float64(vcfg.gravity)
    mtot = np.float64(vcfg.cart_mass)
    for i in range(NL):
        mtot = mtot + m[i]
    b, adiag = np.zeros(NL), np.zeros(NL)
    for i in range(NL):
        distal = np.float64(0)
        for k in range(i + 1, NL):
            distal = distal + m[k]
        b[i] = m[i] * l + L * distal
        adiag[i] = m[i] * l * l + L * L * distal + inertia[i]
    return np.concatenate([[mtot], b, g * b, adiag, (L * b)[1:]])


def push_replay(state, reset, spec, seed, gids, steps, geometry, inertia=None, table=None, dtype=np.float64):
    """The launch behind T steps, on the host.  ``state`` [T, VF_COUNT, N] float32: the state block as each launch finds it;
    ``reset`` [T, N]: the step's flags; ``spec``: ``push_config``'s result; ``gids`` [N]: global env ids; ``steps`` [T]: the
    index of the step each launch rides behind; ``geometry``: ``geometry_of``'s result; ``inertia``: ``None`` or the bound table
    float32 [VI_COUNT, N]; ``table``: the float32 [2, N] table in force before the first step (default: episode 0's draw);
    ``dtype``: np.float64 (the reference) or np.float32 (the kernel's arithmetic restated).  P, the point and who is pushed
    are the same in both: they are float32 and integer statements.  Returns one dict per step, the state BEHIND that step's
    launch: ``pushed`` [N] bool, ``P`` [N, 2] float32, ``point`` [N], ``dqd`` [N, 6] in ``dtype`` (zeros where not pushed),
    ``qd`` [N, 6] in ``dtype`` (qd before + dqd; float32: the bits the kernel's statement gives), ``stored`` [N] bool (pushed
    with IMPULSE != 0: the envs whose velocities the launch stores), ``table`` [2, N], ``episode_index`` [N], ``push_count`` [N]."""
    gids = np.asarray(gids, dtype=np.int64).reshape(-1)
    n = len(gids)
    state = np.asarray(state, dtype=np.float32)
    reset = np.asarray(reset).reshape(len(state), n) != 0
    points = np.asarray(spec["POINTS"], dtype=np.int64)
    table = (draw_push(spec, seed, gids, 0).astype(np.float32) if table is None else np.array(table, dtype=np.float32).reshape(2, n))
    composites = (np.repeat(np.asarray(geometry["composites"])[None], n, axis=0) if inertia is None
                  else np.ascontiguousarray(np.asarray(inertia)[abi.VI_MTOT:].T))      # (as given: float32 on the device)
    episode = np.zeros(n, dtype=np.int64)
    count = np.zeros(n, dtype=np.int64)
    out = []
    for t in range(len(state)):
        u, a, pick = push_draw(seed, gids, int(steps[t]), len(points))
        pushed = ~reset[t] & (u < table[0])
        P = np.where(pushed[:, None], table[1][:, None] * a, np.float32(0)).astype(np.float32)
        point = points[pick]
        stored = pushed & (table[1] != 0)
        q = state[t, abi.VF_Q0:abi.VF_Q0 + ND].T
        qd = state[t, abi.VF_QD0:abi.VF_QD0 + ND].T.astype(dtype)
        dqd = np.zeros((n, ND), dtype=dtype)
        f = np.flatnonzero(stored)
        if len(f):
            dqd[f] = impulse_response(q[f], P[f], point[f], composites[f], geometry, dtype)
        count = count + pushed
        if spec["PER_EPISODE"]:
            r = np.flatnonzero(reset[t])
            if len(r):
                episode = episode.copy()
                episode[r] += 1
                table = table.copy()
                table[:, r] = draw_push(spec, seed, gids[r], episode[r]).astype(np.float32)
        qd_after = np.where(stored[:, None], qd + dqd, qd)           # (nothing is stored elsewhere: a -0 stays a -0)
        out.append({"pushed": pushed, "P": P, "point": point, "dqd": dqd, "qd": qd_after, "stored": stored, "table": table,
                    "episode_index": episode.copy(), "push_count": count.copy()})
    return out


# ---- the episode log's columns
def episode_params(spec, seed, gids, episodes):
    """``{"PUSH_<NAME>": float32 [M]}`` of the names that vary: ``named_draw.episode_params``."""
    return named_draw.episode_params(NAMES, DRAW_NAMES, spec, seed, gids, episodes)


class EnvPush(TableObserver):
    """A step observer (the protocol: utils/observers.py) that adds impulses to the velocities of the state block the step
    has just written.  In launch order it stands behind ``EnvSensor`` and in front of ``EnvRedraw`` / ``EnvAdr``.  The draw
    follows the device's count."""

    NAMES, DRAW_NAMES = NAMES, DRAW_NAMES

    def __init__(self, lib, handle, vcfg, spec, reset, num_envs, device):
        """``spec``: ``push_config``'s result; ``reset``: the step's buffer."""
        import torch
        super().__init__(lib, handle, vcfg, spec, num_envs, device)
        self.reset = reset
        self.pspec = push_spec(lib, vcfg, spec, self.values_ptr)
        self.push_count = torch.zeros(self.num_envs, dtype=torch.int32, device=device)

    def enqueue(self, stream, actions=None):
        native.check(self.lib.vine_env_push_scheduled(
            self.handle, self.pspec, self.reset.data_ptr(), self.table.data_ptr(), self.episode_index.data_ptr(),
            self.push_count.data_ptr(), stream), self.lib)

    def live_tensors(self):
        """A rolled-back pass has counted pushes and, per episode, redrawn values and counted episodes.  The velocities it
        wrote are in the state block, which is the env's own live tensor."""
        return [self.table, self.episode_index, self.push_count]
