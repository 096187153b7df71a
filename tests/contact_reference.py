"""Reference of the obstacle contacts, feature by feature: the step kernels' pipe and shelf contacts held to float32
round-off of the float64 oracle (tests/test_step_contact_gpu.py; tests/test_contact_reference.py runs all of it with the
oracle builds alone).  Nothing here needs a GPU.

Features.  The two contact models of oracle/vine_oracle.c (``pipe_contact``, ``shelf_contact``) restated in float64 numpy
as a list of *features*, each one (kind, link, item, body, face):

* ``pipe_point``: point ``item`` = 3 e + t of link ``link`` (edge e: y = LINK_Y0 / LINK_Y1, position t: z0, middle, z1)
  inside wall ``body``, leaving through its y face (``face`` 0: ey < ez) or its z face (1); 5 x 6 x 2 x 2 = 120;
* ``pipe_corner``: corner ``item`` (bit 0: outer side of the wall, bit 1: far end of the tube) of wall ``body`` inside
  link ``link``'s rectangle, nearest side ``face`` (0: z0, 1: z1, 2: LINK_Y0, 3: LINK_Y1); 5 x 4 x 2 x 4 = 160;
* ``shelf_point``: as ``pipe_point`` against board ``body``; 120;
* ``shelf_corner``: front corner ``item`` of the strip inside link ``link``'s rectangle, nearest side ``face``; 40.

``census`` returns per env which features are active (the geometric decision: the clamp f > 0 may still leave a zero
force), each feature's generalised force, the force on the strip and the margin of every discontinuous decision (a point
entering a box: |min(ey, ez)|; the choice ey < ez: |ey - ez|; a corner entering a rectangle: |smallest depth|; the nearest
side: second smallest depth - smallest), in metres, minimum over the env.

Directed states.  The obstacle pose is per-env state the step only reads, so ``directed`` builds a state *for a feature*:
a random posture (tests/helpers.py random_state; velocities, FIFO, flags, progress as tests/step_reference.py seed_device
draws them), then the obstacle's origin solved so that the feature's point (corner) sits 0.2 - 2 mm inside the chosen face
(side), both ends of the tube and both signs of every face drawn.  Env e targets feature e mod count, twice over.  The
link is the fastest index of the feature list, so any five consecutive envs -- the first five of every wave and workgroup
of either kernel (64 envs a wave on the one-lane kernel, 16 on the four-lane kernel) among them -- hold contacts of five
different links.  The first 1/16 of the envs is at the time limit;
the last 1/8 (second copies only: every feature keeps a copy that is compared) has its reset flag set.

Yardstick (short step: dt / 10, one substep, control_freq_inv 4 -- four substeps of the production length).  Classes per
env-step: ``undecided`` (the oracles' flags differ), ``near`` (the float64 oracle's margin over the step,
``OracleEnv.contact_margin``, below ``DELTA`` = 2^-20 m, about 3 x the position error of the float32 oracle after four
substeps: a rounding may decide a contact the other way; left out, flags included), ``reset`` (flag set in front of the
step), ``contact`` (some feature active in front of the step by the census), ``kept`` (the rest).  Every group of
step_reference.GROUP_NAMES and ``contact`` (VF_CONTACT, VF_CONTACT_MEAN) per class in both norms:
error <= ``K_CONTACT x max(float32 oracle's error, FLOOR)``; flags, progress and time-outs equal the float64 oracle's on every
decided env.  The 40 substeps of a production step carry the float32 error itself to ``DELTA``, so the full step
(``run_full``) is judged by percentiles of the per-env error instead.  ``shifted`` moves every env's obstacle along its
feature's normal (the direction in which the contact opens) for the test of the broad phase; its
bit-for-bit part runs on states of its own (``isolated``) in which the targeted feature is the env's only contact.
"""
import collections
import types

import numpy as np

from oracle import vine_oracle as vo
from tests import step_reference as sr
from tests.helpers import base_cfg, random_state
from vine_robot_isaacgymenvs_amd import abi

DELTA = 2.0 ** -20            # metres: margin under which a contact decision counts as undecidable in float32
MAX_NEAR = 0.01               # share of env-steps of a short-step case that may be ``near``
MAX_UNDECIDED_FULL = 0.06     # share of envs of a full step the oracles may disagree on or that are ``near``
PEN = (2.0e-4, 2.0e-3)        # directed penetrations, metres
CULL_EPS = 1.0e-5             # vine_hip.hip PIPE_CULL_EPS
# error <= K_CONTACT x max(float32 oracle's error, FLOOR): 1.5 x the worst ratio measured on an MI355X over every case,
# route, class, group and norm of tests/test_step_contact_gpu.py part (a) (its docstring has the table): 3.294 (``q`` of the
# ``kept`` class, pipe, one-lane kernel) -> 4.95.  No group comes near step_reference.K_JOINT = 8.7; the ``contact`` class
# stays within 1.36.  K_CONTACT x CONTROL_MARGIN = 19.8 stays below the weakest control's oracle-only ratio (contact_c x
# 1.001: 61 - 72; tests/test_contact_reference.py asserts it)
K_CONTACT = 4.95
CASES = collections.OrderedDict([("pipe", 560), ("shelf", 320), ("shelf+pipe", 880)])      # envs: two per feature
ROUTES = {"pipe": ("lane", "quad", "lane+params"), "shelf": ("lane", "quad"), "shelf+pipe": ("lane", "quad")}
CASE_ROUTES = [(c, r) for c in CASES for r in ROUTES[c]]
SEED = {"pipe": 51, "shelf": 52, "shelf+pipe": 53}
GROUP_NAMES = sr.GROUP_NAMES + ("contact",)

# the constants of oracle/vine_oracle.c, as its float64 build holds them (BOARD is a table of float literals there)
CONTACT_K, CONTACT_C = 2000.0, 2.0
LINK_Y0, LINK_Y1 = -0.0381, 0.0719
LINK0_Z0, LINK0_Z1 = -0.00575, 0.09425
PIPE_LEN, PIPE_WALL, PIPE_OUTER = 0.34125, 0.00525, 0.1554
_f = lambda x: float(np.float32(x))                                                            # noqa: E731
BOARD = ((_f(-0.001), _f(0.0), _f(0.1995), _f(0.005)), (_f(0.0), _f(0.2), _f(0.2), _f(0.005)))
STRIP_Y, STRIP_HZ = 0.2, 0.005
NL = 5

Feature = collections.namedtuple("Feature", "kind link item body face")


def features(obstacle):
    """The feature list of ``obstacle`` ("pipe": 280, "shelf": 160, "shelf+pipe": pipe then shelf), link fastest."""
    out = []
    if "pipe" in obstacle:
        out += [Feature("pipe_point", k, p, w, f) for f in range(2) for w in range(2) for p in range(6) for k in range(NL)]
        out += [Feature("pipe_corner", k, c, w, f) for f in range(4) for w in range(2) for c in range(4) for k in range(NL)]
    if "shelf" in obstacle:
        out += [Feature("shelf_point", k, p, b, f) for f in range(2) for b in range(2) for p in range(6) for k in range(NL)]
        out += [Feature("shelf_corner", k, c, 0, f) for f in range(4) for c in range(2) for k in range(NL)]
    return out


# ------------------------------------------------------------------------------------------------------------ the census
def kinematics(cfg, state):
    """Joint positions PY, PZ [6, n] (entry k: the joint link k hangs from), joint velocities VY, VZ [5, n], sin / cos of the
    links' world angles S, C [5, n], their rates OM [5, n]; float64, as ``pipe_contact`` walks the chain."""
    st = np.asarray(state, np.float64)
    q, qd = st[abi.VF_Q0:abi.VF_Q0 + 6], st[abi.VF_QD0:abi.VF_QD0 + 6]
    n = st.shape[1]
    L = float(cfg.link_length)
    PY, PZ = np.zeros((NL + 1, n)), np.zeros((NL + 1, n))
    VY, VZ, S, C, OM = (np.zeros((NL, n)) for _ in range(5))
    PY[0], PZ[0] = q[0], float(cfg.joint1_z)
    ang, om, pvy, pvz = np.full(n, float(cfg.phi0)), np.zeros(n), qd[0].copy(), np.zeros(n)
    for k in range(NL):
        ang = ang + q[k + 1]
        om = om + qd[k + 1]
        S[k], C[k], OM[k], VY[k], VZ[k] = np.sin(ang), np.cos(ang), om, pvy, pvz
        PY[k + 1], PZ[k + 1] = PY[k] + L * -S[k], PZ[k] + L * C[k]
        pvy, pvz = pvy + L * om * -C[k], pvz + L * om * -S[k]
    return types.SimpleNamespace(PY=PY, PZ=PZ, VY=VY, VZ=VZ, S=S, C=C, OM=OM, L=L, n=n)


def _span(k, L):
    return (LINK0_Z0, LINK0_Z1) if k == 0 else (0.0, L)


def _point(kin, k, p):
    """Point ``p`` = 3 e + t of link k: lever (ry, rz), world position and velocity."""
    z0, z1 = _span(k, kin.L)
    yl = LINK_Y1 if p >= 3 else LINK_Y0
    zl = (z0, 0.5 * (z0 + z1), z1)[p % 3]
    dy, dz, ly, lz = -kin.S[k], kin.C[k], kin.C[k], kin.S[k]
    ry, rz = zl * dy + yl * ly, zl * dz + yl * lz
    return ry, rz, kin.PY[k] + ry, kin.PZ[k] + rz, kin.VY[k] - kin.OM[k] * rz, kin.VZ[k] + kin.OM[k] * ry


def _generalised(kin, k, wy, wz, fy, fz):
    """The generalised force [n, 6] of the world force (fy, fz) at (wy, wz) on link k."""
    Q = np.zeros((kin.n, 6))
    Q[:, 0] = fy
    for j in range(k + 1):
        Q[:, j + 1] = (wy - kin.PY[j]) * fz - (wz - kin.PZ[j]) * fy
    return Q


def _box(ddy, ddz, hy, hz, vy, vz):
    """A point at (ddy, ddz) from the centre of a box of half-extents (hy, hz), velocity (vy, vz), all in the box's frame
    -> inside, leaves through the y face, force through the y face, force through the z face, margin."""
    ey, ez = hy - np.abs(ddy), hz - np.abs(ddz)
    inside = (ey > 0) & (ez > 0)
    yface = ey < ez
    sy, sz = np.where(ddy > 0, 1.0, -1.0), np.where(ddz > 0, 1.0, -1.0)
    fy = sy * np.maximum(CONTACT_K * ey - CONTACT_C * sy * vy, 0.0)
    fz = sz * np.maximum(CONTACT_K * ez - CONTACT_C * sz * vz, 0.0)
    lo = np.minimum(ey, ez)
    margin = np.where(lo > 0, np.minimum(lo, np.abs(ey - ez)), -lo)
    return inside, yface, fy, fz, margin


def _corner(kin, k, wy, wz):
    """An obstacle corner at world (wy, wz) against link k's rectangle -> inside, nearest side [n], force on the link
    (fy, fz), margin."""
    z0, z1 = _span(k, kin.L)
    dy, dz, ly, lz = -kin.S[k], kin.C[k], kin.C[k], kin.S[k]
    ry, rz = wy - kin.PY[k], wz - kin.PZ[k]
    zl, yl = ry * dy + rz * dz, ry * ly + rz * lz
    dep = np.stack([zl - z0, z1 - zl, yl - LINK_Y0, LINK_Y1 - yl])
    inside = (zl > z0) & (zl < z1) & (yl > LINK_Y0) & (yl < LINK_Y1)
    side = np.argmin(dep, axis=0)                              # the first of equal depths, as the oracle's chain of `<`
    ny = np.choose(side, [-dy, dy, -ly, ly])
    nz = np.choose(side, [-dz, dz, -lz, lz])
    vy, vz = kin.VY[k] - kin.OM[k] * rz, kin.VZ[k] + kin.OM[k] * ry
    srt = np.sort(dep, axis=0)
    f = np.maximum(CONTACT_K * srt[0] + CONTACT_C * (vy * ny + vz * nz), 0.0)
    margin = np.where(srt[0] > 0, np.minimum(srt[0], srt[1] - srt[0]), -srt[0])
    return inside, side, -f * ny, -f * nz, margin


def pipe_frame(state):
    st = np.asarray(state, np.float64)
    th = st[abi.VF_OBJ_ANGLE] + 1.5707963267948966
    return st[abi.VF_PIPE_Y], st[abi.VF_PIPE_Z], np.cos(th), np.sin(th)


def census(cfg, state, obstacle, forces=True):
    """-> features, active [F, n] bool, force [F, n, 6], strip [n] (|F| on the shelf's strip), margin [n]."""
    st = np.asarray(state, np.float64)
    kin = kinematics(cfg, st)
    feats = features(obstacle)
    at = {f: i for i, f in enumerate(feats)}
    n = kin.n
    active, force = np.zeros((len(feats), n), bool), np.zeros((len(feats), n, 6) if forces else 0)
    margin, strip_y, strip_z = np.full(n, np.inf), np.zeros(n), np.zeros(n)

    def put(feature, on, wy, wz, fy, fz):
        i = at[feature]
        active[i] = on
        if forces:
            force[i] = _generalised(kin, feature.link, wy, wz, fy, fz) * on[:, None]

    if "pipe" in obstacle:
        oy, oz, ct, sn = pipe_frame(st)
        lo = (0.0, PIPE_OUTER - PIPE_WALL)
        for k in range(NL):
            for p in range(6):
                _, _, wy, wz, vy, vz = _point(kin, k, p)
                gy, gz = wy - oy, wz - oz
                pyl, pzl = gy * ct + gz * sn, -gy * sn + gz * ct
                vyl, vzl = vy * ct + vz * sn, -vy * sn + vz * ct
                for w in range(2):
                    inside, yface, fyl, fzl, m = _box(pyl - (lo[w] + 0.5 * PIPE_WALL), pzl - 0.5 * PIPE_LEN, 0.5 * PIPE_WALL,
                                                      0.5 * PIPE_LEN, vyl, vzl)
                    margin = np.minimum(margin, m)
                    put(Feature("pipe_point", k, p, w, 0), inside & yface, wy, wz, fyl * ct, fyl * sn)
                    put(Feature("pipe_point", k, p, w, 1), inside & ~yface, wy, wz, -fzl * sn, fzl * ct)
            for w in range(2):
                for c in range(4):
                    pyl, pzl = lo[w] + (PIPE_WALL if c & 1 else 0.0), (PIPE_LEN if c & 2 else 0.0)
                    wy, wz = oy + pyl * ct - pzl * sn, oz + pyl * sn + pzl * ct
                    inside, side, fy, fz, m = _corner(kin, k, wy, wz)
                    margin = np.minimum(margin, m)
                    for s in range(4):
                        put(Feature("pipe_corner", k, c, w, s), inside & (side == s), wy, wz, fy, fz)
    if "shelf" in obstacle:
        sy, sz = st[abi.VF_SHELF_Y], st[abi.VF_SHELF_Z]
        for k in range(NL):
            for p in range(6):
                _, _, wy, wz, vy, vz = _point(kin, k, p)
                for b in range(2):
                    cy, cz, hy, hz = BOARD[b]
                    inside, yface, fy, fz, m = _box(wy - (sy + cy), wz - (sz + cz), hy, hz, vy, vz)
                    margin = np.minimum(margin, m)
                    put(Feature("shelf_point", k, p, b, 0), inside & yface, wy, wz, fy, 0.0 * fy)
                    put(Feature("shelf_point", k, p, b, 1), inside & ~yface, wy, wz, 0.0 * fz, fz)
            for c in range(2):
                wy, wz = sy + STRIP_Y, sz + (STRIP_HZ if c else -STRIP_HZ)
                inside, side, fy, fz, m = _corner(kin, k, wy, wz)
                margin = np.minimum(margin, m)
                strip_y, strip_z = strip_y - fy * inside, strip_z - fz * inside
                for s in range(4):
                    put(Feature("shelf_corner", k, c, 0, s), inside & (side == s), wy, wz, fy, fz)
    return types.SimpleNamespace(features=feats, active=active, force=force, strip=np.hypot(strip_y, strip_z), margin=margin)


# --------------------------------------------------------------------------------------------------- the directed states
def _around_tip(st, rng, which):
    """The other obstacle of ``shelf+pipe``: around the tip, as step_reference.seed_device places it."""
    n = st.shape[1]
    if which == "pipe":
        tp = rng.uniform(0.4, 1.1, n)
        th = tp + np.pi / 2
        yl, zl = rng.uniform(-0.01, 0.03, n), rng.uniform(0.0, 0.1, n)
        st[abi.VF_PIPE_Y] = st[abi.VF_TIP_Y] - (yl * np.cos(th) - zl * np.sin(th))
        st[abi.VF_PIPE_Z] = st[abi.VF_TIP_Z] - (yl * np.sin(th) + zl * np.cos(th))
        st[abi.VF_OBJ_ANGLE] = tp
    else:
        st[abi.VF_SHELF_Y] = st[abi.VF_TIP_Y] - 0.2 - 0.05 + rng.uniform(-0.04, 0.04, n)
        st[abi.VF_SHELF_Z] = st[abi.VF_TIP_Z] + rng.uniform(-0.06, 0.06, n)


def _in_box(rng, pen, hy, hz, face):
    """Where in a box (from its centre) a point sits ``pen`` inside face ``face`` and well inside the other pair of faces,
    and the box-frame direction in which the box has to move for the point to come out."""
    sg = rng.choice((-1.0, 1.0))
    if face == 0:
        return sg * (hy - pen), rng.uniform(-1, 1) * (hz - PEN[1] - 4.0e-4), (-sg, 0.0)
    return rng.uniform(-1, 1) * (hy - PEN[1] - 4.0e-4), sg * (hz - pen), (0.0, -sg)


def _in_rect(rng, pen, z0, z1, side):
    """Link-local (zl, yl) of a corner ``pen`` inside side ``side`` of the rectangle and 5 mm or more from the others."""
    zl, yl = rng.uniform(z0 + 5.0e-3, z1 - 5.0e-3), rng.uniform(LINK_Y0 + 5.0e-3, LINK_Y1 - 5.0e-3)
    return ((z0 + pen, yl), (z1 - pen, yl), (zl, LINK_Y0 + pen), (zl, LINK_Y1 - pen))[side]


def _place(st, kin, e, f, rng, alone=False):
    """Writes the obstacle pose of env e that puts feature f ``pen`` deep; -> the world direction in which the obstacle
    leaves the contact, and ``pen``.  ``alone``: a link point that enters a wall through its end face gets a tube that lies
    *in front of* the point's edge (its axis within 20 degrees of the edge's outward normal): the end's corners are then inside
    the link with the point and leave it with the point when the tube moves out along its axis.  With the tube's axis running
    into the link instead, moving the tube out pushes the end's corners into the link, and the env is never free."""
    pen = rng.uniform(*PEN)
    k = f.link
    dy, dz, ly, lz = -kin.S[k, e], kin.C[k, e], kin.C[k, e], kin.S[k, e]
    if f.kind.endswith("point"):
        _, _, wy, wz, _, _ = _point(kin, k, f.item)
        wy, wz = wy[e], wz[e]
    else:
        z0, z1 = _span(k, kin.L)
        zl, yl = _in_rect(rng, pen, z0, z1, f.face)
        wy, wz = kin.PY[k, e] + zl * dy + yl * ly, kin.PZ[k, e] + zl * dz + yl * lz
        normal = ((-dy, -dz), (dy, dz), (-ly, -lz), (ly, lz))[f.face]
    if f.kind.startswith("pipe"):
        tp = rng.uniform(-np.pi, np.pi)
        lo = (0.0, PIPE_OUTER - PIPE_WALL)[f.body]
        if f.kind == "pipe_point":
            ddy, ddz, (ny, nz) = _in_box(rng, pen, 0.5 * PIPE_WALL, 0.5 * PIPE_LEN, f.face)
            if alone and f.face == 1:
                tilt = rng.uniform(-np.radians(20.0), np.radians(20.0))
                outward = (-ly, -lz) if f.item < 3 else (ly, lz)            # from the point's edge out of the link
                ay = outward[0] * np.cos(tilt) - outward[1] * np.sin(tilt)
                az = outward[0] * np.sin(tilt) + outward[1] * np.cos(tilt)
                ay, az = (ay, az) if ddz < 0 else (-ay, -az)                 # the tube's axis e_z = (-sin th, cos th)
                tp = np.arctan2(-ay, az) - 1.5707963267948966
        ct, sn = np.cos(tp + 1.5707963267948966), np.sin(tp + 1.5707963267948966)
        if f.kind == "pipe_point":
            pyl, pzl = lo + 0.5 * PIPE_WALL + ddy, 0.5 * PIPE_LEN + ddz
            normal = (ny * ct - nz * sn, ny * sn + nz * ct)
        else:
            pyl, pzl = lo + (PIPE_WALL if f.item & 1 else 0.0), (PIPE_LEN if f.item & 2 else 0.0)
        st[abi.VF_PIPE_Y, e], st[abi.VF_PIPE_Z, e] = wy - (pyl * ct - pzl * sn), wz - (pyl * sn + pzl * ct)
        st[abi.VF_OBJ_ANGLE, e] = tp
    else:
        if f.kind == "shelf_point":
            cy, cz, hy, hz = BOARD[f.body]
            ddy, ddz, normal = _in_box(rng, pen, hy, hz, f.face)
            oy, oz = cy + ddy, cz + ddz
        else:
            oy, oz = STRIP_Y, (STRIP_HZ if f.item else -STRIP_HZ)
        st[abi.VF_SHELF_Y, e], st[abi.VF_SHELF_Z, e] = wy - oy, wz - oz
    return normal, pen


def directed(cfg, obstacle, seed, resets=True):
    """The directed state block of ``obstacle`` for ``cfg.num_envs`` envs (module docstring) -> namespace(state float32-
    exact [VF_COUNT, n], reset, progress, target [n] feature index, normal [2, n], pen [n], features).  Asserts that every
    env's targeted feature is active and that no decision of the env is within ``DELTA``.  ``resets`` False: the same states
    with no reset flag set (the full step: both copies of every feature are simulated and compared)."""
    rng = np.random.default_rng(seed)
    n = cfg.num_envs
    feats = features(obstacle)
    st = random_state(rng, n, cfg)
    for s in range(1, abi.MAX_DELAY):
        st[abi.VF_FIFO0 + 2 * s] = rng.uniform(-1, 1, n)
        st[abi.VF_FIFO0 + 2 * s + 1] = rng.uniform(-0.1, 3.0, n)
    st = st.astype(np.float32).astype(np.float64)              # the posture the device will hold
    kin = kinematics(cfg, st)
    target = np.arange(n) % len(feats)
    if obstacle == "shelf+pipe":
        _around_tip(st, rng, "pipe")
        _around_tip(st, rng, "shelf")
    normal, pen = np.zeros((2, n)), np.zeros(n)
    todo = np.arange(n)
    for _ in range(40):                                        # redraw the placements a rounding or a second contact spoils
        for e in todo:
            normal[:, e], pen[e] = _place(st, kin, e, feats[target[e]], rng)
        st = st.astype(np.float32).astype(np.float64)
        c = census(cfg, st, obstacle)
        ok = c.active[target, np.arange(n)] & (c.margin >= 4 * DELTA)
        todo = np.flatnonzero(~ok)
        if not todo.size:
            break
    assert not todo.size, ("directed states: the targeted feature is not active with margin", todo.tolist())
    reset = np.zeros(n, np.int64)
    reset[n - n // 8:] = int(resets)
    assert n - n // 8 >= len(feats)
    progress = rng.integers(0, cfg.max_episode_length - 1, n)
    progress[: n // 16] = cfg.max_episode_length - 2
    return types.SimpleNamespace(state=st, reset=reset, progress=progress, target=target, normal=normal, pen=pen,
                                 features=feats)


def _posture(rng, n, cfg):
    st = random_state(rng, n, cfg)
    for s in range(1, abi.MAX_DELAY):
        st[abi.VF_FIFO0 + 2 * s] = rng.uniform(-1, 1, n)
        st[abi.VF_FIFO0 + 2 * s + 1] = rng.uniform(-0.1, 3.0, n)
    return st.astype(np.float32).astype(np.float64)


def free_cfg(cfg):
    """``cfg`` without its obstacles: free space."""
    free = type(cfg).from_buffer_copy(cfg)
    free.set_flag(abi.FLAG_CREATE_PIPE, False)
    free.set_flag(abi.FLAG_CREATE_SHELF, False)
    return free


class FreeOverStep:
    """``check(state, reset, progress, actions)`` -> bool [n]: envs whose step from ``state`` the float64 oracle finds free of
    contact -- its step with the obstacles equals its free-space step bit for bit in q and qd, and no contact decision came
    within ``DELTA`` in any substep."""

    def __init__(self, cfg):
        self.oracles = [vo.OracleEnv(c, "f64") for c in (cfg, free_cfg(cfg))]
        self.margin = self.oracles[0].contact_margin

    def check(self, state, reset, progress, actions):
        out = []
        for o in self.oracles:
            o.state[:] = state
            o.reset_buf[:], o.progress[:], o.step_count = reset, progress, 7
            o.step(actions)
            out.append((np.array(o.state[abi.VF_Q0:abi.VF_Q0 + 6]), np.array(o.state[abi.VF_QD0:abi.VF_QD0 + 6])))
        (q, qd), (fq, fqd) = out
        return (q == fq).all(0) & (qd == fqd).all(0) & (self.margin >= DELTA)

    def close(self):
        for o in self.oracles:
            o.close()


def free_over_step(cfg, state, reset, progress, actions):
    f = FreeOverStep(cfg)
    try:
        return f.check(state, reset, progress, actions)
    finally:
        f.close()


ISOLATED_ROUNDS = 80


def never_alone(f):
    """Features that cannot be an env's only contact.  The strip's two front corners lie 10 mm apart, one above the other, and
    the links hang within 0.4 (k + 1) rad of the vertical: with the upper corner just inside a link's upper (z0) side, or the
    lower corner just inside its lower (z1) side, the other corner lies 10 mm cos(angle) deeper inside the same rectangle
    (every link is longer than that), so it touches too unless the link is all but horizontal -- which links 0 - 2 cannot be
    and links 3, 4 are not drawn to be."""
    return f.kind == "shelf_corner" and (f.item, f.face) in ((1, 0), (0, 1))



def isolated(cfg, obstacle, seed):
    """Directed states for the test of the broad phase (part (d), bit for bit): as ``directed``, with posture, velocities and
    placement of an env redrawn until the targeted feature is the env's *only* contact -- with the obstacle moved out by the
    penetration and 4 x PIPE_CULL_EPS along the feature's normal (``shifted``) the census finds no feature active and no
    decision within ``DELTA``, and the float64 oracle finds the whole short step from there free of contact
    (``free_over_step``: the targeted point must not close the 40 um again within the step, nor any other).  No reset flags;
    ``actions`` [n, 2] are part of the draw.  Envs that stay unsolved after ``ISOLATED_ROUNDS`` redraws are listed in
    ``unsolved`` (their states are the last draw)."""
    rng = np.random.default_rng(seed + 1000)
    n = cfg.num_envs
    feats = features(obstacle)
    target = np.arange(n) % len(feats)
    actions = rng.uniform(-1.3, 1.3, (n, 2)).astype(np.float32)
    reset = np.zeros(n, np.int64)
    progress = rng.integers(0, cfg.max_episode_length - 1, n)
    progress[: n // 16] = cfg.max_episode_length - 2
    st = _posture(rng, n, cfg)
    normal, pen = np.zeros((2, n)), np.zeros(n)
    todo = np.arange(n)
    d = types.SimpleNamespace(state=st, reset=reset, progress=progress, target=target, normal=normal, pen=pen,
                              features=feats, actions=actions)
    step = FreeOverStep(cfg)
    skipped = np.array([never_alone(feats[t]) for t in target])
    kin = kinematics(cfg, st)
    for e in np.flatnonzero(skipped):                      # placed as ``directed`` places them, never among the free envs
        normal[:, e], pen[e] = _place(st, kin, e, feats[target[e]], rng)
    st[:] = st.astype(np.float32).astype(np.float64)
    todo = np.flatnonzero(~skipped)
    for _ in range(ISOLATED_ROUNDS):
        m = min(16, max(1, 2000 // todo.size))             # candidates per env and round: the census is cheap, the step is not
        env = np.repeat(todo, m)
        fresh = _posture(rng, env.size, cfg)
        if obstacle == "shelf+pipe":                       # the obstacle that is not targeted: out of reach, 2 m to the side
            fresh[abi.VF_PIPE_Y], fresh[abi.VF_PIPE_Z], fresh[abi.VF_OBJ_ANGLE] = 2.0, 0.5, 0.7
            fresh[abi.VF_SHELF_Y], fresh[abi.VF_SHELF_Z] = 2.0, 0.5
        kin = kinematics(cfg, fresh)
        cn, cp = np.zeros((2, env.size)), np.zeros(env.size)
        for i, e in enumerate(env):
            cn[:, i], cp[i] = _place(fresh, kin, i, feats[target[e]], rng, alone=True)
        sub = types.SimpleNamespace(state=fresh.astype(np.float32).astype(np.float64), target=target[env], normal=cn, pen=cp,
                                    features=feats)
        c = census(cfg, sub.state, obstacle, forces=False)
        good = c.active[sub.target, np.arange(env.size)] & (c.margin >= 4 * DELTA)
        co = census(cfg, shifted(sub, obstacle, 4 * CULL_EPS), obstacle, forces=False)
        good &= ~co.active.any(0) & (co.margin >= DELTA)
        good = good.reshape(todo.size, m)
        pick = np.arange(todo.size) * m + good.argmax(1)    # the first candidate that is alone (the first of all if none is)
        st[:, todo], normal[:, todo], pen[todo] = sub.state[:, pick], cn[:, pick], cp[pick]
        ok = good.any(1)
        if ok.any():
            ok &= step.check(shifted(d, obstacle, 4 * CULL_EPS), reset, progress, actions)[todo]
        todo = todo[~ok]
        if not todo.size:
            break
    step.close()
    d.unsolved = np.sort(np.concatenate([todo, np.flatnonzero(skipped)]))
    return d


def shifted(d, obstacle, distance):
    """The directed states with every env's targeted obstacle moved so that the targeted feature's penetration is
    ``-distance`` (zero-penetration pose plus ``distance`` along the feature's normal)."""
    st = d.state.copy()
    move = d.normal * (d.pen + distance)
    pipe = np.array([f.kind.startswith("pipe") for f in d.features])[d.target]
    st[abi.VF_PIPE_Y] += np.where(pipe, move[0], 0.0)
    st[abi.VF_PIPE_Z] += np.where(pipe, move[1], 0.0)
    st[abi.VF_SHELF_Y] += np.where(~pipe, move[0], 0.0)
    st[abi.VF_SHELF_Z] += np.where(~pipe, move[1], 0.0)
    return st.astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------- the cases
def case_cfg(obstacle, short=True, n=None):
    """Default physics with randomisation (as step_reference's obstacle cases), delay 1, the non-zero-contact-force reset
    on with a shelf; ``short``: dt / 10 and one substep, so that a step is four substeps of the production length."""
    cfg = base_cfg(n or CASES[obstacle], 0, True, action_delay=1, seed=1000 + SEED[obstacle])
    cfg.obs_noise_std, cfg.action_noise_std = 0.01, 0.02
    cfg.dyn_scale_min, cfg.dyn_scale_max = 0.9, 1.1
    cfg.set_flag(abi.FLAG_CREATE_PIPE, "pipe" in obstacle)
    cfg.set_flag(abi.FLAG_CREATE_SHELF, "shelf" in obstacle)
    cfg.set_flag(abi.FLAG_USE_NONZERO_CONTACT_FORCE_RESET, "shelf" in obstacle)
    if short:
        cfg.dt, cfg.substeps = cfg.dt / 10, 1
    assert cfg.control_freq_inv == 4
    return cfg


def contact_groups(state, obs, rew, reward_matrix, introspect=True):
    g = sr.groups(state, obs, rew, reward_matrix, introspect)
    g["contact"] = np.asarray(state, np.float64)[..., [abi.VF_CONTACT, abi.VF_CONTACT_MEAN], :]
    return g


def margins(oset):
    """The contact margins [n] of an OracleSet's last step (recorded from the first call on: call once before the step)."""
    m = np.stack([o.contact_margin for o in oset.oracles])
    return m[np.arange(oset.n) % len(oset.oracles), np.arange(oset.n)].copy()


def classifier(cfg, obstacle, log=None):
    """The classes of the module docstring, as ``step_reference.run_steps`` asks for them; ``log``: a list that receives
    (census in front of the step, masks) of every step."""
    def classify(state_in, reset_in, runs, refs):
        base = sr.classify(reset_in, runs["f32"], runs["f64"], runs["dev"])
        c = census(cfg, state_in, obstacle)
        decided = ~base["undecided"] & ~base["bad"]
        was_reset = np.asarray(reset_in) != 0
        near = ~base["undecided"] & (margins(refs["f64"]) < DELTA)
        decided &= ~near
        touching = c.active.any(0)
        masks = {"kept": decided & ~was_reset & ~touching, "contact": decided & ~was_reset & touching,
                 "reset": decided & was_reset, "near": near, "undecided": base["undecided"], "bad": base["bad"] & ~near}
        if log is not None:
            log.append((c, masks))
        return masks
    return classify


def bounds(base):
    for k, e in base.items():
        assert np.isfinite(e[0]) and np.isfinite(e[1]), ("float32 baseline not finite", k)
    return {k: (K_CONTACT * max(e[0], sr.FLOOR), K_CONTACT * max(e[1], sr.FLOOR)) for k, e in base.items()}


PROBES = collections.OrderedDict([        # the negative controls: one factor of the contact probe off by 0.1 %
    ("contact_k", 1.001), ("contact_c", 1.001), ("pipe_wall", 1.001), ("pipe_outer", 1.001), ("pipe_len", 1.001),
    ("link_y0", 1.001), ("link_y1", 1.001), ("link0_overhang", 1.001), ("board_hy", 1.001), ("board_hz", 1.001),
    ("strip_offset", 1.001)])
PROBES_OF = {"pipe": ("contact_k", "contact_c", "pipe_wall", "pipe_outer", "pipe_len", "link_y0", "link_y1", "link0_overhang"),
             "shelf": ("contact_k", "contact_c", "link_y0", "link_y1", "link0_overhang", "board_hy", "board_hz", "strip_offset")}
PROBES_OF["shelf+pipe"] = tuple(PROBES)


def controls(cfg, obstacle):
    out = collections.OrderedDict()
    for name in PROBES_OF[obstacle]:
        out[name] = sr.OracleSet([cfg], "f64")
        out[name].oracles[0].set_contact_probe(**{name: PROBES[name]})
    return out


STEPS = 4          # short-step run: one step from the directed states and three teacher-forced steps


def run_short(obstacle, route, make_device, with_controls=False, shift=None):
    """Part (a) of a case on a route -> (Tally, control names, log of (census, masks) per step, the directed states).
    ``shift``: one step from ``shifted(directed, obstacle, shift)`` instead."""
    cfg = case_cfg(obstacle)
    d = directed(cfg, obstacle, SEED[obstacle])
    rng = np.random.default_rng(100 * SEED[obstacle] + 1)
    dev = make_device(cfg, route)
    cfgs = sr.route_cfgs(cfg, route)
    refs = collections.OrderedDict((p, sr.OracleSet(cfgs, p)) for p in ("f32", "f64"))
    names = ()
    if with_controls:
        assert len(cfgs) == 1
        wrong = controls(cfg, obstacle)
        names = tuple(wrong)
        refs.update(wrong)
    log = []
    try:
        dev.bind_reward_matrix()
        for r in refs.values():
            r.bind_reward_matrix()
        margins(refs["f64"])
        dev.set_state(d.state if shift is None else shifted(d, obstacle, shift))
        dev.set_flags(d.reset, d.progress)
        dev.step_count = 7
        actions = rng.uniform(-1.3, 1.3, (STEPS if shift is None else 1, cfg.num_envs, 2)).astype(np.float32)
        tally = sr.run_steps(dev, refs, actions, True, True, ("kept", "reset", "contact"),
                             classifier=classifier(cfg, obstacle, log), group_fn=contact_groups)
    finally:
        dev.close()
        for r in refs.values():
            r.close()
    return tally, names, log, d


def report(tally, controls_of=()):
    """-> (error / bound of the device per class, group and norm; {control: (class, group, margin)} over the ``contact``
    class; the float32 baseline's errors)."""
    ref = tally.of("f64")
    base = sr.errors(tally.of("f32"), ref)
    bound = bounds(base)
    r = sr.ratios(sr.errors(tally.of("dev"), ref), bound)
    out = {}
    for name in controls_of:
        wrong = sr.ratios(sr.errors(tally.of("dev"), tally.of(name)), bound)
        k, m = sr.worst({key: v for key, v in wrong.items() if key[0] == "contact"})
        out[name] = (k[0], k[1], m)
    return r, out, base


def covered(log, n_features):
    """Per feature: in how many compared ``contact`` env-steps of a run it was active."""
    count = np.zeros(n_features, np.int64)
    for c, masks in log:
        count += (c.active & masks["contact"][None, :]).sum(1)
    return count


def _check_bound(title, tally, names, n, max_near=MAX_NEAR):
    """Prints every figure of a short-step run, then asserts the classes' sizes, the bound and the controls -> raw ratios,
    the controls' margins."""
    ratios, ctl, base = report(tally, names)
    raw = {k: (v[0] * K_CONTACT, v[1] * K_CONTACT) for k, v in ratios.items()}
    k, w = sr.worst(raw)
    total = tally.steps * n
    print("\n" + sr.table("%s: kernel error / max(float32 oracle's error, FLOOR); classes %s; near %.3f %%; worst %.3f (%s %s)"
                          % (title, dict(tally.count), 100.0 * tally.count["near"] / total, w, k[0], k[1]), raw)
          .replace("[step dynamics]", "[step contact]"), flush=True)
    if names:
        print("[step contact] %s: controls, error against the wrong oracle / bound: %s"
              % (title, ", ".join("%s %.1f (%s %s)" % (nm, m[2], m[0], m[1]) for nm, m in ctl.items())), flush=True)
    assert tally.count["bad"] == 0
    assert tally.count["near"] <= max_near * total, (title, tally.count)
    assert tally.count["undecided"] <= sr.MAX_UNDECIDED * total, (title, tally.count)
    assert {key[1] for key in ratios} == set(GROUP_NAMES) and "contact" in {key[0] for key in ratios}
    bad = {key: (round(v[0], 3), round(v[1], 3)) for key, v in ratios.items() if not max(v) <= 1.0}
    assert not bad, (title, "kernel error above K_CONTACT = %g x max(float32 oracle's error, FLOOR): error / bound" % K_CONTACT, bad)
    weak = {nm: m for nm, m in ctl.items() if not m[2] >= sr.CONTROL_MARGIN}
    assert not weak, (title, "negative control within the bound", weak)
    return raw, ctl


def check_short(title, tally, names, log, n, n_features):
    """Part (a): the bound and the controls; ``near`` within its share; every feature active in a compared ``contact``
    env; all three classes compared."""
    raw, ctl = _check_bound(title, tally, names, n)
    count = covered(log, n_features)
    assert count.shape == (n_features,) and (count > 0).all(), (title, "features never active in a compared contact env",
                                                               np.flatnonzero(count == 0).tolist())
    assert {key[0] for key in raw} == {"kept", "reset", "contact"}
    return raw, ctl


MIN_SHIFTED = 0.9     # share of the features with a compared env in the shifted runs: a feature has two envs, a quarter of the
#                       second ones is reset and an env drops out as ``near`` with a chance of 0.02 at most


def check_shifted(title, tally, log, d, shift):
    """Part (d), against the oracle: one short step from ``shifted(d, obstacle, shift)``.  Inside (shift < 0) the targeted
    feature is active in its env, outside it is not; either way the step is the oracle's within the bound."""
    # (twice the cases' share of ``near``: the targeted feature starts 40 um from its decision and crosses it within the
    # step wherever it moves that way: one more decision per env that passes through zero)
    raw, _ = _check_bound(title, tally, (), d.state.shape[1], 2 * MAX_NEAR)
    (c, masks), envs = log[0], np.arange(d.state.shape[1])
    hit = c.active[d.target, envs]
    assert hit.all() if shift < 0 else not hit.any(), title
    count = np.zeros(len(d.features), np.int64)
    np.add.at(count, d.target, (masks["contact"] | masks["kept"]))
    print("[step contact] %s: features with a compared env: %d of %d" % (title, (count > 0).sum(), count.size), flush=True)
    assert (count > 0).mean() >= MIN_SHIFTED, (title, (count > 0).mean())
    return raw


def check_outside(title, with_, without, free, d):
    """Part (d), bit for bit: every env of the ``isolated`` states is free of contact with its obstacle 4 x PIPE_CULL_EPS clear
    of the targeted feature (but the ``unsolved``), and there the step with the obstacle is the free-space step.  Every
    feature has such an env except those that cannot be an env's only contact (``never_alone``, which names the reason)."""
    count = np.zeros(len(d.features), np.int64)
    np.add.at(count, d.target, free)
    kinds = collections.Counter(f.kind for f, c in zip(d.features, count) if c)
    missing = [tuple(f) for f, c in zip(d.features, count) if not c]
    print("[step contact] %s: %d of %d envs free of contact with the obstacle 4 x PIPE_CULL_EPS clear of the targeted "
          "feature; features with a free env: %s of %d; without: %s" % (title, free.sum(), free.size, dict(kinds), len(d.features),
                                                                        missing), flush=True)
    assert all(never_alone(Feature(*f)) for f in missing), (title, "features without a free env", missing)
    assert all(count[i] == 0 for i, f in enumerate(d.features) if never_alone(f))
    for name in CULL_FIELDS:
        a, b = with_[name][..., free], without[name][..., free]
        assert a.size and np.array_equal(a, b), (title, name, np.flatnonzero(free)[(a != b).any(0)].tolist())


# -------------------------------------------------------------------------------------------------------- the full step
FULL_GROUPS = ("q", "qd", "th", "w", "tip", "obs", "rew", "VF_CONTACT", "VF_CONTACT_MEAN")
FULL_FACTOR = 2.0           # tests/test_hip_parity.py test_contact_error_is_float32_round_off's rule


def full_groups(state, obs, rew, reward_matrix, introspect=True):
    g = sr.groups(state, obs, rew, reward_matrix, introspect)
    out = collections.OrderedDict((k, g[k]) for k in FULL_GROUPS[:7])
    out["VF_CONTACT"] = np.asarray(state, np.float64)[..., [abi.VF_CONTACT], :]
    out["VF_CONTACT_MEAN"] = np.asarray(state, np.float64)[..., [abi.VF_CONTACT_MEAN], :]
    return out


def run_full(obstacle, route, make_device):
    """Part (b): one step of the production length (40 substeps) from the directed states, no reset flag set (both copies
    of every feature are simulated) -> (Tally, log, directed)."""
    cfg = case_cfg(obstacle, short=False)
    d = directed(cfg, obstacle, SEED[obstacle], resets=False)
    rng = np.random.default_rng(100 * SEED[obstacle] + 2)
    dev = make_device(cfg, route)
    refs = collections.OrderedDict((p, sr.OracleSet(sr.route_cfgs(cfg, route), p)) for p in ("f32", "f64"))
    log = []
    try:
        margins(refs["f64"])
        dev.set_state(d.state)
        dev.set_flags(d.reset, d.progress)
        dev.step_count = 7
        actions = rng.uniform(-1.3, 1.3, (1, cfg.num_envs, 2)).astype(np.float32)
        tally = sr.run_steps(dev, refs, actions, True, True, ("contact",), classifier=classifier(cfg, obstacle, log),
                             group_fn=full_groups)
    finally:
        dev.close()
        for r in refs.values():
            r.close()
    return tally, log, d


def check_full(title, tally, log, n, n_features):
    """Per group, over the compared ``contact`` envs: median and 99th percentile of the per-env error (max over the group's
    fields of |x - float64|) at most ``FULL_FACTOR`` x the float32 oracle's plus one float32 ulp of the group's range.
    Prints every figure first -> {group: (ratio at the median, ratio at the 99th percentile)}."""
    dev, f32, f64 = tally.of("dev"), tally.of("f32"), tally.of("f64")
    out, bad = collections.OrderedDict(), {}
    lines = ["[step contact] %s: per-env error, kernel / float32 oracle at the 50th and 99th percentile; classes %s; "
             "near + undecided %.2f %%" % (title, dict(tally.count), 100.0 * (tally.count["near"] + tally.count["undecided"]) / n)]
    for name in FULL_GROUPS:
        ref = f64[("contact", name)]
        e_dev, e_32 = np.abs(dev[("contact", name)] - ref).max(0), np.abs(f32[("contact", name)] - ref).max(0)
        ulp = float(np.spacing(np.float32(np.abs(ref).max())))
        figures = [(np.percentile(e_dev, p), np.percentile(e_32, p)) for p in (50, 99)]
        out[name] = tuple(a / b if b > 0 else (0.0 if a == 0 else np.inf) for a, b in figures)
        lines.append("    %-16s p50 %.3e / %.3e = %6.3f   p99 %.3e / %.3e = %6.3f   ulp %.1e"
                     % (name, figures[0][0], figures[0][1], out[name][0], figures[1][0], figures[1][1], out[name][1], ulp))
        if not all(a <= FULL_FACTOR * b + ulp for a, b in figures):
            bad[name] = out[name]
    print("\n" + "\n".join(lines), flush=True)
    assert tally.count["bad"] == 0
    assert tally.count["near"] + tally.count["undecided"] <= MAX_UNDECIDED_FULL * n, (title, tally.count)
    count = covered(log, n_features)
    print("[step contact] %s: features active in a compared contact env: %d of %d" % (title, (count > 0).sum(), n_features),
          flush=True)
    # a feature is left without a compared env only where every env that holds it came within DELTA of a decision over the
    # 40 substeps (the margin rule; no env is reset here): with two envs a feature and at most 6 % of them ``near``, that is
    # 0.36 % of the features at most on average, and 1 % is allowed; which ones is printed and recorded
    c, masks = log[0]
    missing = np.flatnonzero(count == 0)
    print("[step contact] %s: features without a compared env (all their envs ``near``): %s"
          % (title, [tuple(c.features[i]) for i in missing]), flush=True)
    assert not (c.active[missing] & ~(masks["near"] | masks["undecided"])[None, :]).any(), (title, missing.tolist())
    assert missing.size <= 0.01 * n_features, (title, missing.tolist())
    assert not bad, (title, "per-env error above %g x the float32 oracle's + one ulp: ratios at p50, p99" % FULL_FACTOR, bad)
    return out


# ----------------------------------------------------------------------------------------------------- culling is exact
CULL_FIELDS = ("q", "qd", "tip", "tipv", "cart", "rail_force", "obs", "rew", "contact")


def _one_step(dev, state, d, actions):
    dev.set_state(state)
    dev.set_flags(d.reset, d.progress)
    dev.step_count = 7
    obs, rew, _, _ = dev.step(actions)
    return contact_groups(dev.state, obs, rew, None)


def run_outside(obstacle, make_device):
    """Part (d), bit for bit: the ``isolated`` states with every env's obstacle 4 x PIPE_CULL_EPS clear of its targeted
    feature, stepped by the device with the obstacle and without it (free space) -> (groups of the device with, without,
    bool [n]: envs the float64 oracle finds free of contact over the step -- all but ``unsolved`` --, the states)."""
    cfg = case_cfg(obstacle)
    d = isolated(cfg, obstacle, SEED[obstacle])
    state = shifted(d, obstacle, 4 * CULL_EPS)
    got = []
    for c in (cfg, free_cfg(cfg)):
        dev = make_device(c, "lane")
        try:
            got.append(_one_step(dev, state, d, d.actions))
        finally:
            dev.close()
    free = free_over_step(cfg, state, d.reset, d.progress, d.actions)
    assert not free[d.unsolved].any() and free.sum() == free.size - d.unsolved.size
    return got[0], got[1], free, d
