"""Reference of one env step: the step kernels held to float32 round-off of the float64 oracle.

Nothing here needs a GPU.  A "device" is anything with tests/hip_env.py's interface; ``OracleDevice`` is the float32 oracle
behind that interface, so tests/test_step_reference.py runs every case below with the oracle builds alone.

Yardstick.  In front of every step both oracle builds (float32, float64; one per parameter / mass set under a per-env table,
``composite``) are loaded with the device's own state block, flags, progress and step count, and all three step with the
same actions.  Everything the step leaves behind is cut into ``groups`` (arrays ``[..., n]``, env last) and the envs into
classes:

* ``reset``: the env's reset flag was set in front of the step, so all three simulated and then re-drew its state
  (``reset_env`` runs behind the physics, oracle/vine_oracle.c ``step_env``); what they hold behind the step is a draw from
  the same counter-based generator, compared with the same metric as a group set of its own;
* ``undecided``: the two oracles leave different reset or time-out flags behind the step; left out;
* ``contact`` (obstacle cases): ``VF_CONTACT`` non-zero in front of or behind the step in any of the three runs; left out
  of the norm metric, and with an obstacle only the ``kept`` class is compared.  ``VF_CONTACT`` is the force on the
  *shelf's strip*: the pipe reports none (oracle/vine_oracle.c ``pipe_contact``), so in the ``pipe`` case every env in pipe
  contact sits in ``kept``, and so does a shelf env whose only contacts are link points against the boards.  The obstacle
  cases here therefore hold the step *around* the contacts; the contacts themselves are held to round-off feature by
  feature by tests/contact_reference.py and tests/test_step_contact_gpu.py;
* ``kept``: the rest.  An env whose flags the oracles agree on and the device does not is a failure, not a class.

Metric: ``_errs`` of tests/test_update_gradients.py (max |d| / max |ref| and ||d|| / ||ref||, float64) per class and group
over all steps of a run; the bound is ``K_STEP x max(float32 oracle's error, FLOOR)`` (``K_JOINT`` for three groups, below);
``ratios`` returns error / bound.
``controls`` rebuilds the float64 oracle with one thing subtly wrong: the device measured against it must break the bound
by ``CONTROL_MARGIN`` on some group.

``K_STEP`` is 1.5 x the worst kernel error / max(float32 oracle's error, FLOOR) measured on an MI355X over every route, case,
class and norm of tests/test_step_dynamics_gpu.py (its docstring has the table, profiles/step_dynamics/ratios.txt every
figure): 3.37 (``w``, effort_limit, four-lane kernel) -> 5.1.  ``K_STEP x CONTROL_MARGIN`` = 20.4 stays below the weakest
control's oracle-only ratio (24 x: ``link_inertia[1]`` x 1.01 on ``w``, effort_limit mode; ``link_mass[2]`` x 1.001 gives
52 - 96 x).

The joint-coordinate groups ``q``, ``qd`` and ``obs`` (which carries both) have a constant of their own, ``K_JOINT``, for a
reason in the formulation and on every route alike (measured 1.4 - 5.8, worst 5.76 -> 8.7).  Both step kernels turn the
joint angles into absolute link angles th_k = q_1 + .. + q_k once in front of the step, integrate th and w over all 160
substeps and take the differences th_k - th_(k-1) once behind it (vine_hip.hip: ``s.th`` / ``s.w``); the oracle's substep
integrates q and qd themselves and forms th afresh in every substep (``forward_dynamics``, FORM_ABS).  A joint angle of the
kernel therefore carries the round-off of two absolute angles, which are up to five times larger (|th_5| <= 2 rad against
|q_k| <= 0.4 rad), while everything the physics and the task read -- the absolute angles, the tip, the cart, the rail force,
the reward -- is as close to float64 as the float32 oracle's (``th`` 1.4 - 2.4, ``tip`` <= 1.6, ``tipv`` <= 1.7).  The groups
``th`` and ``w`` (prefix sums of ``q`` / ``qd``, the kernels' own coordinates) hold the same state to the common ``K_STEP``,
and every negative control must break a bound whichever constant its group has.
"""
import collections
import types

import numpy as np
import torch

from oracle import vine_oracle as vo
from tests import env_inertia_sets, env_params_sets
from tests.helpers import base_cfg, random_state
from tests.test_hip_parity import PHYSICS_MODES
from tests.test_update_gradients import CONTROL_MARGIN, _errs
from vine_robot_isaacgymenvs_amd import abi

K_STEP = 5.1                # kernel error <= K_STEP x max(float32 oracle's error, FLOOR), per class, group and norm
K_JOINT = 8.7               # the same for the groups in joint coordinates (q, qd, obs): see the module docstring
K_OF = {"q": K_JOINT, "qd": K_JOINT, "obs": K_JOINT}
FLOOR = 2.0 ** -24          # float32 unit round-off
N_ENVS = 328                # 5 x 64 + 8: a partial last wave and a partial last workgroup on both kernels
MAX_UNDECIDED = 0.01        # share of env-steps the two oracles may disagree on
MIN_KEPT = 0.5

_F = lambda *fields: list(fields)                                                            # noqa: E731
STATE_GROUPS = collections.OrderedDict([
    ("q", list(range(abi.VF_Q0, abi.VF_Q0 + 6))),
    ("qd", list(range(abi.VF_QD0, abi.VF_QD0 + 6))),
    ("tip", _F(abi.VF_TIP_Y, abi.VF_TIP_Z)),
    ("tipv", _F(abi.VF_TIP_VY, abi.VF_TIP_VZ)),
    ("cart", _F(abi.VF_CART_Y, abi.VF_CART_VY, abi.VF_PREV_CART_VEL, abi.VF_PREV_CART_VEL_ERR)),
    ("cmd", _F(abi.VF_SMOOTHED_U, abi.VF_U_FPAM, abi.VF_U_RAIL, abi.VF_PREV_U_RAIL)),
    ("prev_tip", _F(abi.VF_PREV_TIP_Y, abi.VF_PREV_TIP_Z)),
    ("rail_force", _F(abi.VF_RAIL_FORCE)),
    ("agg_rew", _F(abi.VF_AGG_REW)),
])
# with introspection off the step stores neither the dashboard fields nor (four-lane kernel) the body states: what is left
# of a group is what the next step reads
UNGATED = {"q": STATE_GROUPS["q"], "qd": STATE_GROUPS["qd"], "cart": _F(abi.VF_PREV_CART_VEL, abi.VF_PREV_CART_VEL_ERR),
           "cmd": _F(abi.VF_SMOOTHED_U), "agg_rew": STATE_GROUPS["agg_rew"]}
GROUP_NAMES = tuple(STATE_GROUPS) + ("th", "w", "obs", "rew", "rmat")


def groups(state, obs, rew, reward_matrix, introspect=True):
    """What one step (or a stack of steps: leading axes) left behind, as {name: float64 array [..., k, n]}.  ``state``
    [..., VF_COUNT, n], ``obs`` [..., n, F], ``rew`` [..., n], ``reward_matrix`` [..., n, NUM_REWARDS] or None (not bound).
    ``introspect`` False drops the groups (and the fields of groups) the step only stores with introspection on."""
    state = np.asarray(state, np.float64)
    fields = STATE_GROUPS if introspect else UNGATED
    out = collections.OrderedDict((name, state[..., idx, :]) for name, idx in fields.items())
    # the absolute link angles and rates th_k = q_1 + .. + q_k: the coordinates the step kernels integrate
    out["th"] = np.cumsum(state[..., abi.VF_Q0 + 1:abi.VF_Q0 + 6, :], axis=-2)
    out["w"] = np.cumsum(state[..., abi.VF_QD0 + 1:abi.VF_QD0 + 6, :], axis=-2)
    out["obs"] = np.swapaxes(np.asarray(obs, np.float64), -1, -2)
    out["rew"] = np.asarray(rew, np.float64)[..., None, :]
    if reward_matrix is not None and introspect:
        out["rmat"] = np.swapaxes(np.asarray(reward_matrix, np.float64), -1, -2)
    return out


def snapshot(state, obs, rew, reset, progress, timeouts, reward_matrix=None):
    """What a step left behind, host copies."""
    return types.SimpleNamespace(state=np.array(state, np.float64), obs=np.array(obs), rew=np.array(rew),
                                 reset_buf=np.array(reset), progress=np.array(progress),
                                 timeouts=np.array(timeouts).astype(np.uint8),
                                 reward_matrix=None if reward_matrix is None else np.array(reward_matrix))


def composite(oracles, n):
    """Env e of oracle e % len(oracles), as one oracle-like object (reset_buf, progress, timeouts, obs, rew, state
    [VF_COUNT, n] float64, reward_matrix or None): the reference of a handle whose env e carries set e % len(oracles)."""
    which, envs = np.arange(n) % len(oracles), np.arange(n)
    pick = lambda get: np.stack([np.asarray(get(o)) for o in oracles])[which, envs]         # noqa: E731
    state = np.stack([np.asarray(o.state, np.float64) for o in oracles])[which, :, envs].T
    rmat = None if oracles[0].reward_matrix is None else pick(lambda o: o.reward_matrix)
    return types.SimpleNamespace(reset_buf=pick(lambda o: o.reset_buf), progress=pick(lambda o: o.progress),
                                 timeouts=pick(lambda o: o.timeouts), obs=pick(lambda o: o.obs), rew=pick(lambda o: o.rew),
                                 state=np.ascontiguousarray(state), reward_matrix=rmat)


class OracleSet:
    """``len(cfgs)`` oracles of one precision stepped together; env e of the set is env e of oracle e % len(cfgs)."""

    def __init__(self, cfgs, precision, probe=None):
        self.oracles = [vo.OracleEnv(c, precision) for c in cfgs]
        self.n = cfgs[0].num_envs
        for o in self.oracles:
            if probe:
                o.set_probe(**probe)

    def bind_reward_matrix(self):
        for o in self.oracles:
            o.bind_reward_matrix()

    def load(self, state, reset, progress, step_count):
        for o in self.oracles:
            o.state[:] = np.asarray(state).astype(o.real)
            o.reset_buf[:], o.progress[:], o.step_count = reset, progress, step_count

    def step(self, actions):
        for o in self.oracles:
            o.step(actions)
        c = composite(self.oracles, self.n)
        return snapshot(c.state, c.obs, c.rew, c.reset_buf, c.progress, c.timeouts, c.reward_matrix)

    def close(self):
        for o in self.oracles:
            o.close()


class OracleDevice:
    """The float32 oracle behind tests/hip_env.py's interface: stands in for the device where there is none."""

    def __init__(self, cfgs):
        self.set = OracleSet(cfgs, "f32")
        self.n = self.set.n
        self._held = snapshot(np.zeros((abi.VF_COUNT, self.n)), 0, 0, np.ones(self.n, np.int64), np.zeros(self.n, np.int64), 0)
        self._count = 0

    def set_introspection(self, on):
        pass

    def bind_reward_matrix(self):
        self.set.bind_reward_matrix()

    def set_state(self, st):
        self._held.state = np.asarray(st, np.float32).astype(np.float64)

    def set_flags(self, reset, progress):
        self._held.reset_buf, self._held.progress = np.array(reset, np.int64), np.array(progress, np.int64)

    state = property(lambda self: self._held.state)
    reset_buf = property(lambda self: self._held.reset_buf)
    progress = property(lambda self: self._held.progress)

    @property
    def step_count(self):
        return self._count

    @step_count.setter
    def step_count(self, v):
        self._count = int(v)

    @property
    def reward_matrix(self):
        return self._held.reward_matrix

    def step(self, actions):
        self.set.load(self._held.state, self._held.reset_buf, self._held.progress, self._count)
        self._held = self.set.step(actions)
        self._count += 1
        h = self._held
        return h.obs, h.rew, h.reset_buf, h.timeouts

    def close(self):
        self.set.close()


# ------------------------------------------------------------------------------------------------------------ the cases
ROUTES = ("lane", "quad", "lane+params", "lane+params+inertia")
Case = collections.namedtuple("Case", "name mode randomize obs_type delay routes obstacle controls introspect_off seed")


def _cases():
    out = [Case("default", "default", True, 0, 1, ROUTES, None, True, True, 11),
           Case("default_tipobs", "default", False, abi.OBS_TIP_AND_CART_AND_OBJ_INFO, 0, ROUTES[:2], None, False, False, 12)]
    for i, mode in enumerate(m for m in PHYSICS_MODES if m != "default"):
        routes = ROUTES[:2] + ((ROUTES[3],) if mode in ("stiffness", "explicit_extras") else ())
        out.append(Case(mode, mode, True, 0, 3, routes, None, True, False, 20 + i))
    for ot, tag in ((abi.OBS_POS_ONLY, "pos_only"), (abi.OBS_POS_AND_VEL, "pos_and_vel"), (abi.OBS_POS_AND_FD_VEL, "pos_and_fd_vel"),
                    (abi.OBS_POS_AND_PREV_POS, "pos_and_prev_pos")):
        out.append(Case("obs_" + tag, "default", True, ot, 1, ROUTES[:1], None, False, False, 30 + ot))
    for i, obstacle in enumerate(("pipe", "shelf")):
        out.append(Case(obstacle, "default", True, 0, 1, ROUTES[:1], obstacle, False, False, 40 + i))
    return out


CASES = _cases()
CASE_ROUTES = [(c, r) for c in CASES for r in c.routes]
CASE_ROUTE_IDS = ["%s-%s" % (c.name, r) for c, r in CASE_ROUTES]


def case_cfg(case, n=N_ENVS, max_episode_length=None):
    cfg = base_cfg(n, case.obs_type, case.randomize, action_delay=case.delay, seed=1000 + case.seed)
    if case.randomize:
        cfg.obs_noise_std, cfg.action_noise_std = 0.01, 0.02
        cfg.dyn_scale_min, cfg.dyn_scale_max = 0.9, 1.1
    if case.obstacle:
        cfg.set_flag(abi.FLAG_CREATE_PIPE if case.obstacle == "pipe" else abi.FLAG_CREATE_SHELF, True)
    PHYSICS_MODES[case.mode](cfg)
    if max_episode_length is not None:
        cfg.max_episode_length = max_episode_length
    return cfg


def route_cfgs(cfg, route):
    """The configurations whose oracles make up the reference of ``route``: env e is env e of entry e % len."""
    if route == "lane+params":
        return [env_params_sets.set_cfg(cfg, g) for g in range(env_params_sets.NUM_SETS)]
    if route == "lane+params+inertia":
        return [env_inertia_sets.set_cfg(cfg, g) for g in range(env_inertia_sets.NUM_SETS)]
    return [cfg]


def seed_device(dev, case, cfg, rng):
    """tests/test_hip_parity.py seed_both on the device alone (the oracles are loaded from it): a random mid-episode state
    with every FIFO slot filled, 15 % of the envs about to reset, a block at the time limit; pipe / shelf placed around each
    tip as test_contact_error_is_float32_round_off places them."""
    n = cfg.num_envs
    st = random_state(rng, n, cfg)
    for s in range(1, abi.MAX_DELAY):
        st[abi.VF_FIFO0 + 2 * s] = rng.uniform(-1, 1, n)
        st[abi.VF_FIFO0 + 2 * s + 1] = rng.uniform(-0.1, 3.0, n)
    if case.obstacle == "pipe":
        tp = rng.uniform(0.4, 1.1, n)
        th = tp + np.pi / 2
        yl, zl = rng.uniform(-0.01, 0.03, n), rng.uniform(0.0, 0.1, n)
        st[abi.VF_PIPE_Y] = st[abi.VF_TIP_Y] - (yl * np.cos(th) - zl * np.sin(th))
        st[abi.VF_PIPE_Z] = st[abi.VF_TIP_Z] - (yl * np.sin(th) + zl * np.cos(th))
        st[abi.VF_OBJ_ANGLE] = tp
    elif case.obstacle == "shelf":
        st[abi.VF_SHELF_Y] = st[abi.VF_TIP_Y] - 0.2 - 0.05 + rng.uniform(-0.04, 0.04, n)
        st[abi.VF_SHELF_Z] = st[abi.VF_TIP_Z] + rng.uniform(-0.06, 0.06, n)
    reset = (rng.uniform(size=n) < 0.15).astype(np.int64)
    progress = rng.integers(0, cfg.max_episode_length - 1, n)
    progress[: n // 16] = cfg.max_episode_length - 2
    dev.set_state(st)
    dev.set_flags(reset, progress)


# --------------------------------------------------------------------------------------------------------- the controls
def controls(cfg, mode):
    """{name: OracleSet} -- the float64 oracle of ``cfg`` (``mode``: its entry of PHYSICS_MODES) with one thing subtly wrong."""
    def scaled(field, index=None, factor=1.0 + 1e-3):
        c = type(cfg).from_buffer_copy(cfg)
        if index is None:
            assert getattr(c, field) != 0.0, field
            setattr(c, field, getattr(c, field) * factor)
        else:
            assert getattr(c, field)[index] != 0.0, (field, index)
            getattr(c, field)[index] *= factor
        return OracleSet([c], "f64")

    out = collections.OrderedDict()
    for field in ("damping", "gravity", "dt", "cart_mass", "rail_p_gain", "rail_acceleration", "smoothing_alpha_inflate",
                  "smoothing_alpha_deflate", "joint1_z", "phi0"):
        out[field] = scaled(field)
    for field, index in (("link_mass", 2), ("link_mass", 4), ("fpam_K", 1), ("fpam_B", 0)):
        out["%s[%d]" % (field, index)] = scaled(field, index)
    if cfg.fpam_C[2] != 0.0:
        out["fpam_C[2]"] = scaled("fpam_C", 2)
    if cfg.stiffness != 0.0:
        out["stiffness"] = scaled("stiffness")
    if cfg.link_angular_damping != 0.0:
        out["link_angular_damping"] = scaled("link_angular_damping", factor=1.0 + 1e-2)
    out["link_inertia[1]"] = scaled("link_inertia", 1, factor=1.0 + 1e-2)
    out["effort_first_substep_only"] = OracleSet([cfg], "f64", probe={"effort_first_substep_only": True})
    out["armature"] = OracleSet([cfg], "f64", probe={"armature": 1e-6})
    assert ("stiffness" in out) == (mode in ("stiffness", "explicit_extras")), mode
    assert ("link_angular_damping" in out) == (mode in ("linkdamp", "explicit_extras")), mode
    assert ("fpam_C[2]" in out) == (mode not in ("explicit", "explicit_extras")), mode
    return out


# ----------------------------------------------------------------------------------------------------------- the metric
def classify(reset_in, s32, s64, dev, obstacle=False, contact_in=None):
    """The env classes of one step -> {"kept", "reset", "undecided", "contact", "bad": bool [n]}.  ``bad``: the oracles
    agree on the flags behind the step and the device does not."""
    flags = lambda s: (np.asarray(s.reset_buf) != 0, np.asarray(s.timeouts) != 0)            # noqa: E731
    (r32, t32), (r64, t64), (rd, td) = flags(s32), flags(s64), flags(dev)
    undecided = (r32 != r64) | (t32 != t64)
    bad = ~undecided & ((rd != r64) | (td != t64) | (np.asarray(dev.progress) != np.asarray(s64.progress)))
    contact = np.zeros_like(undecided)
    if obstacle:
        for s in (s32, s64, dev):
            contact |= s.state[abi.VF_CONTACT] != 0
        if contact_in is not None:
            contact |= np.asarray(contact_in) != 0
    was_reset = np.asarray(reset_in) != 0
    decided = ~undecided & ~bad
    return {"kept": decided & ~was_reset & ~contact, "reset": decided & was_reset & ~contact, "undecided": undecided,
            "contact": decided & contact, "bad": bad}


class Tally:
    """The compared columns of every step of a run, per run name ("dev", "f32", "f64", a control), class and group."""

    def __init__(self, classes=("kept", "reset"), group_fn=None):
        self.classes = classes
        self.group_fn = group_fn or groups
        self.cols = collections.defaultdict(list)
        self.count = collections.Counter()
        self.steps = 0

    def add(self, masks, runs, introspect=True):
        """``runs``: {run name: snapshot} of one step."""
        self.steps += 1
        for k, m in masks.items():
            self.count[k] += int(m.sum())
        for who, s in runs.items():
            g = self.group_fn(s.state, s.obs, s.rew, s.reward_matrix, introspect)
            for cls in self.classes:
                for name, a in g.items():
                    self.cols[(who, cls, name)].append(a[..., masks[cls]])

    def of(self, who):
        return {(cls, name): np.concatenate(v, axis=-1) for (w, cls, name), v in self.cols.items() if w == who}


def errors(got, ref):
    """{(class, group): (max-relative, rms-relative)} of ``got`` against ``ref`` (both ``Tally.of``)."""
    return {k: _errs(torch.as_tensor(got[k]), torch.as_tensor(ref[k])) for k in ref if ref[k].size}


def bounds(base):
    """``K x max(float32 oracle's error, FLOOR)`` per class, group and norm, from ``errors(f32, f64)``; ``K`` is ``K_JOINT``
    for the groups of ``K_OF`` and ``K_STEP`` for every other."""
    for k, e in base.items():
        assert np.isfinite(e[0]) and np.isfinite(e[1]), ("float32 baseline not finite", k)
    return {k: (K_OF.get(k[1], K_STEP) * max(e[0], FLOOR), K_OF.get(k[1], K_STEP) * max(e[1], FLOOR)) for k, e in base.items()}


def unscaled(r):
    """Ratios error / bound -> error / max(float32 oracle's error, FLOOR)."""
    return {k: (v[0] * K_OF.get(k[1], K_STEP), v[1] * K_OF.get(k[1], K_STEP)) for k, v in r.items()}


def ratios(err, bound):
    """error / bound per class, group and norm."""
    return {k: (err[k][0] / bound[k][0], err[k][1] / bound[k][1]) for k in bound}


def worst(r):
    k = max(r, key=lambda k: max(r[k]))
    return k, max(r[k])


def table(title, r):
    """One line per class and group: the two ratios."""
    lines = ["[step dynamics] %s" % title]
    for (cls, name), v in r.items():
        lines.append("    %-6s %-10s max-rel %8.3f   rms-rel %8.3f" % (cls, name, v[0], v[1]))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------ the driver
def _reward_matrix(dev):
    if hasattr(dev, "reward_matrix_t"):                      # tests/hip_env.py: a device tensor, None until bound
        return None if dev.reward_matrix_t is None else dev.reward_matrix_t.cpu().numpy()
    return dev.reward_matrix


def run_steps(dev, refs, actions, obstacle=False, introspect=True, classes=("kept", "reset"), classifier=None, group_fn=None):
    """Step ``dev`` through ``actions`` [T, n, 2]; in front of every step every entry of ``refs`` ({"f32", "f64", control
    names: OracleSet}) is loaded with the device's state block, flags, progress and step count and steps with it.  Asserts
    the flags, progress and time-outs of every decided env against the float64 oracle -> Tally.  ``classifier(state, reset,
    runs, refs)`` (tests/contact_reference.py) replaces ``classify``; an env of its ``near`` class counts as not decided.
    ``group_fn`` replaces ``groups``."""
    tally = Tally(classes, group_fn)
    for a in actions:
        state, reset, progress, count = dev.state, np.array(dev.reset_buf), np.array(dev.progress), dev.step_count
        for r in refs.values():
            r.load(state, reset, progress, count)
        obs, rew, rst, to = dev.step(a)
        runs = {"dev": snapshot(dev.state, obs, rew, rst, dev.progress, to, _reward_matrix(dev) if introspect else None)}
        for k, r in refs.items():
            runs[k] = r.step(a)
        if classifier:
            masks = classifier(state, reset, runs, refs)
        else:
            masks = classify(reset, runs["f32"], runs["f64"], runs["dev"], obstacle, state[abi.VF_CONTACT])
        assert not masks["bad"].any(), ("the oracles agree on the flags of these envs and the device does not",
                                        np.flatnonzero(masks["bad"]).tolist(), count)
        ok = ~masks["undecided"] & ~masks.get("near", False)
        for name in ("reset_buf", "progress", "timeouts"):
            assert np.array_equal(getattr(runs["dev"], name)[ok], getattr(runs["f64"], name)[ok]), (name, count)
        assert dev.step_count == count + 1
        tally.add(masks, runs, introspect)
    return tally


PARTS = {"a": 1, "b": 6}          # steps; "b" runs with max_episode_length 4
B_EPISODE = 4


def run_case(case, route, make_device, part, introspect=True, with_controls=False):
    """Part "a": one step from ``seed_device``'s state with resets and a time-out block, step count 7, reward matrix bound.
    Part "b": six teacher-forced steps from such a state with 4-step episodes, so that delay-ring contents, time-outs and
    the steps behind a reset are all met and no error compounds.  ``make_device(cfg, route)`` creates the device with the
    route's tables bound.  With ``introspect`` off the reward matrix stays unbound (binding it switches introspection on) and
    only part "a" is meaningful: the oracles read the tip position in front of a step from the state block, which the
    four-lane kernel then no longer stores.  -> (Tally, names of the controls)."""
    assert introspect or part == "a"
    cfg = case_cfg(case, max_episode_length=B_EPISODE if part == "b" else None)
    rng = np.random.default_rng(100 * case.seed + ord(part))
    dev = make_device(cfg, route)
    cfgs = route_cfgs(cfg, route)
    refs = collections.OrderedDict((p, OracleSet(cfgs, p)) for p in ("f32", "f64"))
    names = ()
    if with_controls:
        assert len(cfgs) == 1
        wrong = controls(cfg, case.mode)
        names = tuple(wrong)
        refs.update(wrong)
    try:
        if introspect:
            dev.bind_reward_matrix()
            for r in refs.values():
                r.bind_reward_matrix()
        else:
            dev.set_introspection(False)
        seed_device(dev, case, cfg, rng)
        dev.step_count = 7
        actions = rng.uniform(-1.3, 1.3, (PARTS[part], cfg.num_envs, 2)).astype(np.float32)
        tally = run_steps(dev, refs, actions, bool(case.obstacle), introspect, ("kept",) if case.obstacle else ("kept", "reset"))
    finally:
        dev.close()
        for r in refs.values():
            r.close()
    return tally, names


def report(tally, controls_of=()):
    """-> (ratios of the device, {control: (class, group, margin)}, the float32 baseline's errors)."""
    ref = tally.of("f64")
    base = errors(tally.of("f32"), ref)
    bound = bounds(base)
    r = ratios(errors(tally.of("dev"), ref), bound)
    margins = {}
    for name in controls_of:
        k, m = worst(ratios(errors(tally.of("dev"), tally.of(name)), bound))
        margins[name] = (k[0], k[1], m)
    return r, margins, base
