"""tests/contact_reference.py checked with the oracle builds alone: the census against the oracle's own contact functions and
its recorded margin, the directed generator's coverage, and every part of tests/test_step_contact_gpu.py with the float32
oracle in the device's place (so the classes, the conditions and the negative controls are known to hold before a GPU is
asked)."""
import ctypes as C

import numpy as np
import pytest

from oracle import vine_oracle as vo
from tests import contact_reference as cr
from tests import step_reference as sr
from vine_robot_isaacgymenvs_amd import abi

OBSTACLES = tuple(cr.CASES)


def _oracle_device(cfg, route):
    return sr.OracleDevice(sr.route_cfgs(cfg, route))


def _random_states(cfg, obstacle, seed):
    """step_reference.seed_device's placement (both obstacles around the tip for ``shelf+pipe``)."""
    rng = np.random.default_rng(seed)
    st = cr.random_state(rng, cfg.num_envs, cfg)
    for which in ("pipe", "shelf"):
        if which in obstacle:
            cr._around_tip(st, rng, which)
    return st


def _oracle_forces(cfg, st, obstacle):
    """Summed generalised contact force [n, 6] and strip force [n] by vine_oracle_pipe_contact / vine_oracle_shelf_contact."""
    lib = vo.load("f64")
    n = st.shape[1]
    total, strip = np.zeros((n, 6)), np.zeros(n)
    for e in range(n):
        q = np.ascontiguousarray(st[abi.VF_Q0:abi.VF_Q0 + 6, e])
        qd = np.ascontiguousarray(st[abi.VF_QD0:abi.VF_QD0 + 6, e])
        Q = np.zeros(6)
        if "pipe" in obstacle:
            lib.vine_oracle_pipe_contact(C.byref(cfg), vo._dp(q), vo._dp(qd), st[abi.VF_PIPE_Y, e], st[abi.VF_PIPE_Z, e],
                                         st[abi.VF_OBJ_ANGLE, e], vo._dp(Q))
            total[e] += Q
        if "shelf" in obstacle:
            strip[e] = lib.vine_oracle_shelf_contact(C.byref(cfg), vo._dp(q), vo._dp(qd), st[abi.VF_SHELF_Y, e],
                                                     st[abi.VF_SHELF_Z, e], vo._dp(Q))
            total[e] += Q
    return total, strip


@pytest.mark.parametrize("states", ["directed", "random"])
@pytest.mark.parametrize("obstacle", OBSTACLES)
def test_census_forces_sum_to_the_oracles(obstacle, states):
    """The features' forces add up to the oracle's contact function, and the strip's force is the oracle's, to 1e-12."""
    cfg = cr.case_cfg(obstacle)
    st = cr.directed(cfg, obstacle, cr.SEED[obstacle]).state if states == "directed" else _random_states(cfg, obstacle, 7)
    c = cr.census(cfg, st, obstacle)
    total, strip = _oracle_forces(cfg, st, obstacle)
    assert np.abs(total).max() > 0.1 and c.active.any(0).mean() > (0.9 if states == "directed" else 0.05)
    scale = np.maximum(np.abs(total).max(1, keepdims=True), 1e-300)
    assert (np.abs(c.force.sum(0) - total) / scale).max() <= 1e-12
    assert (np.abs(c.strip - strip) <= 1e-12 * np.maximum(np.abs(strip), 1e-300)).all()
    if "shelf" in obstacle:
        assert (strip > 0).any()


@pytest.mark.parametrize("obstacle", OBSTACLES)
def test_oracle_margin_of_one_substep_is_the_census(obstacle):
    """With one control iteration of one substep the oracle evaluates the contacts once, at the state in front of the step:
    the margin it records is the census's (directed and random states)."""
    cfg = cr.case_cfg(obstacle)
    cfg.control_freq_inv = 1
    for st in (cr.directed(cr.case_cfg(obstacle), obstacle, cr.SEED[obstacle]).state, _random_states(cfg, obstacle, 8)):
        o = vo.OracleEnv(cfg, "f64")
        m = o.contact_margin
        assert np.isinf(m).all()
        o.state[:] = st
        o.reset_buf[:] = 0
        o.step(np.zeros((cfg.num_envs, 2), np.float32))
        want = cr.census(cfg, st, obstacle).margin
        assert np.isfinite(want).all() and want.min() < 1e-3 < want.max()
        assert np.abs(m - want).max() <= 1e-12 * np.abs(want).max()
        o.close()


def test_unit_probe_and_margin_leave_the_step_unchanged():
    """All probe factors at 1 and the margin recorded: bit for bit the unprobed step, both precisions."""
    cfg = cr.case_cfg("shelf+pipe", short=False)
    d = cr.directed(cfg, "shelf+pipe", cr.SEED["shelf+pipe"])
    a = np.random.default_rng(3).uniform(-1, 1, (cfg.num_envs, 2)).astype(np.float32)
    for precision in ("f32", "f64"):
        out = []
        for probed in (False, True):
            o = vo.OracleEnv(cfg, precision)
            if probed:
                o.set_contact_probe(**{k: 1.0 for k in vo.CONTACT_PROBE})
                o.contact_margin
            o.state[:] = d.state.astype(o.real)
            o.reset_buf[:], o.progress[:], o.step_count = d.reset, d.progress, 7
            o.step(a)
            out.append((np.array(o.state), np.array(o.obs), np.array(o.rew), np.array(o.reset_buf)))
            o.close()
        for x, y in zip(*out):
            assert np.array_equal(x, y)
    o = vo.OracleEnv(cfg, "f64")
    with pytest.raises(AssertionError):
        o.set_contact_probe(no_such_factor=1.0)
    o.close()


@pytest.mark.parametrize("obstacle,count", [("pipe", 280), ("shelf", 160), ("shelf+pipe", 440)])
def test_directed_states_reach_every_feature(obstacle, count):
    cfg = cr.case_cfg(obstacle)
    assert cfg.num_envs == cr.CASES[obstacle] == 2 * count
    d = cr.directed(cfg, obstacle, cr.SEED[obstacle])
    c = cr.census(cfg, d.state, obstacle)
    n = cfg.num_envs
    assert len(c.features) == len(set(c.features)) == count
    assert np.array_equal(d.target, np.arange(n) % count)
    assert c.active[d.target, np.arange(n)].all() and (c.margin >= cr.DELTA).all()
    assert (c.active.sum(1) >= 2).all()                                   # two envs per feature
    assert np.array_equal(d.state, d.state.astype(np.float32).astype(np.float64))
    # the drawn penetration is the targeted feature's: moved out along its normal by exactly that much, the feature sits on
    # its decision (margin ~ 0, float32 rounding of the pose: 2^-24 x 2 m), and 1 um short of that it is still closed
    assert ((cr.PEN[0] <= d.pen) & (d.pen <= cr.PEN[1])).all()
    assert (cr.census(cfg, cr.shifted(d, obstacle, 0.0), obstacle, forces=False).margin <= 2.0 ** -22).all()
    assert cr.census(cfg, cr.shifted(d, obstacle, -1.0e-6), obstacle, forces=False).active[d.target, np.arange(n)].all()
    # the first five envs of every wave (16 envs on the four-lane kernel, 64 on the one-lane kernel) and workgroup (64 /
    # 256 envs) hold contacts of five different links
    link = np.array([f.link for f in d.features])[d.target]
    for start in range(0, n - 4, 16):
        assert set(link[start:start + 5]) == set(range(5)), start
    # a block with the reset flag set that leaves every feature a copy, a block at the time limit
    assert d.reset.sum() == n // 8 and not d.reset[:count].any()
    assert (d.progress[: n // 16] == cfg.max_episode_length - 2).all()
    # moving the obstacle out along the feature's normal by the penetration and 4 x PIPE_CULL_EPS more opens the targeted
    # contact; 4 x PIPE_CULL_EPS short of that it is still closed
    out = cr.census(cfg, cr.shifted(d, obstacle, 4 * cr.CULL_EPS), obstacle)
    ins = cr.census(cfg, cr.shifted(d, obstacle, -4 * cr.CULL_EPS), obstacle)
    assert not out.active[d.target, np.arange(n)].any() and ins.active[d.target, np.arange(n)].all()


@pytest.mark.parametrize("obstacle,route", [(c, r) for c, r in cr.CASE_ROUTES if r != "quad"])
def test_short_step_case_with_the_oracle_as_device(obstacle, route):
    """Part (a) with the float32 oracle as the device: every ratio is 1 / K_CONTACT at most, ``near`` is within its share,
    every feature is compared; and the negative controls, float32 oracle against the wrong float64 oracle."""
    with_controls = route == "lane"
    tally, names, log, d = cr.run_short(obstacle, route, _oracle_device, with_controls)
    raw, ctl = cr.check_short("%s %s, oracle as device" % (obstacle, route), tally, names, log, d.state.shape[1], len(d.features))
    assert max(max(v) for v in raw.values()) <= 1.0 + 1e-12
    assert tally.count["contact"] >= 0.5 * tally.steps * d.state.shape[1] and tally.count["reset"] > 0
    if with_controls:
        assert set(names) == set(cr.PROBES_OF[obstacle]) and len(names) >= 8
        # K_CONTACT x CONTROL_MARGIN stays below the weakest control's oracle-only ratio
        weakest = min(m[2] for m in ctl.values()) * cr.K_CONTACT
        assert cr.K_CONTACT * sr.CONTROL_MARGIN < weakest, (weakest, ctl)


def test_controls_cover_every_probe_factor():
    assert set(cr.PROBES) == set(vo.CONTACT_PROBE) == set(cr.PROBES_OF["shelf+pipe"])
    assert set(cr.PROBES_OF["pipe"]) | set(cr.PROBES_OF["shelf"]) == set(cr.PROBES)


@pytest.mark.parametrize("obstacle", OBSTACLES)
def test_full_step_case_with_the_oracle_as_device(obstacle):
    tally, log, d = cr.run_full(obstacle, "lane", _oracle_device)
    out = cr.check_full("%s lane, oracle as device" % obstacle, tally, log, d.state.shape[1], len(d.features))
    assert set(out) == set(cr.FULL_GROUPS)


@pytest.mark.parametrize("obstacle", OBSTACLES)
def test_culling_case_with_the_oracle_as_device(obstacle):
    for shift in (-4 * cr.CULL_EPS, 4 * cr.CULL_EPS):
        tally, _, log, d = cr.run_short(obstacle, "lane", _oracle_device, shift=shift)
        cr.check_shifted("%s lane, oracle as device, shift %+.0e" % (obstacle, shift), tally, log, d, shift)
    with_, without, free, d = cr.run_outside(obstacle, _oracle_device)
    cr.check_outside(obstacle, with_, without, free, d)
    # the isolated states: the targeted feature is active, and alone once the obstacle is 4 x PIPE_CULL_EPS clear of it
    cfg, envs = cr.case_cfg(obstacle), np.arange(free.size)
    assert cr.census(cfg, d.state, obstacle, forces=False).active[d.target, envs].all() and not d.reset.any()
    assert not cr.census(cfg, cr.shifted(d, obstacle, 4 * cr.CULL_EPS), obstacle, forces=False).active[:, free].any()
    assert free.sum() >= free.size - 2 * sum(map(cr.never_alone, d.features)) - 0.01 * free.size


def test_graph_captures_keep_the_collector_at_rest():
    """learning/graph_capture.py collector_at_rest: a dead cycle's finaliser runs in front of the body, none inside it, and
    the collector is back on behind it (also behind an exception)."""
    import gc

    from vine_robot_isaacgymenvs_amd.learning.graph_capture import collector_at_rest
    ran = []

    class Owner:
        def __del__(self):
            ran.append(gc.isenabled())

    def cycle():
        a = Owner()
        a.me = a
    gc.collect()
    cycle()
    with collector_at_rest():
        assert ran == [True] and not gc.isenabled()
        cycle()
        [[] for _ in range(100000)]
        assert ran == [True]
    assert gc.isenabled()
    gc.collect()
    assert len(ran) == 2
    with pytest.raises(ZeroDivisionError), collector_at_rest():
        1 / 0
    assert gc.isenabled()
