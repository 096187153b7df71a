"""tests/step_reference.py with the oracle builds alone: every case and route of tests/test_step_dynamics_gpu.py with the
float32 oracle standing in for the device.  What is pinned here, without a GPU: the float32 baseline is finite on every group,
the two oracles leave at most 1 % of the env-steps undecided and at least half the envs in ``kept``, every negative control
breaks ``CONTROL_MARGIN x K_STEP x`` baseline on some group, and the composite of nine oracles is the nine oracles column for
column."""
import numpy as np
import pytest

from oracle import vine_oracle as vo
from tests import step_reference as sr
from tests.env_inertia_sets import NUM_SETS, set_cfg
from vine_robot_isaacgymenvs_amd import abi


def _device(cfg, route):
    return sr.OracleDevice(sr.route_cfgs(cfg, route))


def test_constants_leave_room_for_the_controls():
    """K_STEP x CONTROL_MARGIN stays below the weakest control's oracle-only ratio (24 x: link_inertia[1] x 1.01 on ``w`` in
    effort_limit mode; test_oracles_alone measures every control of every mode against the bound itself), and the constant
    of the joint-coordinate groups below the 59 x of link_mass[2] x 1.001 on ``qd``."""
    assert sr.FLOOR == 2.0 ** -24 and sr.CONTROL_MARGIN == 4.0
    assert sr.K_STEP * sr.CONTROL_MARGIN < 24.0 and sr.K_STEP < sr.K_JOINT and sr.K_JOINT * sr.CONTROL_MARGIN < 59.0
    assert set(sr.K_OF) == {"q", "qd", "obs"}


def test_groups_cover_the_named_fields():
    n = 5
    state = np.arange(abi.VF_COUNT * n, dtype=np.float64).reshape(abi.VF_COUNT, n)
    g = sr.groups(state, np.zeros((n, 28)), np.zeros(n), np.zeros((n, abi.NUM_REWARDS)))
    assert set(g) == set(sr.GROUP_NAMES) and len(g) == len(sr.GROUP_NAMES)
    assert np.array_equal(g["th"][2], state[abi.VF_Q0 + 1] + state[abi.VF_Q0 + 2] + state[abi.VF_Q0 + 3]) and g["w"].shape == (5, n)
    assert {k: v.shape for k, v in g.items()} == {"q": (6, n), "qd": (6, n), "tip": (2, n), "tipv": (2, n), "cart": (4, n),
                                                  "cmd": (4, n), "prev_tip": (2, n), "rail_force": (1, n), "agg_rew": (1, n),
                                                  "th": (5, n), "w": (5, n), "obs": (28, n), "rew": (1, n), "rmat": (abi.NUM_REWARDS, n)}
    assert np.array_equal(g["tipv"], state[[abi.VF_TIP_VY, abi.VF_TIP_VZ]])
    off = sr.groups(state, np.zeros((n, 28)), np.zeros(n), np.zeros((n, abi.NUM_REWARDS)), introspect=False)
    assert tuple(off) == ("q", "qd", "cart", "cmd", "agg_rew", "th", "w", "obs", "rew")
    stacked = sr.groups(np.stack([state, state]), np.zeros((2, n, 28)), np.zeros((2, n)), None)
    assert stacked["q"].shape == (2, 6, n) and stacked["obs"].shape == (2, 28, n) and "rmat" not in stacked


@pytest.mark.parametrize("case,route", sr.CASE_ROUTES, ids=sr.CASE_ROUTE_IDS)
def test_oracles_alone(case, route):
    """Parts "a" and "b" of a case and route; the controls on the first case of each physics mode (one-lane route)."""
    with_controls = case.controls and route == "lane"
    for part in sr.PARTS:
        tally, names = sr.run_case(case, route, _device, part, with_controls=with_controls and part == "a")
        ratios, margins, base = sr.report(tally, names)
        total = tally.steps * sr.N_ENVS
        assert {k[1] for k in base} == set(sr.GROUP_NAMES), (part, sorted(base))
        assert tally.count["bad"] == 0
        assert tally.count["undecided"] <= sr.MAX_UNDECIDED * total, (part, tally.count)
        assert tally.count["kept"] >= sr.MIN_KEPT * total, (part, tally.count)
        if not case.obstacle:
            assert tally.count["reset"] > 0 and tally.count["contact"] == 0, (part, tally.count)
        # the stand-in IS the float32 oracle: its ratio is 1 / K_STEP wherever the baseline is above the floor
        k, w = sr.worst(sr.unscaled(ratios))
        assert w <= 1.0 + 1e-12, (part, k, w)
        print("%s %s part %s: %s, worst float32 error %s" % (case.name, route, part, dict(tally.count),
                                                             max((max(v), k) for k, v in base.items())))
        if part == "a" and with_controls:
            print("  controls (error against the wrong oracle / bound): " +
                  ", ".join("%s %.0f (%s %s)" % (n, m[2], m[0], m[1]) for n, m in margins.items()))
            weak = {n: m for n, m in margins.items() if not m[2] >= sr.CONTROL_MARGIN}
            assert not weak, ("negative control within the bound", case.name, weak)
            assert len(margins) >= 17 and {"gravity", "link_mass[2]", "link_inertia[1]", "armature"} <= set(margins)


def test_composite_reproduces_nine_uniform_oracles():
    """Env e of ``composite`` is env e of oracle e % 9, column for column, after a step that resets and times out."""
    case = sr.CASES[0]
    cfg = sr.case_cfg(case)
    n = cfg.num_envs
    rng = np.random.default_rng(3)
    dev = sr.OracleDevice([cfg])
    sr.seed_device(dev, case, cfg, rng)
    oracles = [vo.OracleEnv(set_cfg(cfg, g), "f64") for g in range(NUM_SETS)]
    acts = rng.uniform(-1.3, 1.3, (n, 2)).astype(np.float32)
    for o in oracles:
        o.bind_reward_matrix()
        o.state[:] = dev.state
        o.reset_buf[:], o.progress[:], o.step_count = dev.reset_buf, dev.progress, 7
        o.step(acts)
    c = sr.composite(oracles, n)
    assert c.reset_buf.sum() > 0 and c.timeouts.sum() > 0
    for e in range(n):
        o = oracles[e % NUM_SETS]
        assert np.array_equal(c.state[:, e], np.asarray(o.state, np.float64)[:, e])
        assert np.array_equal(c.obs[e], o.obs[e]) and c.rew[e] == o.rew[e] and np.array_equal(c.reward_matrix[e], o.reward_matrix[e])
        assert c.reset_buf[e] == o.reset_buf[e] and c.progress[e] == o.progress[e] and c.timeouts[e] == o.timeouts[e]
    assert not np.array_equal(c.state[abi.VF_Q0:abi.VF_Q0 + 6, 0], np.asarray(oracles[1].state)[abi.VF_Q0:abi.VF_Q0 + 6, 0])
    dev.close()
    for o in oracles:
        o.close()
