"""tests/mpc_reference.py with the oracle builds alone: every case of tests/test_mpc_record_gpu.py with a float32 host
controller (``HostController``: ``OracleDevice`` handles, ``fork_reference``, ``sample_actions``, ``cost_sums``, ``mpc_replay``)
in the device's place.  What is pinned here, without a GPU: every comparison of the replay passes; the caps hold with the two
oracles alone (undecided env-steps, kept share, left-out plant-windows; a sample dies by time-out and one by the rail limit
inside a window, a plant's reset is consumed by an update); every negative control breaks its bound by ``CONTROL_MARGIN``; and
``fork_reference`` reproduces, for delays 0..8 and two step counts, the ring an oracle leaves after stepping through the same
actions.  The seeds and episode lengths of the cases were chosen here."""
import numpy as np
import pytest

from oracle import vine_oracle as vo
from tests import env_params_sets
from tests import mpc_reference as mr
from tests import step_reference as sr
from vine_robot_isaacgymenvs_amd import abi

CONTROLS_OF = {"params9": ("history_shift", "rotated_sets", "progress_zero", "cost_drop", "action_next"),
               "inertia9": ("ignore_inertia",)}


def test_constants():
    assert mr.CONTROL_MARGIN == 4.0 and mr.WEIGHT_BOUND == 1e-12 and mr.ENTROPIC_BOUND <= 1e-12
    for c in mr.CASES:
        assert c.model is None or c.K % mr.NUM_SETS == 0, c.name         # sample j of every plant carries set j % 9
        assert c.K % c.members == 0 and (c.model is None or c.M * c.K <= 2 * 27)
    assert [c.name for c in mr.CASES][:2] == ["params9", "inertia9"] and mr.CASES[0].episode == 7
    assert set(sum(CONTROLS_OF.values(), ())) == set(mr.CONTROLS)


@pytest.mark.parametrize("count", [11, 16])       # (the oracle starts MAX_DELAY steps earlier, at a count that is not negative)
def test_fork_reference_reproduces_the_ring_an_oracle_leaves(count):
    """Nine oracles with delays 0..8 (tests/env_params_sets.py: the delay of set g is g) step through eight random actions and
    end at ``count``; ``fork_reference`` with the same actions as the history (most recent first) holds the same words in the
    slots below the delay, in both precisions, and the prior's above."""
    M, K = 2, 9
    cfg = mr.model_cfg(mr.CASES[0])
    cfg.num_envs = M * K
    cfgs = [env_params_sets.set_cfg(cfg, g) for g in range(9)]
    delays = np.arange(M * K) % 9                        # also the index of each sample's configuration
    assert np.array_equal(mr.sample_delays(cfgs, delays), delays)
    rng = np.random.default_rng(count)
    acts = rng.uniform(-1.3, 1.3, (abi.MAX_DELAY, M, 2)).astype(np.float32)
    history = np.ascontiguousarray(acts[::-1].transpose(1, 0, 2))
    plant_state = rng.uniform(-1, 1, (abi.VF_COUNT, M))
    prior = np.full((abi.VF_COUNT, M * K), mr.SENTINEL)
    for precision in ("f32", "f64"):
        got = mr.fork_reference(plant_state, history, count, delays, cfgs, delays, precision, prior)
        for g in range(9):
            o = vo.OracleEnv(cfgs[g], precision)
            o.step_count = count - abi.MAX_DELAY
            for a in acts:
                o.step(np.repeat(a, K, axis=0))
            assert o.step_count == count
            ring = np.array(o.state[mr.RING0:mr.RING1], np.float64)
            o.close()
            for e in range(g, M * K, 9):
                assert np.array_equal(got[mr.RING0:mr.RING0 + 2 * g, e], ring[:2 * g, e]), (precision, g, e)
                assert np.all(got[mr.RING0 + 2 * g:mr.RING1, e] == mr.SENTINEL)
        assert np.array_equal(got[mr.NOT_RING], plant_state[mr.NOT_RING][:, np.arange(M * K) // K])
        # the age order undoes the step count: the same rows at another count
        other = mr.fork_reference(plant_state, history, count + 3, delays, cfgs, delays, precision, prior)
        assert np.array_equal(mr.ring_group(got, count, delays), mr.ring_group(other, count + 3, delays))
        assert not np.array_equal(got[mr.RING0:mr.RING1], other[mr.RING0:mr.RING1])


@pytest.mark.parametrize("case", mr.CASES, ids=mr.CASE_IDS)
def test_oracles_alone(case):
    controls = CONTROLS_OF.get(case.name, ())
    res, clip = mr.run_case(case, mr.HostController, controls)
    print("\n" + "\n".join(mr.lines(case, res, clip)))
    mr.check_caps(case, res)
    # the stand-in IS the float32 oracle: its ratio is 1 wherever the baseline is above the floor
    for tally in (res.model, res.plant):
        ratios, _, base = sr.report(tally)
        k, w = sr.worst(sr.unscaled(ratios))
        assert w <= 1.0 + 1e-12, (k, w)
    assert {k[1] for k in sr.report(res.model)[2]} == set(sr.GROUP_NAMES)
    rr, _ = mr.ring_report(res)
    assert max(rr) <= 1.0 / sr.K_STEP + 1e-12
    # ... and its decision is the float32 planner's rounded to float32 once more: error <= float32 planner's + 2^-24 clipActions
    assert mr.worst_decision_ratio(mr.decision_report(res, clip)) <= 2.0
    mr.check_bounds(case, res, clip)
    margins = mr.control_margins(case, res, clip, controls)
    if controls:
        print("[mpc record] %s controls (error against the wrong reference / bound): %s" % (
            case.name, ", ".join("%s %.3g (%s)" % (n, m[1], m[0]) for n, m in margins.items())))
    weak = {n: m for n, m in margins.items() if not m[1] >= mr.CONTROL_MARGIN}
    assert not weak, ("negative control within the bound", case.name, weak)
    assert len(margins) >= len(controls)
