"""vine_step_kernel and vine_step_quad_kernel held to float32 round-off of the float64 oracle (tests/step_reference.py).

328 envs (5 x 64 + 8: a partial last wave and a partial last workgroup on both kernels).  Four routes, each asserted by
``vine_step_kernel_name`` and the two ``..._bound`` entries: the one-lane kernel, the four-lane kernel (skipped where
``use_quad_kernel`` does not cover the configuration, as tests/test_hip_parity.py skips), the one-lane kernel with the
heterogeneous parameter table of tests/env_params_sets.py, and with the configuration's own parameter rows beside the
heterogeneous inertia table of tests/env_inertia_sets.py (env e carries set e % 9; the reference is nine oracles).

Cases (``step_reference.CASES``): default physics with randomisation (noise 0.01 / 0.02, dynamics scaling 0.9 - 1.1), delay
1, on all four routes; default physics without randomisation, TIP_AND_CART_AND_OBJ_INFO, delay 0; every other physics mode
at delay 3 (the inertia route for ``stiffness`` and ``explicit_extras``, where the substep reads I[] from the table); the
four unscaled observation layouts; pipe and shelf placed around the tips (``kept`` envs only).  Per case and route: (a) one
step from a random mid-episode state with resets and a time-out block, step count 7, reward matrix bound; (b) six
teacher-forced steps with 4-step episodes, the oracles loaded with the device's state, flags, progress and step count in
front of every step.  Flags, progress and time-outs equal the float64 oracle's on every decided env; every group's error is
at most ``K_STEP x max(float32 oracle's error, 2^-24)`` in both norms (``K_JOINT`` for q, qd and obs: the kernels integrate
absolute link angles, tests/step_reference.py has the reason), for the envs that kept their state and, as a group set of
its own, for those that re-drew it; on the first default case also with introspection off (part (a): the oracles read
the tip in front of a step from the state block).  On the first case of each physics mode the float64 oracle rebuilt with
one constant off by 0.1 % (1 % for the two weakest) or one probe switch set must break the bound by ``CONTROL_MARGIN``.

Measured on an MI355X: kernel error / max(float32 oracle's error, 2^-24), the worst class, group and norm of each case and
route over parts (a) and (b), for the joint-coordinate groups and for every other group:
    case and route                                   q, qd, obs              every other group
    default lane                                    3.753 (kept q)           2.081 (kept th)
    default quad                                    3.744 (kept q)           2.081 (kept th)
    default lane+params                             3.818 (kept obs)         1.797 (kept th)
    default lane+params+inertia                     2.954 (kept obs)         1.996 (kept th)
    default_tipobs lane                             3.799 (kept qd)          2.185 (kept th)
    default_tipobs quad                             3.251 (kept qd)          2.213 (kept th)
    held lane                                       4.189 (kept obs)         1.802 (kept th)
    held quad                                       4.189 (kept obs)         1.950 (kept th)
    explicit lane                                   1.678 (kept qd)          1.420 (kept w)
    stiffness lane                                  3.488 (kept q)           1.477 (kept th)
    stiffness lane+params+inertia                   5.116 (kept q)           1.957 (kept th)
    linkdamp lane                                   3.065 (kept q)           1.586 (kept th)
    explicit_extras lane                            2.316 (kept qd)          2.016 (kept w)
    explicit_extras lane+params+inertia             3.038 (kept q)           2.727 (reset rail_force)
    effort_limit lane                               5.618 (kept qd)          2.963 (kept w)
    effort_limit quad                               5.757 (kept qd)          3.368 (kept w)
    obs_pos_only lane                               4.764 (kept q)           2.137 (kept th)
    obs_pos_and_vel lane                            3.420 (kept q)           2.135 (kept th)
    obs_pos_and_fd_vel lane                         5.655 (kept q)           2.250 (kept th)
    obs_pos_and_prev_pos lane                       3.132 (kept qd)          2.316 (kept th)
    pipe lane                                       1.454 (kept q)           1.597 (kept th)
    shelf lane                                      1.800 (kept q)           2.024 (kept cart)
    default lane (a, introspection off)             3.016 (kept qd)          1.438 (kept th)
    default quad (a, introspection off)             2.851 (kept qd)          1.351 (kept th)
    default lane+params (a, introspection off)      3.818 (kept obs)         1.373 (kept th)
    default lane+params+inertia (a, introspection off)  2.954 (kept obs)         1.996 (kept th)
hence K_JOINT = 8.7 (1.5 x 5.76) and K_STEP = 5.1 (1.5 x 3.37).  The four-lane kernel does not cover explicit, stiffness,
linkdamp and explicit_extras (those routes skip).  No env-step of any case was undecided.  The weakest negative controls on
the device, as error against the wrong oracle / bound: link_inertia[1] x 1.01 5 (effort_limit) to 37, link_angular_damping
x 1.01 6 and 10, link_mass[2] x 1.001 10 to 43, mostly on ``w``; every other control 26 and more.  Each run prints its figures;
profiles/step_dynamics/ratios.txt has every group of every case, the controls and the rollout record's env steps.
"""
import numpy as np
import pytest
import torch

from tests import env_inertia_sets, env_params_sets
from tests import step_reference as sr
from vine_robot_isaacgymenvs_amd import abi
from vine_robot_isaacgymenvs_amd.utils import env_params

pytestmark = pytest.mark.gpu

KERNEL_OF = {"lane": "vine_step_kernel", "quad": "vine_step_quad_kernel", "lane+params": "vine_step_kernel",
             "lane+params+inertia": "vine_step_kernel"}


def _upload(dev, table, rows, check):
    check(dev.lib, dev.cfg, table)
    t = torch.as_tensor(np.ascontiguousarray(table, np.float32)).to(dev.dev).contiguous()
    assert t.shape == (rows, dev.n)
    torch.cuda.synchronize(dev.dev)
    return t


def _device(cfg, route):
    """A handle on ``route``: the kernel forced, the route's tables bound, the route asserted."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    from tests.hip_env import HipEnv
    dev = type("HipEnv_" + route, (HipEnv,), {"kernel": "quad" if route == "quad" else "lane"})(cfg)
    lib = dev.lib
    name = lambda: lib.vine_step_kernel_name(dev.h).decode()                                   # noqa: E731
    if route == "quad" and name() != "vine_step_quad_kernel":
        dev.close()
        pytest.skip("vine_step_quad_kernel does not cover this configuration (runs as the 'lane' case)")
    if route in ("lane+params", "lane+params+inertia"):
        params = (env_params_sets.table_of(lib, dev.cfg, dev.n) if route == "lane+params" else
                  np.repeat(env_params.config_row(lib, dev.cfg)[:, None], dev.n, axis=1))
        dev.params_t = _upload(dev, params, abi.VP_COUNT, env_params.check_table)
        assert lib.vine_bind_env_params(dev.h, dev.params_t.data_ptr()) == abi.OK
    if route == "lane+params+inertia":
        dev.inertia_t = _upload(dev, env_inertia_sets.table_of(lib, dev.cfg, dev.n), abi.VI_COUNT, env_params.check_inertia_table)
        assert lib.vine_bind_env_inertia(dev.h, dev.inertia_t.data_ptr()) == abi.OK
    assert name() == KERNEL_OF[route], (route, name())
    assert lib.vine_env_params_bound(dev.h) == int("params" in route), route
    assert lib.vine_env_inertia_bound(dev.h) == int("inertia" in route), route
    return dev


def _check(title, tally, names=()):
    """Prints every figure, then asserts the classes' sizes, the bound and the controls."""
    ratios, margins, base = sr.report(tally, names)
    total = tally.steps * sr.N_ENVS
    raw = sr.unscaled(ratios)
    k, w = sr.worst(raw)
    print("\n" + sr.table("%s: kernel error / max(float32 oracle's error, FLOOR); classes %s; worst %.3f (%s %s)"
                          % (title, dict(tally.count), w, k[0], k[1]), raw), flush=True)
    if names:
        print("[step dynamics] %s: controls, error against the wrong oracle / bound: %s"
              % (title, ", ".join("%s %.0f (%s %s)" % (n, m[2], m[0], m[1]) for n, m in margins.items())), flush=True)
    assert tally.count["bad"] == 0
    assert tally.count["undecided"] <= sr.MAX_UNDECIDED * total, (title, tally.count)
    assert tally.count["kept"] >= sr.MIN_KEPT * total, (title, tally.count)
    bad = {key: (round(v[0], 3), round(v[1], 3)) for key, v in ratios.items() if not max(v) <= 1.0}
    assert not bad, (title, "kernel error above K_STEP = %g (q, qd, obs: K_JOINT = %g) x max(float32 oracle's error, FLOOR): "
                     "error / bound" % (sr.K_STEP, sr.K_JOINT), bad)
    weak = {n: m for n, m in margins.items() if not m[2] >= sr.CONTROL_MARGIN}
    assert not weak, (title, "negative control within the bound", weak)
    return ratios


@pytest.mark.parametrize("case,route", sr.CASE_ROUTES, ids=sr.CASE_ROUTE_IDS)
def test_step_is_float32_round_off_of_the_float64_oracle(case, route):
    """Parts (a) and (b) of a case on a route; the negative controls on the first case of each physics mode (one-lane route,
    part (a))."""
    with_controls = case.controls and route == "lane"
    for part in sr.PARTS:
        tally, names = sr.run_case(case, route, _device, part, with_controls=with_controls and part == "a")
        ratios = _check("%s %s (%s)" % (case.name, route, part), tally, names)
        assert {k[1] for k in ratios} == set(sr.GROUP_NAMES)
        if not case.obstacle:
            assert tally.count["reset"] > 0
        if with_controls and part == "a":
            assert len(names) >= 17


@pytest.mark.parametrize("route", sr.ROUTES)
def test_step_without_introspection(route):
    """The first default case with introspection off (the branch training runs): what the step still stores -- the DOF state,
    the controller's and the filter's memory, the aggregated reward -- and its outputs, part (a)."""
    case = sr.CASES[0]
    assert case.introspect_off and route in case.routes
    tally, _ = sr.run_case(case, route, _device, "a", introspect=False)
    ratios = _check("%s %s (a, introspection off)" % (case.name, route), tally)
    assert {k[1] for k in ratios} == {"q", "qd", "th", "w", "cart", "cmd", "agg_rew", "obs", "rew"}
