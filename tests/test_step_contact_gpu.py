"""The obstacle contacts of vine_step_kernel and vine_step_quad_kernel held to float32 round-off of the float64 oracle,
feature by feature (tests/contact_reference.py has the features, the directed states, the classes and the metric;
tests/test_contact_reference.py runs every part below with the float32 oracle in the device's place).

Cases ``pipe`` (560 envs), ``shelf`` (320), ``shelf+pipe`` (880): two envs per feature, env e targets feature e mod count,
links interleaved so that every wave and workgroup starts with contacts of five different links.  Routes ``lane`` and
``quad`` for all three and ``lane+params`` for ``pipe``, each asserted by ``vine_step_kernel_name``.

(a) Short step (dt / 10, one substep, control_freq_inv 4): one step from the directed states and three teacher-forced
    steps.  Per class (``kept``, ``reset``, ``contact``), group (step_reference.GROUP_NAMES and ``contact`` = VF_CONTACT,
    VF_CONTACT_MEAN) and norm: error <= ``K_CONTACT x max(float32 oracle's error, 2^-24)``.  Asserted conditions: ``near``
    (margin below 2^-20 m in the float64 oracle) <= 1 % of the env-steps, every feature active in a compared ``contact``
    env, flags / progress / time-outs equal to the float64 oracle's on every decided env (with a shelf the
    non-zero-contact-force reset is on).
(b) Full step (production dt and substeps), one step from the directed states with no reset flag set: per group of
    ``contact_reference.FULL_GROUPS`` the median and the 99th percentile of the per-env error over the ``contact`` class are
    at most 2 x the float32 oracle's plus one float32 ulp of the group's range; ``near`` + ``undecided`` <= 6 %.  Every feature
    is compared but those whose envs are all ``near`` (at most 1 % of the features; printed).
(c) Negative controls on (a), ``lane`` route: the float64 oracle rebuilt with one factor of its contact probe at 1.001
    (``contact_reference.PROBES``); the device against it must break the bound by ``CONTROL_MARGIN`` on some group of the
    ``contact`` class.
(d) Culling is exact, ``lane`` route: every env's obstacle moved to the targeted feature's
    zero-penetration pose -/+ 4 x PIPE_CULL_EPS along the feature's normal.  Inside and outside, the step is the oracle's
    within the bound of (a).  Bit for bit: most directed envs hold further contacts beside the targeted one, so the outside
    pose is also built from states of its own (``contact_reference.isolated``: posture and placement redrawn until the
    targeted feature is the env's only contact and the float64 oracle finds the whole step from the outside pose free); on
    every such env the step equals the step of the same state without the obstacle bit for bit.  Every feature has such an
    env but the ten strip-corner features of ``contact_reference.never_alone`` (the strip's other corner lies inside the same
    link), asserted.

Measured on an MI355X, part (a): kernel error / max(float32 oracle's error, 2^-24), the worst group and norm per class
    case and route          contact               kept               reset              near
    pipe lane               1.187 (qd)            3.294 (q)          1.041 (cart)       0.31 %
    pipe quad               1.155 (q)             3.069 (q)          1.395 (tipv)       0.31 %
    pipe lane+params        1.149 (w)             3.070 (q)          1.027 (tip)        0.27 %
    shelf lane              1.331 (th)            1.766 (q)          1.003 (cart)       0.31 %
    shelf quad              1.141 (q)             1.877 (q)          1.000 (rew)        0.31 %
    shelf+pipe lane         1.051 (q)             1.732 (q)          0.953 (rail_force) 0.14 %
    shelf+pipe quad         1.123 (q)             1.848 (q)          0.841 (q)          0.14 %
hence K_CONTACT = 4.95 (1.5 x 3.294).  The worst figure is a joint angle of an env that touches nothing (the kernels integrate
absolute link angles: tests/step_reference.py has the reason and the same figure, 3.8, for free space); in contact the
kernels are as close to float64 as the float32 oracle to within 1.36, on every feature, and no group comes near K_JOINT.
Part (d): against the oracle 1.05 - 1.36 in the ``contact`` class at either pose, at most 2.29 elsewhere; bit for bit 560 of
560, 299 of 320 and 860 of 880 isolated envs free of contact and identical to free space, every feature among them but the
ten of ``never_alone``.  Part (b): per-env error of the kernel / of the float32 oracle 0.71 - 1.69 at the median (the largest:
obs, shelf, one-lane kernel) and 0.66 - 1.69 at the 99th percentile (rew, shelf, four-lane kernel; the rule allows 2 x + one
ulp), near + undecided 2.1 - 4.5 %; one feature of 440 (shelf+pipe: point 0 of link 3 in wall 1, end face) has both its envs
``near`` and is not compared there.  Part (c), device against the wrong oracle / bound at K_CONTACT: contact_c x 1.001 10.9
(shelf) - 14.7, link0_overhang 27 - 43, board_hz 49, contact_k 101 and more, pipe_wall 78 and more, every other factor above
1000 (a wall or a link side that moves by 0.1 % of its place moves a penetration of 0.2 - 2 mm by tens of per cent); no factor
needs 1.01.
Each run prints its figures; profiles/step_contact/ratios.txt has every group of every case, route and part.
"""
import pytest

from tests import contact_reference as cr
from tests import test_step_dynamics_gpu as dyn

pytestmark = pytest.mark.gpu


def _device(cfg, route):
    """tests/test_step_dynamics_gpu.py's handle on ``route`` (kernel forced and asserted, tables bound).  The four-lane kernel
    covers the obstacles: a ``quad`` route the library does not dispatch is a failure here, not a skip."""
    try:
        return dyn._device(cfg, route)
    except pytest.skip.Exception as e:
        pytest.fail("route %s: %s" % (route, e))


@pytest.mark.parametrize("obstacle,route", cr.CASE_ROUTES, ids=["%s-%s" % cr_ for cr_ in cr.CASE_ROUTES])
def test_contacts_short_step(obstacle, route):
    """Parts (a) and, on the ``lane`` route, (c)."""
    tally, names, log, d = cr.run_short(obstacle, route, _device, with_controls=route == "lane")
    cr.check_short("%s %s (a)" % (obstacle, route), tally, names, log, d.state.shape[1], len(d.features))
    assert tally.steps == cr.STEPS and tally.count["reset"] > 0
    if route == "lane":
        assert set(names) == set(cr.PROBES_OF[obstacle])


@pytest.mark.parametrize("obstacle,route", cr.CASE_ROUTES, ids=["%s-%s" % cr_ for cr_ in cr.CASE_ROUTES])
def test_contacts_full_step(obstacle, route):
    """Part (b)."""
    tally, log, d = cr.run_full(obstacle, route, _device)
    cr.check_full("%s %s (b)" % (obstacle, route), tally, log, d.state.shape[1], len(d.features))


@pytest.mark.parametrize("obstacle", list(cr.CASES))
def test_culling_is_exact(obstacle):
    """Part (d)."""
    for shift in (-4 * cr.CULL_EPS, 4 * cr.CULL_EPS):
        tally, _, log, d = cr.run_short(obstacle, "lane", _device, shift=shift)
        cr.check_shifted("%s lane (d), shift %+.0e m" % (obstacle, shift), tally, log, d, shift)
    with_, without, free, d = cr.run_outside(obstacle, _device)
    cr.check_outside("%s lane (d)" % obstacle, with_, without, free, d)
