"""GPU parity tests proper: the HIP path (through the C ABI of libvine_hip.so) against the CPU oracle on
identical seeded inputs, against the golden fixtures made from the reference's Python, and -- at
BASELINE.json's full size -- through size-independent properties.

Tolerances (north_star: "stated fp32 tolerance"): integer outputs (reset/progress/time_outs) bit-exact;
single-step float outputs vs the float32 oracle (same formulation) 2e-5 abs on positions, 2e-3 on velocities; vs the
float64 oracle 1e-4 / 1e-2.  These are coarse: over one step the float32 oracle is within 2e-7 .. 1.2e-6 of the float64
oracle, relative to each group's largest value (q 2.9e-7, qd 3.8e-7, tip velocity 6.2e-7, rail force 8.1e-7, obs 1.2e-6; at
worst 3.5e-6, obs in the explicit-damping modes), despite the mass matrix's condition number of ~1e3-1e4, so 2e-3 on
velocities of magnitude 3 - 10 is several hundred times float32 round-off and a constant wrong by 0.1 % passes.
tests/test_step_dynamics_gpu.py holds both step kernels to that round-off (tests/step_reference.py).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import vine_oracle as vo
from vine_robot_isaacgymenvs_amd import abi
from tests.helpers import F6_CASES, base_cfg, f6_cfg, random_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["lane", "quad"])
def HipEnv(request):
    """The product library through its C ABI, once per step kernel: "lane" = one env per lane (vine_step_kernel),
    "quad" = four lanes per env (vine_step_quad_kernel) wherever that kernel applies (control_freq_inv 4, implicit joint
    damping without the stiffness / link-damping extras, the two scalable observation layouts, no per-env parameter
    table; obstacles are covered; the library silently takes the one-lane kernel elsewhere)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    from tests.hip_env import HipEnv as H

    def init(self, cfg, device_id=0):
        # the kernel the library REALLY dispatches for this configuration: a "quad" case the four-lanes-per-env kernel
        # does not cover is skipped (it would silently repeat the "lane" case), a "lane" case must be the one-lane kernel
        H.__init__(self, cfg, device_id)
        name = self.lib.vine_step_kernel_name(self.h).decode()
        if request.param == "quad" and name != "vine_step_quad_kernel":
            self.close()
            pytest.skip("vine_step_quad_kernel does not cover this configuration (runs as the 'lane' case)")
        assert name == {"lane": "vine_step_kernel", "quad": "vine_step_quad_kernel"}[request.param], name

    return type("HipEnv_" + request.param, (H,), {"kernel": request.param, "__init__": init})


# Physics-model switches of the step kernel: every instantiation of the substep loop
# (vine_hip.hip VINE_SUBSTEP_LOOP: implicit x extras) and the literal held-torque actuation of V5:1043-1062.
# The explicit-damping modes are only stable for weak joint damping / torque feedback (that is assumption P2), hence the
# scaled-down FPAM coefficients there: the point is HIP-vs-oracle parity of the code path, not the reference's tuning.
def _explicit(cfg):
    cfg.set_flag(abi.FLAG_IMPLICIT_JOINT_DAMPING, False)
    cfg.damping = 0.003
    for i in range(5):
        cfg.fpam_C[i] = 0.0
        cfg.fpam_K[i] *= 0.1


def _held(cfg):
    cfg.damping = 0.08
    cfg.set_flag(abi.FLAG_FPAM_DAMPING_HELD, True)


def _stiff(cfg):
    cfg.stiffness = 0.5


def _linkdamp(cfg):
    cfg.link_angular_damping = 0.5


def _explicit_extras(cfg):
    _explicit(cfg)
    cfg.stiffness, cfg.link_angular_damping = 0.05, 0.5


def _effort_limit(cfg):
    cfg.effort_limit = 0.05


PHYSICS_MODES = {"default": lambda cfg: None, "held": _held, "explicit": _explicit, "stiffness": _stiff,
                 "linkdamp": _linkdamp, "explicit_extras": _explicit_extras, "effort_limit": _effort_limit}


def pair(HipEnv, cfg, precision="f32"):
    return HipEnv(cfg), vo.OracleEnv(cfg, precision)


def seed_both(hip, orc, rng, n, cfg):
    st = random_state(rng, n, cfg)
    hip.set_state(st)
    orc.state[:] = st.astype(orc.real)
    reset = (rng.uniform(size=n) < 0.15).astype(np.int64)
    progress = rng.integers(0, cfg.max_episode_length - 1, n)
    progress[: n // 16] = cfg.max_episode_length - 2      # a block of envs hits the time limit this step
    hip.set_flags(reset, progress)
    orc.reset_buf[:] = reset
    orc.progress[:] = progress
    return st


QPOS = slice(abi.VF_Q0, abi.VF_Q0 + 6)
QVEL = slice(abi.VF_QD0, abi.VF_QD0 + 6)


def compare_step(hip_out, orc, hip, pos_tol, vel_tol, obs_tol):
    obs, rew, rst, to = hip_out
    hs, os_ = hip.state, orc.state.astype(np.float64)
    np.testing.assert_array_equal(rst, orc.reset_buf)
    np.testing.assert_array_equal(hip.progress, orc.progress)
    np.testing.assert_array_equal(to, orc.timeouts)
    np.testing.assert_allclose(hs[QPOS], os_[QPOS], rtol=0, atol=pos_tol)
    np.testing.assert_allclose(hs[QVEL], os_[QVEL], rtol=0, atol=vel_tol)
    for f in (abi.VF_TIP_Y, abi.VF_TIP_Z, abi.VF_CART_Y, abi.VF_TARGET_Y, abi.VF_TARGET_Z, abi.VF_SMOOTHED_U,
              abi.VF_U_FPAM, abi.VF_U_RAIL, abi.VF_PREV_U_RAIL, abi.VF_PREV_TIP_Y, abi.VF_PREV_TIP_Z):
        np.testing.assert_allclose(hs[f], os_[f], rtol=0, atol=pos_tol, err_msg="field %d" % f)
    for f in (abi.VF_TIP_VY, abi.VF_TIP_VZ, abi.VF_CART_VY, abi.VF_PREV_CART_VEL, abi.VF_PREV_CART_VEL_ERR):
        np.testing.assert_allclose(hs[f], os_[f], rtol=0, atol=vel_tol, err_msg="field %d" % f)
    np.testing.assert_allclose(hs[abi.VF_RAIL_FORCE], os_[abi.VF_RAIL_FORCE], rtol=1e-3, atol=30 * vel_tol)
    np.testing.assert_allclose(obs, orc.obs, rtol=0, atol=obs_tol)
    np.testing.assert_allclose(rew, orc.rew, rtol=1e-5, atol=max(1e-4, 0.2 * vel_tol))
    np.testing.assert_allclose(hs[abi.VF_AGG_REW], os_[abi.VF_AGG_REW], rtol=1e-5, atol=max(1e-3, 0.2 * vel_tol))


@pytest.mark.parametrize("obs_type", [0, 1])
@pytest.mark.parametrize("randomize", [False, True])
@pytest.mark.parametrize("delay", [0, 1, 3])
def test_single_step_matches_oracle(HipEnv, obs_type, randomize, delay):
    """One VecTask.step from identical random mid-episode states, incl. resets, time-outs, RNG draws."""
    single_step_case(HipEnv, obs_type, randomize, delay, "default")


@pytest.mark.parametrize("mode", [m for m in PHYSICS_MODES if m != "default"])
@pytest.mark.parametrize("randomize", [False, True])
def test_single_step_physics_modes_match_oracle(HipEnv, mode, randomize):
    """The same single-step comparison in every physics-model mode the task YAML can select (``physicsModel.*``,
    ``STIFFNESS``): the literal held-torque actuation of V5:1043-1062 (`held`: both kernels), explicit joint damping,
    joint stiffness, link angular damping, an effort clamp -- all four instantiations of the substep loop."""
    single_step_case(HipEnv, 0, randomize, 1, mode)


def single_step_case(HipEnv, obs_type, randomize, delay, mode):
    n = 1000   # ragged: not a multiple of the 64-wide workgroup
    cfg = base_cfg(n, obs_type, randomize, action_delay=delay, seed=1234 + delay)
    if randomize:
        cfg.obs_noise_std, cfg.action_noise_std = 0.01, 0.02
        cfg.dyn_scale_min, cfg.dyn_scale_max = 0.9, 1.1
    PHYSICS_MODES[mode](cfg)
    rng = np.random.default_rng(10 * obs_type + delay)
    for precision, tol in (("f32", (2e-5, 2e-3, 2e-3)), ("f64", (1e-4, 1e-2, 1e-2))):
        hip, orc = pair(HipEnv, cfg, precision)
        seed_both(hip, orc, rng, n, cfg)
        hip.step_count = 7
        orc.step_count = 7
        hip.bind_reward_matrix()
        orc.bind_reward_matrix()
        actions = rng.uniform(-1.3, 1.3, (n, 2))
        out = hip.step(actions)
        orc.step(actions)
        compare_step(out, orc, hip, *tol)
        np.testing.assert_allclose(hip.reward_matrix_t.cpu().numpy(), orc.reward_matrix, rtol=1e-4, atol=10 * tol[1])
        assert hip.step_count == 8
        assert orc.reset_buf.sum() > 0 and orc.timeouts.sum() > 0
        hip.close(); orc.close()


@pytest.mark.parametrize("force_fpam,force_rail", [(True, False), (False, True), (True, True)])
def test_manual_intervention_flags_match_oracle(HipEnv, force_fpam, force_rail):
    """FORCE_U_FPAM / FORCE_U_RAIL_VELOCITY (TY:25-26; manual_intervention, V5:1007-1026): the applied command is
    zeroed after the delay FIFO, before the smoothing filter."""
    n = 500
    cfg = base_cfg(n, 0, True, action_delay=1, seed=31)
    cfg.set_flag(abi.FLAG_FORCE_U_FPAM, force_fpam)
    cfg.set_flag(abi.FLAG_FORCE_U_RAIL_VELOCITY, force_rail)
    rng = np.random.default_rng(17)
    hip, orc = pair(HipEnv, cfg, "f32")
    seed_both(hip, orc, rng, n, cfg)
    hip.step_count = orc.step_count = 5
    for _ in range(2):
        actions = rng.uniform(-1.3, 1.3, (n, 2))
        out = hip.step(actions)
        orc.step(actions)
        compare_step(out, orc, hip, 2e-5, 2e-3, 2e-3)
    st = hip.state
    if force_fpam:
        assert (st[abi.VF_U_FPAM] == 0).all()
    else:
        assert np.abs(st[abi.VF_U_FPAM]).max() > 0.5
    if force_rail:
        assert (st[abi.VF_U_RAIL] == 0).all() and (st[abi.VF_PREV_U_RAIL] == 0).all()
    hip.close(); orc.close()


def test_introspection_gate(HipEnv):
    """VINE_FLAG_INTROSPECT off: the step produces bit-identical outputs and step-relevant state, and leaves the
    dashboard-only fields alone (they are ~70 B per env of HBM traffic the rollout does not need)."""
    n = 777
    cfg = base_cfg(n, 0, True, action_delay=1, seed=3)
    rng = np.random.default_rng(4)
    a, b = HipEnv(cfg), HipEnv(cfg)
    b.set_introspection(False)
    st = random_state(rng, n, cfg)
    marker = 123.0
    only = [abi.VF_TIP_VY, abi.VF_TIP_VZ, abi.VF_U_FPAM, abi.VF_U_RAIL, abi.VF_PREV_U_RAIL, abi.VF_RAIL_FORCE,
            abi.VF_PREV_TIP_Y, abi.VF_PREV_TIP_Z] + list(range(abi.VF_PREV_Q0, abi.VF_PREV_Q0 + 6))
    for f in only:
        st[f] = marker
    for env in (a, b):
        env.set_state(st)
        env.set_flags(np.zeros(n, np.int64), np.full(n, 5))
    # the four-lanes-per-env kernel goes one step further without introspection: the tip / cart rigid-body states are
    # re-derived from the DOF state (forward kinematics) instead of loaded, and stored only by envs that reset in the
    # step (the one case in which they are the only copy, P5) -- same values up to the rounding of sin / cos
    lazy = [abi.VF_TIP_Y, abi.VF_TIP_Z, abi.VF_CART_Y, abi.VF_CART_VY] if a.kernel == "quad" else []
    for t in range(3):
        acts = rng.uniform(-1, 1, (n, 2))
        oa, ob = a.step(acts), b.step(acts)
        for x, y in zip(oa, ob):
            if lazy and np.asarray(x).dtype.kind == "f":
                np.testing.assert_allclose(x, y, rtol=1e-5, atol=2e-5)
            else:
                np.testing.assert_array_equal(x, y)
    sa, sb = a.state, b.state
    noreset = (a.reset_buf == 0) & (a.progress == 8)            # envs that never went through reset_env
    assert noreset.sum() > n // 2
    fresh = a.progress == 0                                     # reset in the last step: their body states WERE stored
    for f in range(abi.VF_COUNT):
        if f in only:
            assert (sb[f][noreset] == marker).all(), f          # untouched without introspection
            assert not (sa[f][noreset] == marker).all(), f      # written with it
        elif f in lazy:
            np.testing.assert_array_equal(sb[f][noreset], st[f][noreset].astype(np.float32), err_msg="field %d" % f)
            np.testing.assert_allclose(sa[f][fresh], sb[f][fresh], rtol=1e-5, atol=1e-6, err_msg="field %d" % f)
        elif lazy:
            np.testing.assert_allclose(sa[f], sb[f], rtol=1e-5, atol=2e-5, err_msg="field %d" % f)
        else:
            np.testing.assert_array_equal(sa[f], sb[f], err_msg="field %d" % f)
    with pytest.raises(ValueError):
        b.stats()                                               # the dashboard vector needs the gated fields
    a.close(); b.close()


def test_dashboard_vector_matches_oracle(HipEnv):
    """vine_stats (two-stage reduction on the device) against the oracle's plain loops on the same state, incl. the
    shelf's contact entries and a non-trivial view index."""
    n = 3000
    cfg = base_cfg(n, 0, True, action_delay=1, seed=12)
    cfg.set_flag(abi.FLAG_CREATE_SHELF, True)
    rng = np.random.default_rng(6)
    hip, orc = pair(HipEnv, cfg, "f32")
    hip.bind_reward_matrix(); orc.bind_reward_matrix()
    st = seed_both(hip, orc, rng, n, cfg)
    st[abi.VF_SHELF_Y] = st[abi.VF_TIP_Y] - 0.2 - 0.05 + rng.uniform(-0.04, 0.04, n)
    st[abi.VF_SHELF_Z] = st[abi.VF_TIP_Z] + rng.uniform(-0.06, 0.06, n)
    hip.set_state(st); orc.state[:] = st.astype(orc.real)
    for t in range(3):
        a = rng.uniform(-1, 1, (n, 2))
        hip.step(a); orc.step(a)
    # identical inputs to both reductions: summarise the ORACLE's state with both implementations
    hip.set_state(orc.state.astype(np.float64))
    hip.rew_t.copy_(__import__("torch").as_tensor(orc.rew)); hip.progress_t.copy_(__import__("torch").as_tensor(orc.progress))
    hip.reward_matrix_t.copy_(__import__("torch").as_tensor(orc.reward_matrix))
    view = 1234
    got, want = hip.stats(view), orc.stats(view)
    assert want[abi.VS_CONTACT_NONZERO] > 0.01 and want[abi.VS_TARGET_REACHED] >= 0
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    np.testing.assert_array_equal(got[abi.VS_VIEW0:abi.VS_VIEW_U + 5], want[abi.VS_VIEW0:abi.VS_VIEW_U + 5])
    maxes = [abi.VS_MAX_ABS_TIP_Y, abi.VS_MAX_TIP_Z, abi.VS_TIP_VEL_MAX, abi.VS_REW_MAX]
    np.testing.assert_array_equal(got[maxes], want[maxes])
    hip.close(); orc.close()


def test_default_mode_observation_scales(HipEnv):
    """Sanity check against the only physics data the reference holds: per-channel RMS of the unscaled
    observations over 2000 random-policy steps of 4096 envs in the product's default mode, against the empirical
    observation scales of V5:246-255, within a factor 10 below / 3 above (a random policy moves less than a trained one;
    the CPU twin of this test sweeps the literal-mode switches: tests/test_oracle_physics.py)."""
    import torch
    from tests.test_oracle_physics import OBS_SCALE_REF, TIP_SCALE_REF
    n, T = 4096, 2000
    cfg = base_cfg(n, 0, True)
    native_check_set_obs_type(cfg, abi.OBS_POS_AND_FD_VEL_AND_OBJ_INFO, 0)
    cfg.clip_observations = 1e9
    hip = HipEnv(cfg)
    g = torch.Generator(device=hip.dev).manual_seed(1)
    s2 = torch.zeros(28, device=hip.dev, dtype=torch.float64)
    s1 = torch.zeros(28, device=hip.dev, dtype=torch.float64)
    cnt = torch.zeros((), device=hip.dev, dtype=torch.float64)
    for t in range(T):
        fresh = hip.reset_t != 0
        hip.step_t(torch.rand((n, 2), device=hip.dev, generator=g) * 2 - 1, sync=False)
        if t >= T // 4:
            keep = (~fresh).to(torch.float64).unsqueeze(1)
            o = hip.obs_t.to(torch.float64) * keep
            s2 += (o * o).sum(0); s1 += o.sum(0); cnt += keep.sum()
    rms = torch.sqrt(s2 / cnt).cpu().numpy()
    std_tip_y = float(torch.sqrt(s2[13] / cnt - (s1[13] / cnt) ** 2))
    ratios = np.concatenate([rms[:12] / OBS_SCALE_REF, np.array([std_tip_y, rms[16], rms[17]]) / TIP_SCALE_REF])
    assert np.isfinite(ratios).all() and 0.1 < ratios.min() and ratios.max() < 3.0, ratios
    assert float(hip.state_t[abi.VF_QD0 + 1:abi.VF_QD0 + 6].abs().max()) < 30
    hip.close()


@pytest.mark.parametrize("obstacle", ["shelf", "pipe", "shelf+pipe"])
def test_full_size_obstacle_properties(HipEnv, obstacle):
    """BASELINE configs[4]'s per-GPU share at FULL size (16384 envs, vine_randomize, ACTION_DELAY 1, shelf and / or pipe),
    300 random-policy steps, through size-independent properties: two runs from the same seed are
    bit-identical (no atomics, no order dependence at any occupancy), everything stays finite and bounded, the obstacle is
    really in play (shelf: a good share of env steps report a strip contact; pipe: the trajectories differ from the
    obstacle-free run of the same seed for a good share of the envs), and resets keep happening."""
    import torch
    n, T = 16384, 300
    def run(shelf, pipe):
        cfg = base_cfg(n, 0, True, action_delay=1, seed=123)
        cfg.set_flag(abi.FLAG_CREATE_SHELF, shelf)
        cfg.set_flag(abi.FLAG_CREATE_PIPE, pipe)
        hip = HipEnv(cfg)
        g = torch.Generator(device=hip.dev).manual_seed(9)
        touched = torch.zeros((), device=hip.dev, dtype=torch.float64)
        resets = torch.zeros((), device=hip.dev, dtype=torch.float64)
        for _ in range(T):
            hip.step_t(torch.rand((n, 2), device=hip.dev, generator=g) * 2 - 1, sync=False)
            touched += (hip.state_t[abi.VF_CONTACT_MEAN] > 0).double().sum()
            resets += (hip.reset_t != 0).double().sum()
        torch.cuda.synchronize()
        out = (hip.state_t.clone(), hip.obs_t.clone(), hip.rew_t.clone(), float(touched) / (n * T), float(resets))
        hip.close()
        return out
    shelf, pipe = "shelf" in obstacle, "pipe" in obstacle
    a, b = run(shelf, pipe), run(shelf, pipe)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])      # deterministic
    st, obs, rew, contact_frac, resets = a
    assert torch.isfinite(st).all() and torch.isfinite(obs).all() and torch.isfinite(rew).all()
    assert float(st[abi.VF_QD0 + 1:abi.VF_QD0 + 6].abs().max()) < 200 and float(obs.abs().max()) <= 5.0
    assert resets > n                                         # episodes end and restart
    if shelf:
        assert contact_frac > 0.01, contact_frac              # the strip is touched
    else:
        assert contact_frac == 0.0                            # no contact report without a shelf (V5:1246-1248)
    if pipe and not shelf:
        free = run(False, False)
        moved = ((st[abi.VF_Q0:abi.VF_Q0 + 6] - free[0][abi.VF_Q0:abi.VF_Q0 + 6]).abs().max(0).values > 1e-3).double().mean()
        assert float(moved) > 0.05, float(moved)              # the tube's walls deflect a good share of the vines


@pytest.mark.parametrize("obs_type", [abi.OBS_POS_ONLY, abi.OBS_POS_AND_VEL, abi.OBS_POS_AND_FD_VEL,
                                      abi.OBS_POS_AND_PREV_POS])
def test_unscaled_observation_types_match_oracle(HipEnv, obs_type):
    """The four observation layouts the reference only runs with SCALE_OBSERVATIONS=False (V5:1354-1368)."""
    n = 1000
    cfg = base_cfg(n, obs_type, True, action_delay=1, seed=77 + obs_type)
    cfg.obs_noise_std, cfg.action_noise_std = 0.01, 0.02
    rng = np.random.default_rng(100 + obs_type)
    hip, orc = pair(HipEnv, cfg, "f32")
    assert hip.num_obs == orc.num_obs == {abi.OBS_POS_ONLY: 14}.get(obs_type, 26)
    seed_both(hip, orc, rng, n, cfg)
    hip.step_count = 3
    orc.step_count = 3
    for _ in range(3):
        actions = rng.uniform(-1.3, 1.3, (n, 2))
        out = hip.step(actions)
        orc.step(actions)
        compare_step(out, orc, hip, 1e-4, 1e-2, 1e-2)
    assert np.abs(out[0]).max() <= cfg.clip_observations
    with pytest.raises(RuntimeError):        # scaling these types is NotImplemented in the reference too
        c2 = base_cfg(8)
        native_check_set_obs_type(c2, obs_type, 1)
    hip.close(); orc.close()


def native_check_set_obs_type(cfg, obs_type, scale):
    from vine_robot_isaacgymenvs_amd import native
    lib = native.load()
    native.check(lib.vine_config_set_obs_type(C.byref(cfg), obs_type, scale), lib)


def test_shelf_contacts_match_oracle(HipEnv):
    """BASELINE config 5: vine_randomize + CREATE_SHELF + ACTION_DELAY=1.  The shelf is placed around each env's
    tip so that board and front-edge contacts are active in a good fraction of envs."""
    n = 768
    cfg = base_cfg(n, 0, True, action_delay=1, seed=77)
    cfg.set_flag(abi.FLAG_CREATE_SHELF, True)
    cfg.set_flag(abi.FLAG_USE_NONZERO_CONTACT_FORCE_RESET, True)
    rng = np.random.default_rng(21)
    for precision, tol in (("f32", (5e-5, 1e-2, 1e-2)), ("f64", (2e-4, 3e-2, 3e-2))):
        hip, orc = pair(HipEnv, cfg, precision)
        st = seed_both(hip, orc, rng, n, cfg)
        st[abi.VF_SHELF_Y] = st[abi.VF_TIP_Y] - 0.2 - 0.05 + rng.uniform(-0.04, 0.04, n)
        st[abi.VF_SHELF_Z] = st[abi.VF_TIP_Z] + rng.uniform(-0.06, 0.06, n)
        st[abi.VF_CONTACT] = rng.uniform(0, 1, n) * (rng.uniform(size=n) < 0.3)
        hip.set_state(st)
        orc.state[:] = st.astype(orc.real)
        actions = rng.uniform(-1, 1, (n, 2))
        out = hip.step(actions)
        orc.step(actions)
        hs, os_ = hip.state, orc.state.astype(np.float64)
        touched = os_[abi.VF_CONTACT_MEAN] > 0
        assert touched.mean() > 0.05
        # a contact that opens/closes within round-off flips discrete decisions: compare envs whose contact state agrees
        same = (hs[abi.VF_CONTACT_MEAN] > 0) == touched
        assert same.mean() > 0.99
        # the masked envs differ in the contact bit only: one side saw a grazing contact (force below 0.05 N on the
        # strip) the other did not, and the state is still the same to contact-free tolerances
        flipped = ~same
        if flipped.any():
            assert np.maximum(hs[abi.VF_CONTACT_MEAN][flipped], os_[abi.VF_CONTACT_MEAN][flipped]).max() < 0.05
            np.testing.assert_allclose(hs[QPOS][:, flipped], os_[QPOS][:, flipped], rtol=0, atol=1e-4)
        np.testing.assert_allclose(hs[QPOS][:, same], os_[QPOS][:, same], rtol=0, atol=tol[0] * 4)
        np.testing.assert_allclose(hs[QVEL][:, same], os_[QVEL][:, same], rtol=0, atol=tol[1] * 4)
        np.testing.assert_allclose(hs[abi.VF_CONTACT_MEAN][same], os_[abi.VF_CONTACT_MEAN][same], rtol=2e-2, atol=2e-2)
        np.testing.assert_allclose(hs[abi.VF_CONTACT][same], os_[abi.VF_CONTACT][same], rtol=2e-2, atol=2e-2)
        np.testing.assert_array_equal(out[2][same], orc.reset_buf[same])
        hip.close(); orc.close()


@pytest.mark.parametrize("with_shelf", [False, True])
def test_pipe_obstacle_matches_oracle(HipEnv, with_shelf):
    """CREATE_PIPE (the reference's default obstacle) as its planar cross-section: reset pose/object_info and wall
    contacts against the oracle; the pipe is placed around each env's tip so that contacts are active."""
    n = 640
    cfg = base_cfg(n, 0, True, action_delay=1, seed=5)
    cfg.set_flag(abi.FLAG_CREATE_PIPE, True)
    cfg.set_flag(abi.FLAG_CREATE_SHELF, with_shelf)
    rng = np.random.default_rng(33)
    hip, orc = pair(HipEnv, cfg, "f32")
    st = seed_both(hip, orc, rng, n, cfg)
    tp = rng.uniform(0.4, 1.1, n)
    th = tp + np.pi / 2
    # pipe origin such that the tip sits ~5 cm inside the entrance, near the first wall
    yl, zl = rng.uniform(-0.01, 0.03, n), rng.uniform(0.0, 0.1, n)
    st[abi.VF_PIPE_Y] = st[abi.VF_TIP_Y] - (yl * np.cos(th) - zl * np.sin(th))
    st[abi.VF_PIPE_Z] = st[abi.VF_TIP_Z] - (yl * np.sin(th) + zl * np.cos(th))
    st[abi.VF_OBJ_ANGLE] = tp
    hip.set_state(st)
    orc.state[:] = st.astype(orc.real)
    a = rng.uniform(-1, 1, (n, 2))
    out = hip.step(a)
    orc.step(a)
    hs, os_ = hip.state, orc.state.astype(np.float64)
    # contacts were active: the free-space oracle from the same state ends elsewhere
    free_cfg = base_cfg(n, 0, True, action_delay=1, seed=5)
    free = vo.OracleEnv(free_cfg, "f32")
    free.state[:abi.VF_PIPE_Y] = st[:abi.VF_PIPE_Y].astype(free.real)
    free.reset_buf[:] = 0
    free.progress[:] = 5
    assert np.isfinite(hs).all()
    np.testing.assert_array_equal(out[2], orc.reset_buf)
    ok = np.abs(hs[QVEL] - os_[QVEL]).max(0) < 0.5      # a contact opening/closing within round-off flips an env
    assert ok.mean() > 0.99
    # the masked envs are flips of one stiff contact, not wrong physics: positions still agree to a millimetre-radian
    np.testing.assert_allclose(hs[QPOS][:, ~ok], os_[QPOS][:, ~ok], rtol=0, atol=5e-3)
    # stiff penalty contacts (k = 2000 N/m on 5 g links) amplify float32 round-off within the 40 substeps
    np.testing.assert_allclose(hs[QPOS][:, ok], os_[QPOS][:, ok], rtol=0, atol=1e-3)
    np.testing.assert_allclose(hs[QVEL][:, ok], os_[QVEL][:, ok], rtol=0, atol=1e-1)
    for f in (abi.VF_PIPE_Y, abi.VF_PIPE_Z, abi.VF_OBJ_ANGLE, abi.VF_OBJ_DEPTH, abi.VF_TARGET_Y, abi.VF_TARGET_Z):
        np.testing.assert_allclose(hs[f], os_[f], rtol=0, atol=2e-5, err_msg="field %d" % f)
    np.testing.assert_allclose(out[0][ok], orc.obs[ok], rtol=0, atol=2e-2)
    hip.close(); orc.close()


@pytest.mark.parametrize("obstacle", ["pipe", "shelf"])
def test_contact_error_is_float32_round_off(HipEnv, obstacle):
    """How wide the contact tolerances above really are: the HIP kernel (float32) and the oracle run in float32 are both
    compared with the oracle run in float64 on the same contact-rich step.  The stiff penalty contacts amplify round-off
    for BOTH float32 runs alike, and the kernel's error distribution must sit inside the float32 oracle's: median and
    99th percentile of |q - q64| and |qd - qd64| at most 2x the float32 oracle's (+ one float32 ulp of the value range;
    measured: 0.8x .. 1.5x -- q 2e-7 median / 1.6e-6 at the 99th percentile, qd 1e-5 / 1.5e-4)."""
    n = 768
    cfg = base_cfg(n, 0, True, action_delay=1, seed=9)
    cfg.set_flag(abi.FLAG_CREATE_PIPE if obstacle == "pipe" else abi.FLAG_CREATE_SHELF, True)
    rng = np.random.default_rng(91)
    hip, o32 = pair(HipEnv, cfg, "f32")
    o64 = vo.OracleEnv(cfg, "f64")
    st = seed_both(hip, o32, rng, n, cfg)
    if obstacle == "pipe":
        tp = rng.uniform(0.4, 1.1, n)
        th = tp + np.pi / 2
        yl, zl = rng.uniform(-0.01, 0.03, n), rng.uniform(0.0, 0.1, n)
        st[abi.VF_PIPE_Y] = st[abi.VF_TIP_Y] - (yl * np.cos(th) - zl * np.sin(th))
        st[abi.VF_PIPE_Z] = st[abi.VF_TIP_Z] - (yl * np.sin(th) + zl * np.cos(th))
        st[abi.VF_OBJ_ANGLE] = tp
    else:
        st[abi.VF_SHELF_Y] = st[abi.VF_TIP_Y] - 0.2 - 0.05 + rng.uniform(-0.04, 0.04, n)
        st[abi.VF_SHELF_Z] = st[abi.VF_TIP_Z] + rng.uniform(-0.06, 0.06, n)
    hip.set_state(st)
    o32.state[:] = st.astype(o32.real)
    o64.state[:] = st.astype(o64.real)
    o64.reset_buf[:] = o32.reset_buf
    o64.progress[:] = o32.progress
    a = rng.uniform(-1, 1, (n, 2))
    hip.step(a)
    o32.step(a)
    o64.step(a)
    hs, s32, s64 = hip.state, o32.state.astype(np.float64), o64.state.astype(np.float64)
    keep = (o32.reset_buf == 0) & (o64.reset_buf == 0)          # (a reset re-draws the state: nothing to compare)
    assert keep.mean() > 0.5
    for name, sl, ulp in (("q", QPOS, 1e-6), ("qd", QVEL, 1e-4)):
        e_hip = np.abs(hs[sl][:, keep] - s64[sl][:, keep]).max(0)
        e_o32 = np.abs(s32[sl][:, keep] - s64[sl][:, keep]).max(0)
        stats = [(np.percentile(e_hip, p), np.percentile(e_o32, p)) for p in (50, 90, 99)]
        print("%s %s: |HIP - f64| / |oracle f32 - f64| at the 50 / 90 / 99th percentile: %s"
              % (obstacle, name, "  ".join("%.2e / %.2e" % t for t in stats)))
        for h_, o_ in (stats[0], stats[2]):
            assert h_ <= 2.0 * o_ + ulp
    hip.close(); o32.close(); o64.close()


def test_first_step_resets_everything(HipEnv):
    """reset_buf starts at ones (vec_task.py:275): the first step simulates the zero pose, then resets all envs."""
    n = 512
    cfg = base_cfg(n)
    hip, orc = pair(HipEnv, cfg, "f32")
    a = np.zeros((n, 2))
    out = hip.step(a)
    orc.step(a)
    compare_step(out, orc, hip, 1e-6, 1e-4, 1e-4)
    assert (hip.progress == 0).all()
    st = hip.state
    assert np.abs(st[abi.VF_Q0 + 1:abi.VF_Q0 + 6]).max() <= np.radians(10) + 1e-6
    assert (st[QVEL] == 0).all()


@pytest.mark.parametrize("introspect", [True, False])
@pytest.mark.parametrize("mode", list(PHYSICS_MODES))
def test_trajectory_tracks_oracle(HipEnv, mode, introspect):
    """40 consecutive steps (1600 substeps) with resets: float32 round-off may grow, flags must stay identical
    for every env whose decision margins are not within round-off.  Every physics mode; with introspection OFF (the
    branch training and bench run: body states re-derived by forward kinematics, dashboard fields not stored) the
    algorithmic outputs and the DOF state are compared, the gated fields are skipped."""
    n, T = 256, 40
    cfg = base_cfg(n, randomize=True, max_episode_length=25)
    PHYSICS_MODES[mode](cfg)
    hip, orc = pair(HipEnv, cfg, "f32")
    hip.set_introspection(introspect)
    rng = np.random.default_rng(5)
    worst_q = 0.0
    mismatched = np.zeros(n, bool)
    for t in range(T):
        a = rng.uniform(-1, 1, (n, 2))
        obs, rew, rst, to = hip.step(a)
        orc.step(a)
        mismatched |= (rst != orc.reset_buf)
        ok = ~mismatched
        worst_q = max(worst_q, np.abs(hip.state[QPOS][:, ok] - orc.state[QPOS][:, ok]).max())
        np.testing.assert_allclose(obs[ok], orc.obs[ok], rtol=0, atol=2e-2)
        np.testing.assert_allclose(rew[ok], orc.rew[ok], rtol=1e-4, atol=5e-3)
        np.testing.assert_array_equal(hip.progress[ok], orc.progress[ok])
    assert mismatched.mean() < 0.02          # threshold decisions flipped by round-off only
    assert worst_q < 5e-3
    hip.close(); orc.close()


@pytest.mark.parametrize("tag,delay,obs_type,held", F6_CASES)
def test_golden_trajectory_from_reference(HipEnv, golden, tag, delay, obs_type, held):
    """F6: the reference's real VecTask.step over 64 steps (fixture), replayed on the GPU.  ``held`` = the literal
    actuation semantics of V5:1043-1062 (efforts incl. C_j*qd_j held over the sim step) at DAMPING 0.08 / with the effort
    clamp, or the obstacle of the case ("shelf", "shelf_contact_reset", "pipe": tests/golden/make_golden.py)."""
    g = golden("f6_traj_" + tag)
    T, N, _ = g["actions"].shape
    cfg = f6_cfg(N, delay, obs_type, held)
    hip = HipEnv(cfg)
    worst = {"q": 0.0, "obs": 0.0, "contact": 0.0}
    for t in range(T):
        hip.bind_reset_values(g["reset_values"][t])
        np.testing.assert_array_equal(hip.reset_buf.astype(bool), g["did_reset"][t])
        obs, rew, rst, to = hip.step(g["actions"][t])
        np.testing.assert_array_equal(rst, g["reset"][t])
        np.testing.assert_array_equal(to.astype(bool), g["timeouts"][t])
        np.testing.assert_array_equal(hip.progress, g["progress"][t])
        st = hip.state
        if "contact_mean" not in g:
            np.testing.assert_allclose(st[QPOS].T, g["q"][t], rtol=0, atol=5e-5)
            np.testing.assert_allclose(obs, g["obs"][t], rtol=1e-3, atol=3e-3)
            np.testing.assert_allclose(rew, g["rew"][t], rtol=1e-4, atol=1e-3)
            continue
        # shelf / pipe (round 4; BASELINE configs[4]'s sequencing): penalty contacts at k = 2000 N/m amplify float32
        # round-off in the positions, hence the wider state tolerances (as in test_shelf_contacts_match_oracle); the
        # contact bookkeeping itself -- mean of the four norms read BEFORE each simulate, the value carried into the
        # next step across the shelf's teleport -- must follow the reference's VecTask.step
        worst["q"] = max(worst["q"], float(np.abs(st[QPOS].T - g["q"][t]).max()))
        worst["obs"] = max(worst["obs"], float(np.abs(obs - g["obs"][t]).max()))
        worst["contact"] = max(worst["contact"], float(np.abs(st[abi.VF_CONTACT_MEAN] - g["contact_mean"][t]).max()))
        # (measured on MI355X, both kernels: |dq| <= 1.5e-5, |dobs| <= 8.3e-4, |dcontact| <= 1.9e-4 N)
        np.testing.assert_allclose(st[QPOS].T, g["q"][t], rtol=0, atol=1e-4)
        np.testing.assert_allclose(obs, g["obs"][t], rtol=1e-3, atol=5e-3)
        np.testing.assert_array_equal(st[abi.VF_CONTACT_MEAN] > 0, g["contact_mean"][t] > 0)
        np.testing.assert_allclose(st[abi.VF_CONTACT_MEAN], g["contact_mean"][t], rtol=1e-3, atol=2e-3)
        if t + 1 < T:
            np.testing.assert_allclose(st[abi.VF_CONTACT], g["contact_norms"][t + 1][0], rtol=1e-3, atol=2e-3)
        # the reward carries -0.1 x contact mean (V5:1529-1530)
        np.testing.assert_allclose(rew, g["rew"][t], rtol=1e-4, atol=1e-3)
    if "contact_mean" in g:
        print("F6 %s through %s: max |dq| %.2e, |dobs| %.2e, |dcontact| %.2e"
              % (tag, hip.lib.vine_step_kernel_name(hip.h).decode(), worst["q"], worst["obs"], worst["contact"]))


def test_dashboard_scalars_match_reference(HipEnv, golden):
    """F7: after replaying the F6 trajectory through the Python task class, ``collect_stats()`` reproduces the ~120
    scalars the reference's compute_reward left in ``wandb_dict`` at the same step (V5:1250-1322), key for key."""
    import torch
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    from vine_robot_isaacgymenvs_amd.utils.config import load_task_config
    g, ref = golden("f6_traj_delay1"), golden("f7_wandb_keys")
    T, N, _ = g["actions"].shape
    ov = ["num_envs=%d" % N, "vine_randomize=False", "task.env.CREATE_PIPE=False", "task.env.ACTION_DELAY=1",
          "task.env.maxEpisodeLength=20", "task.env.SUCCESS_DIST=0.12", "RAIL_SOFT_LIMIT=0.2",
          "task.env.MIN_TARGET_Y=-0.3", "task.env.MAX_TARGET_Y=-0.1", "task.env.MIN_TARGET_Z=0.53",
          "task.env.MAX_TARGET_Z=0.6", "task.env.RANDOM_INIT_CART_MIN_Y=-0.02", "task.env.RANDOM_INIT_CART_MAX_Y=0.2"]
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=load_task_config("Vine5LinkMovingBase", overrides=ov),
                                                  rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                  headless=True)
    assert env.index_to_view == int(ref["index_to_view"])
    env.bind_reward_matrix()
    for t in range(T):
        env.bind_reset_values(g["reset_values"][t])
        obs, rew, rst, _ = env.step(torch.as_tensor(g["actions"][t], device="cuda:0"))
    np.testing.assert_allclose(rew.cpu().numpy(), g["rew"][T - 1], rtol=1e-4, atol=1e-3)
    stats = env.collect_stats()
    bad = []
    for k, v in zip(ref["keys"], ref["values"]):
        got = stats[str(k)]
        if not abs(got - v) <= 3e-3 + 2e-3 * abs(v):
            bad.append((str(k), got, float(v)))
    assert not bad, bad
    env.close()


def test_reset_idx_outside_step(HipEnv):
    n = 300
    cfg = base_cfg(n)
    hip, orc = pair(HipEnv, cfg, "f32")
    ids = np.arange(0, n, 3)
    hip.reset_idx(ids)
    orc.reset_idx(ids)
    np.testing.assert_allclose(hip.state, orc.state, rtol=0, atol=1e-6)
    assert (hip.reset_buf[ids] == 0).all() and (hip.reset_buf[1::3] == 1).all()
    hip.reset_idx(np.zeros(0, np.int64))    # empty id list is a no-op


@pytest.mark.parametrize("how", ["reset_idx", "set_introspection", "bind_reward_matrix"])
def test_lazy_body_states_stay_consistent(HipEnv, how):
    """With introspection off the four-lanes-per-env kernel does not store the tip / cart rigid-body states every step
    (they are re-derived from the DOF state).  Whoever CONSUMES the memory copies must still see current values:
    reset_idx from outside the step (the stale-body rule P5 keeps the pre-reset tip as prev_tip: it must be the tip of the
    LAST step, not of the env's last in-step reset) and switching introspection on mid-run (directly or through
    vine_bind_reward_matrix).  Twin run with introspection always on; after the event the two must agree."""
    n = 512
    cfg = base_cfg(n, 0, True, action_delay=1, seed=21, max_episode_length=40)
    rng = np.random.default_rng(9)
    a, b = HipEnv(cfg), HipEnv(cfg)
    b.set_introspection(False)
    for t in range(7):
        acts = rng.uniform(-1, 1, (n, 2))
        a.step(acts); b.step(acts)
    ids = np.arange(1, n, 3)
    if how == "reset_idx":
        a.reset_idx(ids); b.reset_idx(ids)
    elif how == "set_introspection":
        b.set_introspection(True)
    else:
        a.bind_reward_matrix(); b.bind_reward_matrix()
    for t in range(2):
        acts = rng.uniform(-1, 1, (n, 2))
        oa, ob = a.step(acts), b.step(acts)
        np.testing.assert_allclose(oa[0], ob[0], rtol=0, atol=2e-4)       # fd_tip columns are (tip - prev_tip) * 30
        np.testing.assert_allclose(oa[1], ob[1], rtol=1e-5, atol=1e-4)
        np.testing.assert_array_equal(oa[2], ob[2])
    sa, sb = a.state, b.state
    np.testing.assert_allclose(sa[QPOS], sb[QPOS], rtol=0, atol=2e-6)
    np.testing.assert_allclose(sa[QVEL], sb[QVEL], rtol=0, atol=2e-4)
    if how != "reset_idx":
        for f in (abi.VF_TIP_Y, abi.VF_TIP_Z, abi.VF_CART_Y, abi.VF_CART_VY, abi.VF_PREV_TIP_Y, abi.VF_PREV_TIP_Z):
            np.testing.assert_allclose(sa[f], sb[f], rtol=0, atol=2e-5, err_msg="field %d" % f)
    a.close(); b.close()


def test_reset_idx_after_steps_matches_oracle(HipEnv):
    """reset_idx from outside the step AFTER several steps (the production branch: introspection off), against the
    oracle: the next step's observation carries the stale tip of the last step (P5), not an older one."""
    n = 300
    cfg = base_cfg(n, 0, False, action_delay=1, seed=4, max_episode_length=60)
    hip, orc = pair(HipEnv, cfg, "f32")
    hip.set_introspection(False)
    rng = np.random.default_rng(12)
    for t in range(6):
        acts = rng.uniform(-1, 1, (n, 2))
        hip.step(acts); orc.step(acts)
    ids = np.arange(0, n, 2)
    hip.reset_idx(ids); orc.reset_idx(ids)
    bad = np.zeros(n, bool)
    for t in range(2):
        acts = rng.uniform(-1, 1, (n, 2))
        obs, rew, rst, to = hip.step(acts)
        orc.step(acts)
        bad |= rst != orc.reset_buf
        np.testing.assert_allclose(obs[~bad], orc.obs[~bad], rtol=0, atol=5e-3)
        np.testing.assert_array_equal(hip.progress, orc.progress)
    assert bad.mean() < 0.01
    hip.close(); orc.close()


def test_full_size_properties(HipEnv):
    """BASELINE config 3 size (16384 envs): determinism, bounds, episode bookkeeping over 600 steps."""
    import torch
    n, T = 16384, 600
    cfg = base_cfg(n, randomize=True)
    runs = []
    for rep in range(2):
        hip = HipEnv(cfg)
        g = torch.Generator(device=hip.dev).manual_seed(0)
        n_done = torch.zeros((), device=hip.dev)
        n_to = torch.zeros((), device=hip.dev)
        max_prog = 0
        for t in range(T):
            a = torch.rand((n, 2), device=hip.dev, generator=g) * 2 - 1
            hip.step_t(a, sync=False)
            n_done += hip.reset_t.sum()
            n_to += hip.timeouts_t.sum()
            assert bool(((hip.timeouts_t == 0) | (hip.reset_t != 0)).all()) if t % 100 == 0 else True
        torch.cuda.synchronize()
        st = hip.state_t.clone()
        assert torch.isfinite(st).all()
        assert float(hip.obs_t.abs().max()) <= 5.0
        assert int(hip.progress_t.max()) <= cfg.max_episode_length - 1
        assert float(st[abi.VF_QD0 + 1:abi.VF_QD0 + 6].abs().max()) < 50
        assert float(n_done) > 0 and float(n_to) > 0
        runs.append((st, hip.obs_t.clone(), hip.rew_t.clone(), float(n_done)))
        assert hip.step_count == T
        hip.close()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][3] == runs[1][3]


def test_baseline_config2_free_space_reaching(HipEnv):
    """BASELINE.json configs[1]: 4096 envs, README.md:63 free-space overrides (TIP_AND_CART_AND_OBJ_INFO obs,
    maxEpisodeLength 100, SUCCESS_DIST 0.04, targets y in +-0.4, z in [0.55, 0.7], soft limit 0.25, P gain 30,
    acceleration 6), fp32: 30 steps from reset against the float32 oracle."""
    n = 4096
    cfg = base_cfg(n, 1, False, action_delay=1, max_episode_length=100, success_dist=0.04, min_target_y=-0.4,
                   max_target_y=0.4, min_target_z=0.55, max_target_z=0.7, rail_soft_limit=0.25, rail_p_gain=30.0,
                   rail_acceleration=6.0, random_init_cart_min_y=-0.025, random_init_cart_max_y=0.25)
    hip, orc = pair(HipEnv, cfg, "f32")
    rng = np.random.default_rng(8)
    bad = np.zeros(n, bool)
    for t in range(30):
        a = rng.uniform(-1, 1, (n, 2))
        obs, rew, rst, to = hip.step(a)
        orc.step(a)
        bad |= rst != orc.reset_buf
        ok = ~bad
        np.testing.assert_allclose(obs[ok], orc.obs[ok], rtol=0, atol=5e-3)
        np.testing.assert_allclose(rew[ok], orc.rew[ok], rtol=1e-4, atol=2e-3)
    assert bad.mean() < 0.01 and obs.shape == (n, 18)
    assert orc.reset_buf.sum() > 0          # targets get reached / limits hit within 30 steps


@pytest.mark.parametrize("n", [100, 3000, 4097])
def test_step_counter_on_padded_grids(HipEnv, n):
    """The step count is base + (finished workgroups >> log2 grid) and step launches have power-of-two grids: env counts
    whose natural grid is NOT a power of two (the padding workgroups find no live env and only report their arrival) must
    count one per step, survive set / get, and key the random streams exactly as the oracle's explicit counter does."""
    cfg = base_cfg(n, 0, True)
    hip, orc = HipEnv(cfg), vo.OracleEnv(cfg, "f32")
    rng = np.random.default_rng(9)
    for k in range(1, 6):
        a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        obs, rew, rst, _ = hip.step(a)
        orc.step(a)
        assert hip.step_count == k == orc.step_count
        np.testing.assert_allclose(obs, orc.obs, rtol=0, atol=2e-4)
    hip.step_count = orc.step_count = 1000
    assert hip.step_count == 1000
    a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    obs, rew, rst, _ = hip.step(a)
    orc.step(a)
    assert hip.step_count == 1001
    np.testing.assert_allclose(obs, orc.obs, rtol=0, atol=2e-4)      # (observation noise keyed by step 1000: the same draws)
    np.testing.assert_array_equal(rst, orc.reset_buf)


def test_largest_single_gpu_configuration(HipEnv):
    """BASELINE.json configs[3] puts 131072 envs on 8 GPUs; one GPU takes all of them too (state 31 MB).
    Determinism, bounds and the step counter at that size; first and last env against the oracle."""
    import torch
    n = 131072
    cfg = base_cfg(n, 0, True)
    hip = HipEnv(cfg)
    g = torch.Generator(device=hip.dev).manual_seed(3)
    acts = [torch.rand((n, 2), device=hip.dev, generator=g) * 2 - 1 for _ in range(8)]
    for a in acts:
        hip.step_t(a, sync=False)
    torch.cuda.synchronize()
    assert torch.isfinite(hip.state_t).all() and float(hip.obs_t.abs().max()) <= 5.0 and hip.step_count == 8
    # envs 0..63 and n-64..n-1 replayed on the oracle with the same (seed, global env id, step) keys
    for lo in (0, n - 64):
        sub = base_cfg(64, 0, True)
        sub.env_id_offset = lo
        orc = vo.OracleEnv(sub, "f32")
        for a in acts:
            orc.step(a[lo:lo + 64].cpu().numpy())
        np.testing.assert_allclose(hip.obs_t[lo:lo + 64].cpu().numpy(), orc.obs, rtol=0, atol=5e-3)
        np.testing.assert_array_equal(hip.reset_t[lo:lo + 64].cpu().numpy(), orc.reset_buf)
        # the reset draws of the block (targets: an affine map of pure RNG outputs) agree with the shard's to 1 ulp
        # (the kernel contracts min + span * u into one fma)
        np.testing.assert_allclose(hip.state_t[abi.VF_TARGET_Y, lo:lo + 64].cpu().numpy(),
                                   orc.state[abi.VF_TARGET_Y].astype(np.float32), rtol=0, atol=1e-7)
    hip.close()


def test_env_id_offset_shards_reproduce_the_batch(HipEnv):
    """VineConfig.env_id_offset: a shard [lo, lo + m) of a batch, created with offset lo, draws (resets, noise,
    dynamics scaling) exactly what those envs draw inside the whole batch -- what a strong-scaling rank needs."""
    n, lo, m = 1024, 384, 256
    cfg = base_cfg(n, 0, True, seed=9)
    cfg.obs_noise_std, cfg.action_noise_std = 0.01, 0.02
    cfg.dyn_scale_min, cfg.dyn_scale_max = 0.9, 1.1
    sub = base_cfg(m, 0, True, seed=9)
    sub.obs_noise_std, sub.action_noise_std = 0.01, 0.02
    sub.dyn_scale_min, sub.dyn_scale_max = 0.9, 1.1
    sub.env_id_offset = lo
    whole, shard = HipEnv(cfg), HipEnv(sub)
    rng = np.random.default_rng(2)
    for t in range(12):
        a = rng.uniform(-1, 1, (n, 2))
        o1, r1, d1, _ = whole.step(a)
        o2, r2, d2, _ = shard.step(a[lo:lo + m])
        np.testing.assert_array_equal(o1[lo:lo + m], o2)
        np.testing.assert_array_equal(r1[lo:lo + m], r2)
        np.testing.assert_array_equal(d1[lo:lo + m], d2)
    np.testing.assert_array_equal(whole.state_t[:, lo:lo + m].cpu().numpy(), shard.state_t.cpu().numpy())
    whole.close(); shard.close()


def test_envs_are_independent_of_batch_position(HipEnv):
    """Sharding property used by the multi-GPU path: env i of a big batch == the same env stepped alone,
    given the same state, action and (seed, env id, step) RNG key."""
    n = 256
    cfg = base_cfg(n, randomize=False)
    rng = np.random.default_rng(3)
    hip = HipEnv(cfg)
    st = random_state(rng, n, cfg)
    hip.set_state(st)
    hip.set_flags(np.zeros(n, np.int64), np.full(n, 5))
    a = rng.uniform(-1, 1, (n, 2))
    obs, rew, rst, to = hip.step(a)
    sub = slice(64, 128)
    cfg2 = base_cfg(64, randomize=False)
    hip2 = HipEnv(cfg2)
    hip2.set_state(st[:, sub])
    hip2.set_flags(np.zeros(64, np.int64), np.full(64, 5))
    obs2, rew2, rst2, to2 = hip2.step(a[sub])
    np.testing.assert_array_equal(obs[sub], obs2)
    np.testing.assert_array_equal(rew[sub], rew2)
    np.testing.assert_array_equal(rst[sub], rst2)


def test_task_class_step_contract(HipEnv, golden):
    """The Python drop-in: shapes, dtypes, devices and first-step semantics of VecTask.step/reset."""
    import torch
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    from vine_robot_isaacgymenvs_amd.utils.config import load_task_config
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=128", "task.env.CREATE_PIPE=False"])
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg, rl_device="cuda:0", sim_device="cuda:0",
                                                  graphics_device_id=0, headless=True, virtual_screen_capture=False,
                                                  force_render=False)
    assert env.num_envs == 128 and env.num_obs == 28 and env.num_acts == 2 and env.num_states == 0
    assert env.observation_space.shape == (28,) and env.action_space.shape == (2,)
    first = env.reset()
    assert first["obs"].shape == (128, 28) and float(first["obs"].abs().max()) == 0.0
    obs, rew, done, info = env.step(env.zero_actions())
    assert obs["obs"].shape == (128, 28) and obs["obs"].dtype == torch.float32
    assert rew.shape == (128,) and done.dtype == torch.long and info["time_outs"].dtype == torch.bool
    assert int(env.progress_buf.max()) == 0                      # everything was reset inside the first step
    assert env.dof_pos.shape == (128, 6) and env.tip_positions.shape == (128, 3)
    for _ in range(5):
        obs, rew, done, info = env.step(torch.rand(128, 2, device="cuda:0") * 2 - 1)
    assert int(env.progress_buf.max()) == 5
    assert float(obs["obs"].abs().max()) <= 5.0
    # metrics side channel: same keys as the reference's wandb_dict (V5:1250-1322)
    env.bind_reward_matrix()
    env.step(torch.rand(128, 2, device="cuda:0") * 2 - 1)
    stats = env.collect_stats()
    for key in ("dist_tip_to_target", "target_reached", "limit_hit", "tip_velocities_max", "Aggregated Reward",
                "prismatic_q0 at self.index_to_view", "finite_diff_qd4 at self.index_to_view",
                "tip_pos_z at self.index_to_view", "Mean Position Success Reward", "Weighted Max Contact Force Reward",
                "Mean Total Reward", "progress_buf"):
        assert key in stats and np.isfinite(stats[key]), key
    # exactly the key set the reference's compute_reward leaves in wandb_dict (golden F7, from the reference's Python)
    ref_keys = set(str(k) for k in golden("f7_wandb_keys")["keys"])
    assert set(stats) == ref_keys, (sorted(ref_keys - set(stats)), sorted(set(stats) - ref_keys))
    assert len(stats) >= 118
    assert abs(stats["Mean Const Negative Reward"] + 1.0) < 1e-6 and 0.0 < stats["progress_buf"] <= 6.0
    env.close()


def test_mat_file_replay(HipEnv, tmp_path):
    """MAT_FILE (V5:281-297, 947-982): before every step all envs are put on sample num_steps % T of the recording
    (joint positions, zero velocities, target, tip state).  Checked against a second env whose state is set by hand."""
    import scipy.io
    import torch
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    from vine_robot_isaacgymenvs_amd.utils.config import load_task_config
    rng = np.random.default_rng(5)
    T = 7
    mat = {"cart_pos": rng.uniform(-0.1, 0.1, (1, T)), "Q": rng.uniform(-0.2, 0.2, (5, T)),
           "moving_target_pos": np.stack([np.zeros(T), rng.uniform(-0.3, -0.1, T), rng.uniform(0.5, 0.6, T)]),
           "target_vel": np.zeros((3, 1)), "tip_pos": np.stack([np.zeros(T), rng.uniform(-0.2, 0.2, T), rng.uniform(0.5, 0.6, T)]),
           "tip_vel": rng.uniform(-0.1, 0.1, (3, T))}
    path = str(tmp_path / "replay.mat")
    scipy.io.savemat(path, mat)
    common = ["num_envs=64", "task.env.CREATE_PIPE=False", "vine_randomize=False"]

    def make(extra):
        cfg = load_task_config("Vine5LinkMovingBase", overrides=common + extra)
        return isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg, rl_device="cuda:0", sim_device="cuda:0",
                                                        graphics_device_id=0, headless=True,
                                                        virtual_screen_capture=False, force_render=False)
    a, b = make(["task.env.MAT_FILE=" + path]), make([])
    assert a.graph_capturable is False and b.graph_capturable is True
    # a host that writes tip / cart rigid-body states by hand must have introspection on: without it the four-lanes-per-env
    # kernel re-derives them from the DOF state (the MAT_FILE task arms it itself)
    assert a._introspection is True
    b.set_introspection(True)
    acts = torch.rand(64, 2, device="cuda:0") * 2 - 1
    for step in range(T + 2):                                  # wraps around the recording
        i = step % T
        st = b.state
        st[abi.VF_Q0] = float(mat["cart_pos"][0, i])
        for j in range(5):
            st[abi.VF_Q0 + 1 + j] = float(mat["Q"][j, i])
        st[abi.VF_QD0:abi.VF_QD0 + 6] = 0.0
        st[abi.VF_TARGET_Y], st[abi.VF_TARGET_Z] = float(mat["moving_target_pos"][1, i]), float(mat["moving_target_pos"][2, i])
        st[abi.VF_TIP_Y], st[abi.VF_TIP_Z] = float(mat["tip_pos"][1, i]), float(mat["tip_pos"][2, i])
        st[abi.VF_TIP_VY], st[abi.VF_TIP_VZ] = float(mat["tip_vel"][1, i]), float(mat["tip_vel"][2, i])
        oa, ra, da, _ = a.step(acts)
        ob, rb, db, _ = b.step(acts)
        if step > 0:      # step 0 resets every env (reset_buf starts at ones) with each env's own draws
            torch.testing.assert_close(ra, rb, rtol=0, atol=0)
        assert torch.equal(da, db)
    mat["target_vel"] = np.ones((3, 1))
    scipy.io.savemat(path, mat)
    with pytest.raises(NotImplementedError):
        make(["task.env.MAT_FILE=" + path])
    a.close(); b.close()


def test_ppo_iteration_on_gpu_eager_and_graphed(HipEnv):
    """The PPO agent on the real task class: one iteration with an eager rollout and one with the rollout
    replayed from a hipGraph start from the same state and must produce the same experience."""
    import torch
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map

    results = []
    for use_graphs in (False, True):
        cfg = load_config(overrides=["num_envs=256", "minibatch_size=1024"])
        cfg["task"]["seed"] = 42
        env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0",
                                                      graphics_device_id=0, headless=True)
        params = cfg["train"]["params"]
        params["config"].update(write_files=False, print_stats=False, use_graphs=use_graphs, mixed_precision=False)
        torch.manual_seed(0)
        agent = A2CAgent("t", params, vec_env=env)
        agent.init_tensors()
        agent.obs = agent.env_reset()["obs"]
        torch.manual_seed(123)
        for it in range(2):
            play, upd, stats = agent.train_epoch()
        torch.cuda.synchronize()
        assert all(torch.isfinite(p).all() for p in agent.model.parameters())
        assert torch.isfinite(agent.buf["obses"]).all() and float(agent.buf["obses"].abs().max()) <= 5.0
        assert int(env.progress_buf.max()) > 0
        results.append((agent.buf["obses"].clone(), agent.buf["rewards"].clone(), env.step_count,
                        {k: float(v) for k, v in stats.items()}))
        env.close()
    assert results[0][2] == results[1][2] == 32
    # the same RNG stream is not guaranteed between eager and captured torch.randn: compare statistics
    for k in ("a_loss", "c_loss", "kl"):
        assert np.isfinite(results[0][3][k]) and np.isfinite(results[1][3][k])
    assert abs(float(results[0][0].mean()) - float(results[1][0].mean())) < 0.05


def test_train_entry_checkpoint_and_play(HipEnv, tmp_path, monkeypatch):
    """train.py semantics end to end (train.py:35-171): compose config from CLI overrides, train a few iterations,
    write runs/<name>/config.yaml + the config pickle + checkpoints, then `test=True checkpoint=...` plays it."""
    import glob
    import os
    import pickle
    from vine_robot_isaacgymenvs_amd.train import main
    monkeypatch.chdir(tmp_path)
    ov = ["task=Vine5LinkMovingBase", "num_envs=256", "minibatch_size=1024", "max_iterations=3", "headless=True",
          "experiment=unit", "train.params.config.save_frequency=1", "train.params.config.save_best_after=0",
          "train.params.config.env_stats_every=1", "task.env.CREATE_HISTOGRAMS_PERIODICALLY=True",
          "train.params.config.horizon_length=64"]
    last_mean, epoch = main(ov)
    assert epoch == 3
    run = tmp_path / "runs" / "unit"
    assert (run / "config.yaml").exists() and glob.glob(str(run / "*_rlg_config_dict.pkl"))
    cfgd = pickle.load(open(glob.glob(str(run / "*_rlg_config_dict.pkl"))[0], "rb"))
    assert cfgd["params"]["config"]["name"] == "unit" and cfgd["params"]["network"]["rnn"]["units"] == 256
    ckpts = glob.glob(str(run / "nn" / "*.pth"))
    assert ckpts, "no checkpoint written"
    scal = (run / "summaries" / "scalars.csv").read_text()
    for tag in ("performance/step_inference_rl_update_fps", "losses/a_loss", "info/kl", "info/last_lr",
                # the task's dashboard keys (V5:1250-1322) through the observer
                "env/dist_tip_to_target", "env/Aggregated Reward", "env/Weighted Mean Position Success Reward",
                "env/tip_pos_z at self.index_to_view"):
        assert tag in scal, tag
    hists = glob.glob(str(run / "summaries" / "histograms" / "observation_histograms_*.npz"))
    assert hists, "CREATE_HISTOGRAMS_PERIODICALLY wrote nothing"
    h = np.load(hists[0])
    assert h["rows"].shape == (100, 28) and h["joint_pos_0_counts"].sum() == 100 and "target_angle_edges" in h
    # resume + play
    ck = sorted(ckpts)[-1]
    main(ov[:-5] + ["checkpoint=" + ck, "max_iterations=4", "train.params.config.horizon_length=64"])
    reward, steps = main(["task=Vine5LinkMovingBase", "num_envs=256", "test=True", "checkpoint=" + ck, "headless=True",
                          "+train.params.config.player={max_steps: 40}"])
    assert np.isfinite(reward) and steps > 0
