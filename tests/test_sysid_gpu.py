"""SYSID on the GPU (include/vine_sysid.h, utils/sysid.py): the pin against a numpy restatement and against the rings the
step kernel itself leaves; exact recovery of the plant that made a log; the error sum against float64 numpy; a candidate
that leaves the log's episode; the captured graph against the eager path; ``fit`` end to end.

The shapes: 70 envs = two waves, the second partial; windows of H = 12 steps; logs of 40 rows (the recovery log: the
hand-made row 0 and the 40 rows its 40 steps left).  "Bit-identical" is literal: floats are compared as words.

Why the recovery can be exact from windows that start mid-run (rows 12 and 24).  A log row does not hold the rail
controller's two memories: VF_PREV_CART_VEL_ERR enters the force only through RAIL_D_GAIN, which is
0 in the task YAML and in this test; VF_PREV_CART_VEL enters only the bang-bang branch, |u_rail - cart velocity| > 0.1 m/s.
The action table keeps the rail command within 0.01 .. 0.03 m/s and row 0 gives the cart 0.02 m/s, so the controller stays
in its proportional branch and nothing a row lacks is read.  Everything else the step reads is in the row or rebuilt by
the pin from the log's last ACTION_DELAY actions."""
import json

import numpy as np
import pytest
import torch

from tests.helpers import base_cfg
from tests.test_trajectory_gpu import POS_ULPS, VEL_ULPS, _fk64, _ulp32
from vine_robot_isaacgymenvs_amd import abi, load_task_config, native
from vine_robot_isaacgymenvs_amd.utils import env_params, sysid
from vine_robot_isaacgymenvs_amd.utils.trajectory import record_config, write_trajectory_mat

pytestmark = pytest.mark.gpu

N, H, T = 70, 12, 40
SENTINEL = -7777.0
STARTS = [0, 12, 24]
TRUTH = {"DAMPING": 0.035, "ACTION_DELAY": 2, "FPAM_K": 1.1}
TRUE_ENV, DELAY_ENV, ULP_ENV, RUNAWAY_ENV = 17, 18, 19, 40
F = abi


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ------------------------------------------------------------------------------------------------------------ 1: the pin
def _made_up_log(seed=5):
    rng = np.random.default_rng(seed)
    log = np.zeros((T, abi.RECORD_FIELDS), dtype=np.float32)
    log[:, F.VRF_Q0] = rng.uniform(-0.25, 0.25, T)
    log[:, F.VRF_Q0 + 1:F.VRF_Q0 + 6] = rng.uniform(-0.4, 0.4, (T, 5))
    log[:, F.VRF_QD0] = rng.uniform(-1, 1, T)
    log[:, F.VRF_QD0 + 1:F.VRF_QD0 + 6] = rng.uniform(-3, 3, (T, 5))
    log[:, F.VRF_TIP_Y:F.VRF_TIP_VZ + 1] = 99.0                     # not what the pin may copy
    log[:, F.VRF_TARGET_Y] = rng.uniform(-0.48, -0.4, T)
    log[:, F.VRF_TARGET_Z] = rng.uniform(0.58, 0.67, T)
    log[:, F.VRF_ACTION0:F.VRF_ACTION0 + 2] = rng.uniform(-1.3, 1.3, (T, 2))      # beyond clipActions = 1 too
    log[:, F.VRF_SMOOTHED_U] = rng.uniform(-0.1, 3.0, T)
    log[:, F.VRF_PROGRESS] = np.arange(T)
    return log


def _lane_cfg(**flags):
    cfg = base_cfg(N, 0, False, max_episode_length=100, action_delay=1)
    for f in (abi.FLAG_USE_TARGET_REACHED_RESET, abi.FLAG_USE_TIP_LIMIT_HIT_RESET, abi.FLAG_USE_NONZERO_CONTACT_FORCE_RESET,
              abi.FLAG_CREATE_SHELF, abi.FLAG_CREATE_PIPE):
        cfg.set_flag(f, False)
    for f, on in flags.items():
        cfg.set_flag(getattr(abi, f), on)
    return cfg


def _lane(cfg, table=None):
    from tests.hip_env import HipEnv
    env = type("HipEnvLane", (HipEnv,), {"kernel": "lane"})(cfg)
    if table is not None:
        env_params.check_table(env.lib, env.cfg, table)
        env.table_t = torch.as_tensor(np.ascontiguousarray(table, np.float32)).to(env.dev).contiguous()
        torch.cuda.synchronize(env.dev)
        native.check(env.lib.vine_bind_env_params(env.h, env.table_t.data_ptr()), env.lib)
    return env


class _PinBuffers:
    def __init__(self, env):
        d = env.dev
        self.actions = torch.full((env.n, 2), SENTINEL, device=d)
        self.rew = torch.full((env.n,), SENTINEL, device=d)
        self.reset = torch.ones(env.n, dtype=torch.long, device=d)
        self.progress = torch.full((env.n,), 7, dtype=torch.long, device=d)
        self.window = torch.full((2,), -99, dtype=torch.long, device=d)

    def pin(self, env, scfg, log_t, row):
        return env.lib.vine_sysid_pin(env.h, scfg, log_t.data_ptr(), int(row), self.actions.data_ptr(), self.rew.data_ptr(),
                                      self.reset.data_ptr(), self.progress.data_ptr(), self.window.data_ptr(), _stream(env.dev))


@pytest.mark.parametrize("row", [9, 3])
def test_pin_writes_the_listed_fields_and_nothing_else(row):
    """Delays 0..8 inside one wave and a RAIL_VELOCITY_SCALE of its own per env; the step counter at 5; the state block full
    of a sentinel.  Row 9 has eight rows before it (every delay finds its actions in the log); row 3 has three, so delays
    above 4 also need the command (0, 0) of rows before row 0.

    Copies are exact.  The tip fields against the float64 kinematics of the row's q, qd within the recorder test's budget
    (tests/test_trajectory_gpu.py: POS_ULPS / VEL_ULPS ulps of the largest magnitude in the sums).  The ring against what
    the step kernel itself leaves: a reference handle with the same table steps through the actions of the rows up to
    `row`, ending at step count 16, so its slot (16 - k) mod d holds the command of row + 1 - k's action; the pinned
    handle, at count 5, must hold the same words in slot (5 - k) mod d, and slots d .. 7 keep the sentinel."""
    lib = native.load()
    cfg = _lane_cfg()
    table = np.repeat(env_params.config_row(lib, cfg)[:, None], N, axis=1)
    delays = np.arange(N) % 9
    table[abi.VP_ACTION_DELAY] = delays
    table[abi.VP_RAIL_VELOCITY_SCALE] = 0.7 + 0.01 * np.arange(N)
    log = _made_up_log()
    env, ref = _lane(cfg, table), _lane(cfg, table)
    try:
        log_t = torch.as_tensor(log, device=env.dev)
        scfg = sysid.sysid_config(lib, T, H)
        # the reference rings
        first = max(0, row - 7)
        ref.step_count = 16 - (row + 1 - first)
        for r in range(first, row + 1):
            ref.step_t(log_t[r, F.VRF_ACTION0:F.VRF_ACTION0 + 2].expand(N, 2).contiguous(), sync=False)
        torch.cuda.synchronize()
        assert ref.step_count == 16
        ref_ring = ref.state_t[F.VF_FIFO0:F.VF_FIFO0 + 16].cpu().numpy()
        # the pin
        env.state_t.fill_(SENTINEL)
        env.step_count = 5
        b = _PinBuffers(env)
        assert b.pin(env, scfg, log_t, row) == abi.OK, lib.vine_last_error()
        torch.cuda.synchronize()
        assert env.step_count == 5
        st = env.state_t.cpu().numpy()
        L = log[row]
        touched = set()

        def field(f, want, count=1):
            for i in range(count):
                w = want[i] if count > 1 else want
                assert np.array_equal(st[f + i].view(np.uint32), np.full(N, w, np.float32).view(np.uint32)), (f, i)
                touched.add(f + i)

        field(F.VF_Q0, L[F.VRF_Q0:F.VRF_Q0 + 6], 6)
        field(F.VF_QD0, L[F.VRF_QD0:F.VRF_QD0 + 6], 6)
        field(F.VF_PREV_Q0, L[F.VRF_Q0:F.VRF_Q0 + 6], 6)
        field(F.VF_CART_Y, L[F.VRF_Q0]); field(F.VF_CART_VY, L[F.VRF_QD0])
        field(F.VF_SMOOTHED_U, L[F.VRF_SMOOTHED_U])
        field(F.VF_PREV_CART_VEL, L[F.VRF_QD0])
        field(F.VF_PREV_CART_VEL_ERR, 0.0); field(F.VF_PREV_U_RAIL, 0.0); field(F.VF_AGG_REW, 0.0)
        field(F.VF_TARGET_Y, L[F.VRF_TARGET_Y]); field(F.VF_TARGET_Z, L[F.VRF_TARGET_Z])
        # the tip: float64 kinematics of the row's joint state, the recorder test's budget
        q64, qd64 = L[None, 0:6].astype(np.float64), L[None, 6:12].astype(np.float64)
        want, m_pos, m_vel = _fk64(q64, qd64, float(cfg.link_length), float(cfg.joint1_z), float(cfg.phi0))
        tol = [POS_ULPS * _ulp32(m_pos)[0]] * 2 + [VEL_ULPS * _ulp32(m_vel)[0]] * 2
        for i, f in enumerate((F.VF_TIP_Y, F.VF_TIP_Z, F.VF_TIP_VY, F.VF_TIP_VZ)):
            assert (st[f] == st[f][0]).all() and abs(float(st[f][0]) - want[0, i]) <= tol[i], (f, st[f][0], want[0, i], tol[i])
            touched.add(f)
        assert np.array_equal(st[F.VF_PREV_TIP_Y], st[F.VF_TIP_Y]) and np.array_equal(st[F.VF_PREV_TIP_Z], st[F.VF_TIP_Z])
        touched |= {F.VF_PREV_TIP_Y, F.VF_PREV_TIP_Z}
        # the ring
        ring = st[F.VF_FIFO0:F.VF_FIFO0 + 16]
        commands = 0
        for e in range(N):
            d = int(delays[e])
            for s in range(d, abi.MAX_DELAY):
                assert ring[2 * s, e] == SENTINEL and ring[2 * s + 1, e] == SENTINEL, (e, s)
            for k in range(1, d + 1):
                s_pin, s_ref = (5 - k) % d, (16 - k) % d
                got = ring[2 * s_pin:2 * s_pin + 2, e]
                exp = ref_ring[2 * s_ref:2 * s_ref + 2, e] if row + 1 - k >= 0 else np.zeros(2, np.float32)
                assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (e, k, got, exp)
                commands += int(row + 1 - k >= 0)
        touched |= set(range(F.VF_FIFO0, F.VF_FIFO0 + 16))
        # (the reference rings are not trivially equal: the command depends on the env's own rail scale)
        assert commands >= 150 and len(np.unique(ref_ring[0])) > 30
        # a numpy restatement of the command for one slot, to a float32 ulp (the device may contract a*b + c)
        e, a = N - 1, log[row, F.VRF_ACTION0:F.VRF_ACTION0 + 2]
        d = int(delays[e])
        rail = np.clip(a[0], -cfg.clip_actions, cfg.clip_actions) * table[abi.VP_RAIL_VELOCITY_SCALE, e]
        fpam = (np.clip(a[1], -cfg.clip_actions, cfg.clip_actions) + 1.0) * 0.5 * (cfg.fpam_max - cfg.fpam_min) + cfg.fpam_min
        got = ring[2 * ((5 - 1) % d):2 * ((5 - 1) % d) + 2, e]
        assert abs(got[0] - rail) <= np.spacing(np.float32(abs(rail))) and abs(got[1] - fpam) <= 4 * np.spacing(np.float32(3.1))
        # everything not in the list keeps the sentinel
        for f in range(abi.VF_COUNT):
            if f not in touched:
                assert (st[f] == SENTINEL).all(), f
        assert len(touched) == abi.VF_COUNT - 11
        # the step's buffers, the next action, the window words
        assert np.array_equal(b.actions.cpu().numpy(), np.repeat(log[row + 1:row + 2, F.VRF_ACTION0:F.VRF_ACTION0 + 2], N, 0))
        assert not b.rew.any() and not b.reset.any() and not b.progress.any()
        assert b.window.tolist() == [5, row]
    finally:
        env.close()
        ref.close()


def test_pin_refusals():
    lib = native.load()
    log = _made_up_log()
    scfg = sysid.sysid_config(lib, T, H)
    for flags, word in ((dict(FLAG_CREATE_SHELF=True), b"CREATE_SHELF"), (dict(FLAG_CREATE_PIPE=True), b"CREATE_PIPE"),
                        (dict(FLAG_VINE_RANDOMIZE=True), b"vine_randomize")):
        env = _lane(_lane_cfg(**flags))
        try:
            before = env.state_t.clone()
            rc = _PinBuffers(env).pin(env, scfg, torch.as_tensor(log, device=env.dev), 9)
            assert rc == abi.ERR_UNSUPPORTED and word in lib.vine_last_error(), (flags, lib.vine_last_error())
            torch.cuda.synchronize()
            assert torch.equal(env.state_t, before)
        finally:
            env.close()
    env = _lane(_lane_cfg())
    try:
        log_t, b = torch.as_tensor(log, device=env.dev), _PinBuffers(env)
        for row, word in ((-1, b"row outside"), (T, b"row outside"), (T - H, b"horizon outside"), (T - 1, b"horizon outside")):
            assert b.pin(env, scfg, log_t, row) == abi.ERR_INVALID_ARG and word in lib.vine_last_error(), row
        assert b.pin(env, scfg, log_t, T - H - 1) == abi.OK         # the last row a window fits behind; no table: the config's delay
        torch.cuda.synchronize()
        assert b.window.tolist() == [0, T - H - 1]
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------- 2-6: one recorded log
def _task_cfg(n):
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % n])
    cfg["seed"] = 42
    assert cfg["env"]["RAIL_D_GAIN"] == 0.0          # (see the module's docstring)
    return cfg


def _hand_made_log():
    """41 rows: row 0 is a pose, rows 1..40 carry only the action table."""
    log = np.zeros((T + 1, abi.RECORD_FIELDS), dtype=np.float32)
    log[0, F.VRF_Q0:F.VRF_Q0 + 6] = [0.05, 0.1, -0.15, 0.2, -0.1, 0.05]
    log[0, F.VRF_QD0:F.VRF_QD0 + 6] = [0.02, 0.3, -0.2, 0.1, 0.2, -0.1]
    log[0, F.VRF_SMOOTHED_U] = 0.8
    log[0, F.VRF_TARGET_Y], log[0, F.VRF_TARGET_Z] = -0.45, 0.6
    t = np.arange(T + 1)
    log[:, F.VRF_ACTION0] = 0.02 + 0.01 * np.sin(0.7 * t)
    log[:, F.VRF_ACTION0 + 1] = 0.2 + 0.3 * np.sin(0.4 * t + 0.5)
    return log


@pytest.fixture(scope="module")
def recorded():
    """The log of test 2: handle A, 70 envs that all carry TRUTH, pinned to the hand-made row 0, 40 steps on the actions the
    node hands out, env 3 recorded by vine_record behind every step.  Row 0 of the result is the hand-made row."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    log0 = _hand_made_log()
    A = sysid.candidate_task(_task_cfg(N), TRUTH, N, T)
    try:
        assert A.step_kernel_name == "vine_step_kernel"
        ev = sysid.Evaluator(A, log0, T, graph=False)
        rcfg = record_config(A._lib, T, T, 1)
        envs = torch.as_tensor([3], dtype=torch.int32, device=A.device)
        ring = torch.zeros((T, 1, abi.RECORD_FIELDS), device=A.device)
        steps = torch.zeros(T, dtype=torch.int64, device=A.device)
        ev.pin(0)
        for k in range(T):
            A.step_into(ev.actions, ev.obs)
            native.check(A._lib.vine_record(A._handle, rcfg, k, envs.data_ptr(), ev.actions.data_ptr(), A.rew_buf.data_ptr(),
                                            A.reset_buf.data_ptr(), A.progress_buf.data_ptr(), A.timeout_buf.data_ptr(),
                                            ring.data_ptr(), steps.data_ptr(), _stream(A.device)), A._lib)
            ev.node()
        torch.cuda.synchronize()
        rows = ring[:, 0].cpu().numpy()
        truth = A.env_params_of([3])[:, 0].astype(np.float32)
    finally:
        A.close()
    log = np.concatenate([log0[:1], rows])
    assert np.array_equal(log[1:, F.VRF_ACTION0:F.VRF_ACTION0 + 2], log0[1:, F.VRF_ACTION0:F.VRF_ACTION0 + 2])
    assert np.array_equal(log[:, F.VRF_PROGRESS], np.arange(T + 1)) and not log[:, F.VRF_RESET].any()
    assert sysid.windows(log, H, H) == STARTS
    assert truth[abi.VP_DAMPING] == np.float32(0.035) and truth[abi.VP_ACTION_DELAY] == 2.0
    return log, truth


def _candidates(truth, base):
    """70 columns: the truth at 17; 18 differs in the delay only; 19 in FPAM_K[0] by one float32 step; every other column in
    damping, delay and the FPAM_K factor."""
    table = np.repeat(truth[:, None], N, axis=1)
    e = np.arange(N)
    table[abi.VP_DAMPING] = (0.02 + 0.0005 * e).astype(np.float32)
    table[abi.VP_ACTION_DELAY] = e % 4
    table[abi.VP_FPAM_K0:abi.VP_FPAM_K0 + 5] = (base[abi.VP_FPAM_K0:abi.VP_FPAM_K0 + 5, None].astype(np.float64)
                                                * (1.0 + 0.002 * e)[None, :]).astype(np.float32)
    for col in (TRUE_ENV, DELAY_ENV, ULP_ENV):
        table[:, col] = truth
    table[abi.VP_ACTION_DELAY, DELAY_ENV] = 3
    table[abi.VP_FPAM_K0, ULP_ENV] = np.nextafter(truth[abi.VP_FPAM_K0], np.float32(np.inf))
    assert sum(np.array_equal(table[:, c], truth) for c in range(N)) == 1
    return table


def _candidate_batch(log, table=None, weights=None, graph=False):
    B = sysid.candidate_task(_task_cfg(N), TRUTH, N, H)
    if table is not None:
        B.set_env_params({B.env_param_names[p]: table[p] for p in range(abi.VP_COUNT)})
    return B, sysid.Evaluator(B, log, H, weights, graph=graph)


@pytest.fixture(scope="module")
def eager_run(recorded):
    """The candidates of tests 2-5 over windows 0, 12, 24, eagerly: err, alive, the final state block, and the joint state of
    every env after every step (what the node compared)."""
    log, truth = recorded
    B, ev = _candidate_batch(log)
    try:
        base = env_params.config_row(B._lib, B._vcfg)
        table = _candidates(truth, base)
        B.set_env_params({B.env_param_names[p]: table[p] for p in range(abi.VP_COUNT)})
        ev.err.zero_()
        ev.alive.fill_(1)
        snaps = []
        for r in STARTS:
            ev.pin(r)
            for k in range(1, H + 1):
                ev.step()
                snaps.append(B.state[F.VF_Q0:F.VF_Q0 + 12].clone())
        torch.cuda.synchronize()
        out = dict(err=ev.err.cpu().numpy(), alive=ev.alive.cpu().numpy(), state=B.state.clone().cpu(), table=table,
                   snaps=torch.stack(snaps).cpu().numpy().reshape(len(STARTS), H, 12, N),
                   vcfg=(float(B._vcfg.link_length), float(B._vcfg.joint1_z), float(B._vcfg.phi0)))
        # the same through evaluate(): bit-identical sums
        again = ev.evaluate(STARTS)
        assert np.array_equal(again, out["err"])
    finally:
        B.close()
    return out


def test_exact_recovery(recorded, eager_run):
    err, alive = eager_run["err"], eager_run["alive"]
    print("\nerr[17] = %r, err[18] = %r, err[19] = %r, smallest other = %r" % (
        err[TRUE_ENV], err[DELAY_ENV], err[ULP_ENV], np.delete(err, [TRUE_ENV, DELAY_ENV, ULP_ENV]).min()))
    assert alive.all()
    assert err[TRUE_ENV] == 0.0
    others = np.delete(err, TRUE_ENV)
    assert (others > 0.0).all() and np.isfinite(others).all()


def test_exact_recovery_from_a_cold_start(recorded, eager_run):
    """Windows 12 and 24 of the run above start on a batch whose true env has just walked the log up to there.  Here a fresh
    batch is pinned to row 12 first, and then to 24, 12, 0 in that order: whatever the pin leaves alone is not the log's."""
    log, _ = recorded
    B, ev = _candidate_batch(log, eager_run["table"])
    try:
        for starts in ([12], [24, 12, 0]):
            err = ev.evaluate(starts)
            print("\nstarts %s: err[17] = %r, err[18] = %r, err[19] = %r" % (starts, err[TRUE_ENV], err[DELAY_ENV], err[ULP_ENV]))
            assert ev.alive.cpu().numpy().all()
            assert err[TRUE_ENV] == 0.0
            others = np.delete(err, TRUE_ENV)
            assert (others > 0.0).all() and np.isfinite(others).all()
    finally:
        B.close()


def _q_qd_sum(log, snaps, w):
    """float64 numpy: sum over windows, steps and the twelve joint-state fields of w_f (x_f - log_f)^2."""
    want = np.zeros(N)
    for i, r in enumerate(STARTS):
        ref = log[r + 1:r + H + 1, 0:12].astype(np.float64)         # rows r + 1 .. r + H
        want += (w[None, :, None] * (snaps[i] - ref[:, :, None]) ** 2).sum(axis=(0, 1))
    return want


@pytest.mark.parametrize("weights", [[1.0] * 6 + [0.0] * 6, [1.0] * 6 + [0.25] * 6, [1.0, 0.0, 1.0, 2.0, 0.0, 1.0, 0.25, 0.0, 0.0, 0.5, 0.5, 0.0]],
                         ids=["q", "q_qd", "some_q_some_qd"])
def test_error_arithmetic_q_and_qd(recorded, eager_run, weights):
    """Weights on q and qd only (no tip weight: the node reads just the weighted fields).  The device's float64 sums against
    numpy's over the same float32 values, the state block after every eager step: at most 36 x 12 non-negative float64
    terms added in another order, so relative 1e-12.  The weights are exact in float32."""
    log, _ = recorded
    w = np.asarray(weights)
    if weights[:6] == [1.0] * 6 and not any(weights[6:]):
        got = eager_run["err"]                                       # the default weights: the run the snapshots are from
    else:
        B, ev = _candidate_batch(log, eager_run["table"], weights + [0.0] * 4)
        try:
            got = ev.evaluate(STARTS)
            assert torch.equal(B.state.cpu(), eager_run["state"])     # the same trajectories as the run the snapshots are from
        finally:
            B.close()
    want = _q_qd_sum(log, eager_run["snaps"].astype(np.float64), w)
    print("\nmax relative |device - float64| = %.3e" % np.max(np.abs(got - want) / np.maximum(want, 1e-300)))
    assert want[TRUE_ENV] == 0.0 and got[TRUE_ENV] == 0.0
    assert np.isfinite(got).all() and (np.delete(want, TRUE_ENV) > 0).all()
    assert np.all(np.abs(got - want) <= 1e-12 * want)


def test_error_arithmetic_with_qd_and_tip_weights(recorded, eager_run):
    """Weights on q, qd and the four tip fields.  q / qd terms as above.  A tip term is w (x - l)^2 with x the device's fp32
    kinematics of the env's joint state: x = x64 + delta, |delta| <= POS_ULPS (VEL_ULPS) ulps of the largest magnitude in
    the sum, the recorder test's budget for exactly this function; so the term differs from w (x64 - l)^2 by at most
    w (2 |x64 - l| |delta| + delta^2), summed over the compared rows."""
    log, _ = recorded
    weights = [1.0] * 6 + [0.1] * 6 + [2.0, 2.0, 0.5, 0.5]
    B, ev = _candidate_batch(log, eager_run["table"], weights)
    try:
        got = ev.evaluate(STARTS)
        assert torch.equal(B.state.cpu(), eager_run["state"])         # the same trajectories as the run the snapshots are from
    finally:
        B.close()
    snaps = eager_run["snaps"].astype(np.float64)
    w = np.asarray(weights)
    L, z1, phi0 = eager_run["vcfg"]
    want, budget = np.zeros(N), np.zeros(N)
    for i, r in enumerate(STARTS):
        for k in range(H):
            ref = log[r + 1 + k].astype(np.float64)
            x = snaps[i, k]                                          # [12, N]
            want += (w[:12, None] * (x - ref[:12, None]) ** 2).sum(axis=0)
            tip, m_pos, m_vel = _fk64(x[0:6].T, x[6:12].T, L, z1, phi0)
            delta = np.stack([POS_ULPS * _ulp32(m_pos)] * 2 + [VEL_ULPS * _ulp32(m_vel)] * 2, axis=1)      # [N, 4]
            d = np.abs(tip - ref[None, 12:16])
            want += (w[None, 12:] * d ** 2).sum(axis=1)
            budget += (w[None, 12:] * (2.0 * d * delta + delta ** 2)).sum(axis=1)
    print("\nmax |device - float64| = %.3e, its budget there %.3e" % (np.abs(got - want).max(), budget[np.argmax(np.abs(got - want))]))
    assert np.isfinite(got).all()
    assert np.all(np.abs(got - want) <= budget + 1e-12 * want)


def test_a_candidate_that_leaves_the_episode(recorded, eager_run):
    """Env 40 with a RAIL_VELOCITY_SCALE of 60: the log's rail actions (0.01 .. 0.03) become 0.6 .. 1.8 m/s and carry the
    cart from 0.05 m past RAIL_SOFT_LIMIT = 0.3 m within a window of 0.4 s."""
    log, _ = recorded
    table = eager_run["table"].copy()
    table[abi.VP_RAIL_VELOCITY_SCALE, RUNAWAY_ENV] = 60.0
    B, ev = _candidate_batch(log, table)
    try:
        err = ev.evaluate(STARTS)
        alive = ev.alive.cpu().numpy()
    finally:
        B.close()
    assert alive[RUNAWAY_ENV] == 0 and err[RUNAWAY_ENV] == np.inf
    keep = np.arange(N) != RUNAWAY_ENV
    assert alive[keep].all()
    assert np.array_equal(err[keep].view(np.uint64), eager_run["err"][keep].view(np.uint64))
    assert np.isfinite(eager_run["err"][RUNAWAY_ENV])


def test_graph_replay_equals_eager(recorded, eager_run):
    log, _ = recorded
    B, ev = _candidate_batch(log, eager_run["table"], graph=True)
    try:
        assert ev.use_graph
        err = ev.evaluate(STARTS)
        assert ev.graph is not None and ev.steps_run == len(STARTS) * H
        assert np.array_equal(err.view(np.uint64), eager_run["err"].view(np.uint64))
        assert np.array_equal(ev.alive.cpu().numpy(), eager_run["alive"])
        assert torch.equal(B.state.cpu().view(torch.int32), eager_run["state"].view(torch.int32))
        # and again, replaying the same graph
        again = ev.evaluate(STARTS)
        assert np.array_equal(again.view(np.uint64), err.view(np.uint64))
    finally:
        B.close()


def test_fit_end_to_end(recorded, tmp_path, capsys):
    log, truth = recorded
    path = write_trajectory_mat(str(tmp_path / "log.mat"), log, np.arange(len(log)), 0.03332, env=3)
    spec = {"DAMPING": {"values": [0.01, 0.02, 0.03, 0.035, 0.04, 0.05, 0.06, 0.08]}, "ACTION_DELAY": {"values": [0, 1, 2, 3]},
            "FPAM_K": 1.1}                                       # (FPAM_K is no YAML key: the known factor rides in the spec)
    out = sysid.fit(_task_cfg(512), path, spec, num_envs=512, iterations=2, horizon=H, stride=H, seed=42,
                    directory=str(tmp_path), time_str="t")
    assert out["starts"] == STARTS
    assert out["best_error"] == 0.0
    assert np.array_equal(out["best"], truth)
    assert out["best"][abi.VP_DAMPING] == np.float32(0.035) and out["best"][abi.VP_ACTION_DELAY] == 2.0
    assert (out["errors"] == 0.0).sum() >= 1 and out["errors"][0] == 0.0          # column 0 carries the best
    z = np.load(str(tmp_path / "t_sysid.npz"))
    assert out["path"] == str(tmp_path / "t_sysid.npz")
    assert np.array_equal(z["best"], truth) and float(z["best_error"]) == 0.0
    assert list(z["env_param_names"]) == list(abi.ENV_PARAM_ROW_NAMES)
    assert z["table"].shape == (abi.VP_COUNT, 512) and z["errors"].shape == (512,) and list(z["starts"]) == STARTS
    history = json.loads(str(z["history"]))
    assert [h["best_error"] for h in history] == [0.0, 0.0] and "2.0" in history[1]["counts"]["ACTION_DELAY"]
    text = capsys.readouterr().out
    assert text.count("sysid iteration") == 2 and "DAMPING" in text and "candidate-steps/s" in text
