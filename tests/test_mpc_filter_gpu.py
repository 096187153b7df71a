"""MPC_FILTER on the GPU (include/vine_mpc_filter.h, utils/mpc_filter.py): both launches against ``filter_pin_replay`` and
``filter_correct_replay`` with every case of the correction taken; gains 1 against MPC_OBSERVE; the wiring (with an exact model
and no noise the estimate IS the plant's column of the step it belongs to, a dropped frame included, and the controller then
does what a plain one does); the estimate's error under noise against the raw frames'; the captured graph against eager
launches; ``mpc.py``; and ``play`` without ``filter=`` against the golden bits.

Settings: those of tests/test_mpc_observe_gpu.py, whose rig and helpers are used as they are -- episodes of 8 steps, K = 2,
H = 2, M = 3 and M = 257.  "Bit for bit" is literal: floats are compared as words."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_mpc_observe_gpu import SEED, SENTINEL, STEPS, Rig, _cfg, _drive, _env, _plant_cfg, _same, _stream
from tests.test_trajectory_gpu import POS_ULPS, VEL_ULPS, _fk64, _ulp32
from vine_robot_isaacgymenvs_amd import abi, load_task_config, native
from vine_robot_isaacgymenvs_amd.utils import env_params, mpc, mpc_filter, mpc_observe, sysid

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = abi
SLOTS, LOG = abi.MPC_OBSERVE_SLOTS, abi.MPC_OBSERVE_LOG
RING = slice(F.VF_FIFO0, F.VF_PIPE_Y)
NOT_RING = [f for f in range(F.VF_COUNT) if not F.VF_FIFO0 <= f < F.VF_PIPE_Y]
TIP = slice(F.VF_TIP_Y, F.VF_TIP_VZ + 1)
Q, QD = slice(F.VF_Q0, F.VF_Q0 + 6), slice(F.VF_QD0, F.VF_QD0 + 6)


def _np(t):
    return t.cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------------ the two launches
class FilterRig(Rig):
    """The observe rig, and the filter's state: the estimate ring and the diagnostic full of a sentinel, no estimate yet."""

    def __init__(self, M, gain, predictor_table=None):
        super().__init__(M, C=3, predictor_table=predictor_table)
        d = self.dev
        self.gain_host = np.ascontiguousarray(gain, dtype=np.float32)
        self.gain = torch.as_tensor(self.gain_host, device=d).contiguous()
        self.est = torch.full((SLOTS, F.VF_COUNT, M), SENTINEL, device=d)
        self.est_index = torch.full((M,), -1, dtype=torch.int64, device=d)
        self.innov = torch.full((2, M), SENTINEL, device=d)

    def filter_pin(self, predictor=None, plant=None):
        r = predictor or self.predictor
        return self.lib.vine_mpc_filter_pin(
            (plant or self.plant).h, r.h, self.ocfg, self.table.data_ptr(), self.plant.progress_t.data_ptr(), self.est.data_ptr(),
            self.est_index.data_ptr(), self.act_log.data_ptr(), self.age.data_ptr(), self.fresh.data_ptr(), self.actions.data_ptr(),
            r.rew_t.data_ptr(), r.reset_t.data_ptr(), r.progress_t.data_ptr(), _stream(self.dev))

    def filter_correct(self, predictor=None, plant=None):
        return self.lib.vine_mpc_filter_correct(
            (plant or self.plant).h, (predictor or self.predictor).h, self.ocfg, self.table.data_ptr(), self.gain.data_ptr(),
            self.snap.data_ptr(), self.age.data_ptr(), self.fresh.data_ptr(), self.est.data_ptr(), self.est_index.data_ptr(),
            self.innov.data_ptr(), _stream(self.dev))


def _gains(M):
    """GAIN_Q and GAIN_QD over {0, 0.3, 1}.  M = 3: a plant blended with GAIN_Q 0, one with both gains 1, and the noise-free
    one; beyond that every pair of the three values, the delays (p mod 3) running through each."""
    if M == 3:
        return np.float32([[0.0, 1.0, 0.3], [0.3, 1.0, 0.3]])
    p = np.arange(M)
    return np.stack([np.float32([0, 0.3, 1])[(p // 3) % 3], np.float32([0.3, 1, 0])[(p // 9) % 3]])


@pytest.mark.parametrize("M", [3, 257])
def test_both_launches_against_their_replays_and_every_case_occurs(M):
    """In front of the plant's first step and behind every one of twelve: the pin, one predictor step, the correction, each
    against its numpy statement in every bit -- the column every lane is put on, progress, reset, rew, the rebuilt ring
    (against what ``vine_mpc_fork`` rebuilds on a third handle from ``ring_history`` at the same step count) and the action;
    the estimate ring, ``est_index`` and ``innov``.  DELAY {0, 1, 3}, HOLD 0.3, both noises (but on the last plant), gains
    {0, 0.3, 1}; the predictors of the noisy plants have delays 0 .. 8 and rail scales of their own.  Episodes of 8 steps end
    inside the run.  Two things are done from outside so that every case is taken: one ``est_index`` is knocked off its step
    (the case no steady run reaches), and the last plant's frames are given the joint values of their predictions (innovations
    of exactly zero).  Every case of the correction is asserted to have occurred.  The tips a blended estimate derives are
    handed to the replay from the device (numpy does not reproduce float32 sincosf) and held to their own two checks, the
    measurement's: all four components against the float64 kinematics within POS_ULPS / VEL_ULPS ulps of the largest magnitude
    in the sums, and -- M = 3 -- every joint-determined field against ``vine_sysid_pin`` fed the same q, qd, in every bit."""
    lib = native.load()
    ptable = np.repeat(env_params.config_row(lib, _cfg(M))[:, None], M, axis=1)
    noisy = np.arange(M) != M - 1                                    # (the observe rig's table: its last plant is noise-free)
    ptable[abi.VP_ACTION_DELAY, noisy] = (np.arange(M) % 9)[noisy]
    ptable[abi.VP_RAIL_VELOCITY_SCALE, noisy] = (0.7 + 0.001 * np.arange(M))[noisy]
    rig = FilterRig(M, _gains(M), predictor_table=ptable)
    ref = _env(_cfg(2 * M), np.repeat(ptable, 2, axis=1))
    seen = {c: 0 for c in mpc_filter.CASES}
    seen.update(advancing=0, ring=0)
    blended = []                                                     # the columns of the blended estimates
    try:
        table, gain, d, pred = rig.table_host, rig.gain_host, rig.dev, rig.predictor
        assert np.all(table[abi.VMO_NOISE_Q][noisy] != 0) and table[abi.VMO_NOISE_Q, M - 1] == table[abi.VMO_NOISE_QD, M - 1] == 0
        mcfg = mpc.mpc_config(M, 2, 1, 0.05, [0.0, 0.0], SEED)
        fork_buf = {"nominal": torch.zeros((M, 1, 2), device=d), "history": torch.zeros((M, F.MAX_DELAY, 2), device=d),
                    "tick": torch.zeros(M, dtype=torch.long, device=d), "actions": torch.zeros((2 * M, 2), device=d),
                    "cost": torch.zeros(2 * M, dtype=torch.float64, device=d), "alive": torch.zeros(2 * M, dtype=torch.uint8, device=d),
                    "window": torch.zeros(1, dtype=torch.long, device=d)}

        def fork_ring(history):
            """The ring ``vine_mpc_fork`` rebuilds from the same actions at the predictor's step count."""
            fork_buf["history"].copy_(torch.as_tensor(np.ascontiguousarray(history)))
            ref.state_t[RING] = SENTINEL
            ref.step_count = pred.step_count
            b = fork_buf
            rc = lib.vine_mpc_fork(rig.plant.h, ref.h, mcfg, rig.plant.progress_t.data_ptr(), b["nominal"].data_ptr(),
                                   b["history"].data_ptr(), b["tick"].data_ptr(), b["actions"].data_ptr(), ref.rew_t.data_ptr(),
                                   ref.reset_t.data_ptr(), ref.progress_t.data_ptr(), b["cost"].data_ptr(), b["alive"].data_ptr(),
                                   b["window"].data_ptr(), _stream(d))
            assert rc == abi.OK, lib.vine_last_error()
            torch.cuda.synchronize()
            return ref.state_t[RING][:, ::2].cpu().numpy()

        def control_step_front(t, state, column, progress):
            """What a control step issues in front of the observe pin, with ``t`` plant steps completed."""
            if t == 7:                                               # from outside: plant 0's estimate is of another step
                rig.est_index[0] = 1
            est0, index0, innov0 = _np(rig.est), _np(rig.est_index), _np(rig.innov)
            pred.state_t[RING] = SENTINEL
            pred.reset_t.fill_(1)
            pred.rew_t.fill_(SENTINEL)
            pred.progress_t.fill_(2)
            rig.actions.fill_(SENTINEL)
            assert rig.filter_pin() == abi.OK, lib.vine_last_error()
            torch.cuda.synchronize()
            want = mpc_filter.filter_pin_replay(table, state, est0, index0, column, progress, t)
            adv, st = want["advancing"], _np(pred.state_t)
            assert _same(st[NOT_RING], want["column"][NOT_RING]), t
            assert np.array_equal(_np(pred.progress_t), np.where(adv, want["progress"], 2)), t
            assert np.array_equal(_np(pred.reset_t), np.where(adv, 0, 1)), t
            assert _same(_np(pred.rew_t), np.where(adv, 0, SENTINEL).astype(np.float32)), t
            assert _same(_np(rig.actions), want["actions"]), t
            ring = fork_ring(want["ring_history"])
            rebuilt = (np.arange(2 * F.MAX_DELAY)[:, None] // 2 < ptable[abi.VP_ACTION_DELAY][None, :]) & adv[None, :]
            assert _same(st[RING][rebuilt], ring[rebuilt]) and np.all(st[RING][~rebuilt] == SENTINEL), t
            assert _same(_np(rig.est), est0) and np.array_equal(_np(rig.est_index), index0)          # the pin reads them only
            seen["advancing"] += int(adv.sum())
            seen["ring"] += int(rebuilt.sum())
            pred.step_t(rig.actions, sync=False)
            torch.cuda.synchronize()
            xminus = _np(pred.state_t)
            if adv[M - 1]:                                           # from outside: a frame that agrees with its prediction
                rig.snap[int(want["e"][M - 1]) % SLOTS, :12, M - 1] = pred.state_t[:12, M - 1]
                state = dict(state, snap=_np(rig.snap))
            assert rig.filter_correct() == abi.OK, lib.vine_last_error()
            torch.cuda.synchronize()
            got = {"est": _np(rig.est), "est_index": _np(rig.est_index), "innov": _np(rig.innov)}

            def device_tip(q, qd, plants):                           # numpy does not reproduce float32 sincosf
                p = int(plants[0])
                return got["est"][int(want["e"][p]) % SLOTS][TIP][:, [p]].T

            new = mpc_filter.filter_correct_replay(table, gain, SEED, state, est0, index0, innov0, xminus, t, tip=device_tip)
            for k in ("est", "est_index", "innov"):
                assert _same(got[k], new[k]), (t, k, list(new["case"][:9]))
            assert np.all(got["est"][:, RING] == SENTINEL), t            # an estimate holds no delay ring
            assert _same(_np(pred.state_t), xminus), t                   # the correction reads the predictor only
            for c in new["case"]:
                seen[c] += 1
            assert np.array_equal(adv, np.isin(new["case"], ("held", "unit", "still", "blend"))), t
            # the replay was handed the device's tips: every blended estimate's four tip components are held to the float64
            # kinematics of its own joint values within the recorder test's budget, as the measurement's are
            sel = np.flatnonzero(new["case"] == "blend")
            if len(sel):
                cols = np.stack([got["est"][int(want["e"][p]) % SLOTS][:, p] for p in sel])          # [B, VF_COUNT]
                vc = rig.plant.cfg
                tip64, m_pos, m_vel = _fk64(cols[:, Q].astype(np.float64), cols[:, QD].astype(np.float64), float(vc.link_length),
                                            float(vc.joint1_z), float(vc.phi0))
                tol = np.stack([POS_ULPS * _ulp32(m_pos)] * 2 + [VEL_ULPS * _ulp32(m_vel)] * 2, axis=1)
                assert np.all(np.abs(cols[:, TIP].astype(np.float64) - tip64) <= tol), t
                blended.extend(cols)
            assert new["case"][M - 1] in ("known", "first", "same", "held", "still"), t

        control_step_front(0, rig.state(), _np(rig.plant.state_t), _np(rig.plant.progress_t))
        assert seen["known"] == M

        def each(t, cols, progress, states):
            control_step_front(t + 1, states[-1], cols[-1], progress[-1])

        _drive(rig, each=each)
        for c in mpc_filter.CASES:
            assert seen[c] >= 1, (c, seen)
        assert seen["first"] >= 2 * M and seen["advancing"] >= 2 * M and seen["ring"] >= 2, seen
        assert len(blended) == seen["blend"]
        if M == 3:
            _derived_against_sysid_pin(lib, blended)
    finally:
        ref.close()
        rig.close()


def _derived_against_sysid_pin(lib, columns):
    """``vine_sysid_pin`` on a log whose rows are the blended joint states: the same q, qd, the same ``tip_fk_joint`` -- the
    joint-determined fields of every blended estimate are the bits the measurement forms (tests/test_mpc_observe_gpu.py holds
    the measurement's own to the same pin)."""
    H = 1
    assert len(columns) >= 3
    log = np.zeros((len(columns) + H + 1, abi.RECORD_FIELDS), dtype=np.float32)
    for r, col in enumerate(columns):
        log[r, F.VRF_Q0:F.VRF_Q0 + 12] = col[:12]
    env = _env(_cfg(4), lane=True)
    try:
        log_t = torch.as_tensor(log, device=env.dev)
        scfg = sysid.sysid_config(lib, len(log), H)
        buf = [torch.zeros((4, 2), device=env.dev), torch.zeros(4, device=env.dev), torch.ones(4, dtype=torch.long, device=env.dev),
               torch.zeros(4, dtype=torch.long, device=env.dev), torch.zeros(2, dtype=torch.long, device=env.dev)]
        for r, col in enumerate(columns):
            rc = lib.vine_sysid_pin(env.h, scfg, log_t.data_ptr(), r, *[b.data_ptr() for b in buf], _stream(env.dev))
            assert rc == abi.OK, lib.vine_last_error()
            torch.cuda.synchronize()
            st = env.state_t.cpu().numpy()[:, 0]
            for f in list(range(12)) + [F.VF_TIP_Y, F.VF_TIP_Z, F.VF_TIP_VY, F.VF_TIP_VZ, F.VF_CART_Y, F.VF_CART_VY, F.VF_PREV_TIP_Y,
                                        F.VF_PREV_TIP_Z, F.VF_PREV_CART_VEL] + list(range(F.VF_PREV_Q0, F.VF_PREV_Q0 + 6)):
                assert _same(st[f], col[f]), (r, f)
    finally:
        env.close()


def test_filter_refusals_name_the_reason():
    M = 3
    rig = FilterRig(M, _gains(M))
    lib, others = rig.lib, []
    try:
        def other(cfg):
            others.append(_env(cfg))
            return others[-1]

        def refused(rc, code, word, whole=False):
            assert rc == code and (lib.vine_last_error() == word if whole else word in lib.vine_last_error()), (rc, lib.vine_last_error())

        for launch in (rig.filter_pin, rig.filter_correct):
            refused(launch(predictor=other(_cfg(M + 1))), abi.ERR_INVALID_ARG, b"mpc filter: the predictor handle has 4 envs, not num_plants = 3")
            refused(launch(plant=others[-1]), abi.ERR_INVALID_ARG, b"mpc filter: the plant handle does not have num_plants envs")
            cfg = _cfg(M)
            cfg.set_flag(abi.FLAG_VINE_RANDOMIZE, True)
            refused(launch(predictor=other(cfg)), abi.ERR_UNSUPPORTED, b"mpc filter: a predictor handle with vine_randomize is refused "
                    b"(a replayed step must be a deterministic one)", whole=True)
            refused(launch(predictor=other(_cfg(M, pipe=True))), abi.ERR_UNSUPPORTED,
                    b"mpc filter: the predictor handle's CREATE_SHELF / CREATE_PIPE differ from the plant's", whole=True)
            cfg = _cfg(M)
            cfg.max_episode_length = 9
            refused(launch(predictor=other(cfg)), abi.ERR_INVALID_ARG,
                    b"mpc filter: the predictor handle's max_episode_length differs from the plant's", whole=True)
            refused(launch(predictor=rig.plant), abi.ERR_INVALID_ARG, b"two handles")
            if torch.cuda.device_count() > 1:
                from tests.hip_env import HipEnv
                others.append(HipEnv(_cfg(M), device_id=1))
                refused(launch(predictor=others[-1]), abi.ERR_INVALID_ARG, b"mpc filter: the predictor handle sits on another device")
            assert launch() == abi.OK
        torch.cuda.synchronize()
    finally:
        for o in others:
            o.close()
        rig.close()


# ------------------------------------------------------------------------------------------------------ the task classes
class Tasks:
    """A plant, its model and predictor tasks and the filtering controller; ``beside``: also an identically seeded plant with
    a plain ``Controller`` (``"plain"``) or an ``ObservingController`` (``"observe"``)."""

    def __init__(self, M, observe, filter, pipe=False, beside=None, K=2, H=2, episode=8, **ctl):
        cfg = _plant_cfg(M, pipe, maxEpisodeLength=episode)
        self.all = []
        make = lambda c: self.all.append(mpc.make_task(c)) or self.all[-1]          # noqa: E731
        # cost={}: the model keeps the plant's own reward weights -- an exact model, VF_AGG_REW included
        self.plant, self.model = make(cfg), make(mpc.model_config(cfg, M, K, cost={}))
        self.predictor = make(mpc.model_config(cfg, M, 1, cost={}))
        self.ctl = mpc_filter.FilteringController(self.plant, self.model, self.predictor, K, observe, filter, H, seed=5, **ctl)
        if beside:
            self.plant2, self.model2 = make(cfg), make(mpc.model_config(cfg, M, K, cost={}))
            if beside == "plain":
                self.ctl2 = mpc.Controller(self.plant2, self.model2, K, H, seed=5, **ctl)
            else:
                self.predictor2 = make(mpc.model_config(cfg, M, 1, cost={}))
                self.ctl2 = mpc_observe.ObservingController(self.plant2, self.model2, self.predictor2, K, observe, H, seed=5, **ctl)

    def close(self):
        for t in reversed(self.all):
            t.close()


def _frame_steps(ctl, t):
    """known, dd and e per plant in front of the control step with ``t`` plant steps completed."""
    age, fresh = _np(ctl.age).astype(np.int64), _np(ctl.fresh)
    known = (fresh != 0) | (t == 0)
    dd = np.where(known, 0, np.minimum(ctl.table_host[abi.VMO_DELAY].astype(np.int64), age))
    return known, dd, t - 1 - dd


@pytest.mark.parametrize("M", [3, 257])
def test_gains_one_without_held_frames_reproduce_mpc_observe(M):
    """Both gains 1, HOLD 0, DELAY {0, 1, 3} and both noises: behind the correction of every one of twelve control steps the
    estimate equals the raw frame at every delivered slot, and ``plant_actions`` and ``nominal`` equal those of an
    ``ObservingController`` on an identically seeded plant, every bit."""
    observe = {"DELAY": {"values": [0, 1, 3]}, "NOISE_Q": 0.01, "NOISE_QD": 0.05, "CATCHUP": 3}
    T = Tasks(M, observe, {"GAIN_Q": 1.0, "GAIN_QD": 1.0}, beside="observe", graph=False)
    try:
        ctl, ctl2 = T.ctl, T.ctl2
        assert np.all(ctl.gain_host == 1.0) and not ctl.use_graph and _same(ctl.table_host, ctl2.table_host)
        delivered, resets = 0, 0
        for t in range(STEPS):
            known, dd, e = _frame_steps(ctl, t)
            ctl.predict()
            torch.cuda.synchronize()
            est, snap, index = _np(ctl.est), _np(ctl.snap), _np(ctl.est_index)
            assert np.array_equal(index, np.where(known, -1, e)), t
            for p in np.flatnonzero(~known):
                assert _same(est[e[p] % SLOTS][NOT_RING, p], snap[e[p] % SLOTS][NOT_RING, p]), (t, p)
            delivered += int((~known).sum())
            resets += int(T.plant.reset_buf.sum())
            mpc.Controller.control_step(ctl)
            ctl.measure()
            ctl2.control_step()
            torch.cuda.synchronize()
            assert _same(_np(ctl.plant_actions), _np(ctl2.plant_actions)), t
            assert _same(_np(ctl.nominal), _np(ctl2.nominal)), t
            assert _same(_np(T.plant.state), _np(T.plant2.state)) and _same(_np(ctl.snap), _np(ctl2.snap)), t
        assert delivered == (STEPS - 1) * M and resets >= M and np.abs(_np(ctl.nominal)).max() > 0
        assert ctl.launches["filter_pin"] == ctl.launches["filter_correct"] == STEPS
        assert ctl.launches["predictor_step"] == 4 * STEPS and ctl2.launches["predictor_step"] == 3 * STEPS
    finally:
        T.close()


@pytest.mark.parametrize("M, d, pipe, hold", [
    (3, 0, False, 0.0), (3, 1, False, 0.0), (3, 3, False, 0.0), (3, 0, True, 0.0), (3, 1, True, 0.0), (3, 3, True, 0.0),
    (257, 3, True, 0.0), (3, 1, False, 0.3), (3, 3, True, 0.3), (257, 0, True, 0.3), (257, 3, False, 0.3)])
def test_with_an_exact_model_the_estimate_is_the_plants_column(M, d, pipe, hold):
    """Exact model (the plant's reward weights too), no noise, gains 0.3, a common DELAY d with C = 3.  At every one of twelve
    control steps ``est[e mod S]`` equals the plant's true column behind step e (kept here, step by step) in every bit outside
    the ring; the predictor behind the catch-up equals the plant's current column; ``plant_actions`` and ``nominal`` equal a
    plain ``Controller``'s on an identically seeded plant.  With HOLD 0.3 the same holds -- a held frame is predicted through
    exactly -- whereas the raw ring, which MPC_OBSERVE would deliver, holds the stale frame on at least one such step."""
    T = Tasks(M, {"DELAY": d, "CATCHUP": 3, "HOLD": hold}, {"GAIN_Q": 0.3, "GAIN_QD": 0.3}, pipe=pipe, beside="plain", graph=False)
    try:
        ctl, ctl2 = T.ctl, T.ctl2
        assert ctl.C == 3 and not ctl.use_graph and np.all(ctl.gain_host == np.float32(0.3))
        truth, checked, stale, resets = [], 0, 0, 0
        for t in range(STEPS):
            known, dd, e = _frame_steps(ctl, t)
            ctl.predict()
            torch.cuda.synchronize()
            est, snap, index = _np(ctl.est), _np(ctl.snap), _np(ctl.est_index)
            assert np.array_equal(index, np.where(known, -1, e)), t
            for p in np.flatnonzero(~known):
                want = truth[e[p]][NOT_RING, p]
                assert _same(est[e[p] % SLOTS][NOT_RING, p], want), (t, p, [f for f, a, b in zip(NOT_RING, est[e[p] % SLOTS][NOT_RING, p], want)
                                                                            if not _same(a, b)])
                checked += 1
                stale += int(not _same(snap[e[p] % SLOTS][NOT_RING, p], want))
            pst, st = _np(T.plant.state), _np(T.predictor.state)
            assert _same(st[NOT_RING], pst[NOT_RING]), (t, [f for f in NOT_RING if not _same(st[f], pst[f])])
            assert np.array_equal(_np(T.predictor.progress_buf), _np(T.plant.progress_buf)), t
            resets += int(T.plant.reset_buf.sum())
            mpc.Controller.control_step(ctl)
            ctl.measure()
            ctl2.control_step()
            torch.cuda.synchronize()
            truth.append(_np(T.plant.state))
            assert _same(_np(ctl.plant_actions), _np(ctl2.plant_actions)), t
            assert _same(_np(ctl.nominal), _np(ctl2.nominal)), t
            assert _same(truth[-1], _np(T.plant2.state)), t
        assert checked == (STEPS - 1) * M and resets >= M and np.abs(_np(ctl.nominal)).max() > 0
        assert (stale >= 1) if hold else (stale == 0), stale             # only a held frame differs from its step's column
        assert float(_np(ctl.innov).max()) == 0.0                        # no innovation was ever seen
    finally:
        T.close()


def _estimate_error(gain, steps=40, M=257):
    """rms over plants and steps of est[e mod S] minus the plant's true column behind step e, for q and for qd: an exact model,
    DELAY 1, NOISE_Q 0.01, NOISE_QD 0.1, episodes of ``steps`` steps."""
    T = Tasks(M, {"DELAY": 1, "NOISE_Q": 0.01, "NOISE_QD": 0.1}, {"GAIN_Q": gain, "GAIN_QD": gain}, episode=steps, graph=False)
    try:
        ctl, truth = T.ctl, []
        sq, sqd, n = 0.0, 0.0, 0
        for t in range(steps):
            known, dd, e = _frame_steps(ctl, t)
            ctl.predict()
            torch.cuda.synchronize()
            est = _np(ctl.est)
            for p in np.flatnonzero(~known):
                diff = est[e[p] % SLOTS][:12, p].astype(np.float64) - truth[e[p]][:12, p].astype(np.float64)
                sq, sqd, n = sq + float((diff[:6] ** 2).sum()), sqd + float((diff[6:] ** 2).sum()), n + 6
            mpc.Controller.control_step(ctl)
            ctl.measure()
            torch.cuda.synchronize()
            truth.append(_np(T.plant.state))
        assert n >= 6 * M * (steps - 2)
        return np.sqrt(sq / n), np.sqrt(sqd / n)
    finally:
        T.close()


def test_it_is_a_filter():
    """M = 257, exact model, DELAY 1, NOISE_Q 0.01, NOISE_QD 0.1, 40 control steps in episodes of 40: the rms error of the
    estimate with gains 0.3 lies strictly below the rms error with gains 1 (the raw frames), for q and for qd.  The two ratios
    are printed (profiles/mpc_filter/it_matters.txt records them: 0.52 for q and 0.71 for qd when this test was written, against
    sqrt(G / (2 - G)) = 0.42 for a contractive plant)."""
    raw_q, raw_qd = _estimate_error(1.0)
    fil_q, fil_qd = _estimate_error(0.3)
    print("\nmpc filter: rms error of the estimate, gains 1: q %.6g qd %.6g; gains 0.3: q %.6g qd %.6g; ratios q %.4f qd %.4f" % (
        raw_q, raw_qd, fil_q, fil_qd, fil_q / raw_q, fil_qd / raw_qd), flush=True)
    assert raw_q > 0 and raw_qd > 0
    assert fil_q < raw_q, (fil_q, raw_q)
    assert fil_qd < raw_qd, (fil_qd, raw_qd)


@pytest.mark.parametrize("C", [0, 3])
def test_captured_control_steps_against_eager_ones(C):
    """Two captured control steps replayed three times against six eager ones: every controller tensor -- the estimate ring,
    ``est_index`` and ``innov`` among them -- and all three state blocks bit-identical.  C = 3: DELAY {0, 1, 3}, HOLD 0.3 and
    both noises, gains {0.3, 1} x {0.3}; C = 0: no delay, the rest the same."""
    M = 3
    observe = {"DELAY": {"values": [0, 1, 3]} if C else 0, "HOLD": 0.3, "NOISE_Q": 0.002, "NOISE_QD": 0.01}
    runs = []
    for tag, kw in (("graph", dict(graph=True, graph_steps=2)), ("eager", dict(graph=False))):
        T = Tasks(M, observe, {"GAIN_Q": {"values": [0.3, 1.0]}, "GAIN_QD": 0.3}, **kw)
        try:
            ctl = T.ctl
            assert ctl.use_graph == (tag == "graph") and ctl.C == C
            ctl.run(6)
            torch.cuda.synchronize()
            counts = {"fork": 6, "step": 12, "node": 12, "update": 6, "plant_step": 6, "pin": 6, "catchup": 6 * C,
                      "predictor_step": 6 * (C + 1), "measure": 6, "filter_pin": 6, "filter_correct": 6}
            if tag == "graph":
                assert ctl.graph_launches == {k: v // 3 for k, v in counts.items()}
            assert ctl.launches == counts
            assert (T.plant.step_count, T.model.step_count, T.predictor.step_count) == (6, 12, 6 * (C + 1))
            assert (T.plant.num_steps, T.model.num_steps, T.predictor.num_steps) == (6, 12, 6 * (C + 1))
            tensors = ctl.tensors()
            assert any(t is ctl.est for t in tensors) and any(t is ctl.est_index for t in tensors) and any(t is ctl.innov for t in tensors)
            runs.append(([_np(t) for t in tensors], [_np(t.state) for t in (T.plant, T.model, T.predictor)], _np(ctl.est_index)))
        finally:
            T.close()
    (ta, sa, index), (tb, sb, _) = runs
    for a, b in zip(ta + sa, tb + sb):
        assert _same(a, b)
    assert np.abs(ta[0]).max() > 0 and (index >= 0).all()                  # the nominal moved, every plant has an estimate


def test_reset_plants_forgets_the_estimate():
    T = Tasks(3, {"DELAY": 1}, {})
    try:
        ctl = T.ctl
        assert np.all(ctl.gain_host == np.float32(mpc_filter.DEFAULT_GAIN)) and list(_np(ctl.est_index)) == [-1, -1, -1]
        ctl.run(3)
        torch.cuda.synchronize()
        assert (_np(ctl.est_index) >= 0).all()
        ctl.reset_plants([1])
        torch.cuda.synchronize()
        index = _np(ctl.est_index)
        assert index[1] == -1 and index[0] >= 0 and index[2] >= 0 and list(_np(ctl.fresh)) == [0, 1, 0]
        ctl.run(2)
        torch.cuda.synchronize()
        assert (_np(ctl.est_index) >= 0).all()
    finally:
        T.close()


# ---------------------------------------------------------------------------------------------------------- entry points
def test_the_command_line_with_filter(tmp_path):
    """``mpc.py``'s main with ``observe=`` and ``filter=``: runs from the graph, counts the filter's launches and its extra
    predictor step, reports the gain table and the mean innovation, and bins by the gain that varies."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mpc_cli", os.path.join(REPO, "mpc.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    H = 4
    argv = ["plants=4", "samples=16", "horizon=%d" % H, "steps=12", "sigma=[0.5, 0.25]", "lambda=0.1", "out=%s" % tmp_path,
            "task.env.EPISODE_LOG=True", "task.env.maxEpisodeLength=8", "task.env.CREATE_PIPE=False",
            "task.task.vine_randomize=False", "seed=3", "observe={DELAY: {values: [1, 3]}, HOLD: 0.1, NOISE_Q: 0.002}",
            "filter={GAIN_Q: {values: [0.2, 0.6]}, GAIN_QD: 0.5}"]
    out = cli.main(argv)
    assert out["graphed"] and np.isfinite(out["plant_return"]).all() and out["report"]["episodes"] >= 4
    assert out["launches"] == {"fork": 12, "step": 12 * H, "node": 12 * H, "update": 12, "plant_step": 12, "pin": 12,
                               "catchup": 36, "predictor_step": 48, "measure": 12, "filter_pin": 12, "filter_correct": 12}
    fl = out["filter"]
    assert fl["names"] == ["GAIN_Q", "GAIN_QD"] and fl["gain"].shape == (2, 4) and fl["innov"].shape == (2,)
    assert _same(fl["gain"], np.float32([[0.2, 0.6, 0.2, 0.6], [0.5] * 4])) and np.all(fl["innov"] >= 0)
    assert out["observe"]["catchup"] == 3 and list(out["observe"]["table"][0]) == [1, 3, 1, 3]
    assert list(out["by_param"]) == ["param_FILTER_GAIN_Q"]              # the gain that varies, not the one that does not
    with pytest.raises(mpc_filter.ConfigError, match="filter= needs observe="):
        cli.main(argv[:-2] + [argv[-1]])


def test_without_filter_nothing_changes():
    """``play`` without ``filter=``: the summed plant reward and the launch counts of tests/golden/mpc_play_no_adapt.json, bit
    for bit; with ``observe=`` alone an ``ObservingController`` is what runs, and it launches nothing of the filter."""
    with open(os.path.join(REPO, "tests", "golden", "mpc_play_no_adapt.json")) as f:
        golden = json.load(f)

    def cfg():
        c = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=4"])
        c["seed"] = 9
        c["task"]["vine_randomize"] = False
        c["env"].update(CREATE_PIPE=False, CREATE_SHELF=False, maxEpisodeLength=10)
        return c

    for name, extra in (("plain", {}), ("model_params", {"model_params": {"DAMPING": [0.01, 0.05]}})):
        out = mpc.play(cfg(), samples=16, horizon=6, steps=12, lam=0.05, sigma=[0.5, 0.25], seed=3, **extra)
        want = golden[name]
        assert [int(x) for x in out["plant_return"].view(np.uint64)] == want["plant_return_bits"], name
        assert out["launches"] == want["launches"] == {"fork": 12, "step": 72, "node": 72, "update": 12, "plant_step": 12}
        assert "filter" not in out and "observe" not in out
    out = mpc.play(cfg(), samples=16, horizon=6, steps=4, seed=3, observe={"DELAY": 1})
    assert "filter" not in out and "filter_pin" not in out["launches"] and out["launches"]["predictor_step"] == 4
