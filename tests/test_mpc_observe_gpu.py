"""MPC_OBSERVE on the GPU (include/vine_mpc_observe.h, utils/mpc_observe.py): the measurement against ``measure_replay`` and
the tips it derives against ``vine_sysid_pin`` and a float64 kinematics; the pin and the catch-up node against ``pin_replay``
and ``catchup_schedule``; the wiring (an exact model catches up with its plant in every bit, and the controller then does what
a plain one does); the stale frame without compensation; the captured graph against eager launches; ``mpc.py``; and ``play``
without ``observe=`` against the golden bits.

Settings: episodes of 8 steps, so resets and young episodes occur inside a dozen steps; K = 2, H = 2; M = 3 (the smallest that
holds the three delays 0, 1, 3) and M = 257 (crosses a workgroup boundary).  "Bit for bit" is literal: floats are compared as
words."""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import base_cfg
from tests.test_trajectory_gpu import POS_ULPS, VEL_ULPS, _fk64, _ulp32
from vine_robot_isaacgymenvs_amd import abi, load_task_config, native
from vine_robot_isaacgymenvs_amd.utils import env_params, mpc, mpc_observe, sysid

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = abi
SENTINEL = -7777.0
SLOTS, LOG = abi.MPC_OBSERVE_SLOTS, abi.MPC_OBSERVE_LOG
RING = slice(F.VF_FIFO0, F.VF_PIPE_Y)
NOT_RING = [f for f in range(F.VF_COUNT) if not F.VF_FIFO0 <= f < F.VF_PIPE_Y]
TIP = slice(F.VF_TIP_Y, F.VF_TIP_VZ + 1)
STEPS = 12
SEED = 77


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _cfg(n, pipe=False):
    cfg = base_cfg(n, 0, False, max_episode_length=8, action_delay=1)
    for f in (abi.FLAG_USE_TARGET_REACHED_RESET, abi.FLAG_USE_TIP_LIMIT_HIT_RESET, abi.FLAG_USE_NONZERO_CONTACT_FORCE_RESET,
              abi.FLAG_CREATE_SHELF, abi.FLAG_CREATE_PIPE):
        cfg.set_flag(f, False)
    cfg.set_flag(abi.FLAG_CREATE_PIPE, pipe)
    return cfg


def _env(cfg, table=None, lane=False):
    from tests.hip_env import HipEnv
    env = (type("HipEnvLane", (HipEnv,), {"kernel": "lane"}) if lane else HipEnv)(cfg)
    if table is not None:
        env_params.check_table(env.lib, env.cfg, table)
        env.table_t = torch.as_tensor(np.ascontiguousarray(table, np.float32)).to(env.dev).contiguous()
        torch.cuda.synchronize(env.dev)
        native.check(env.lib.vine_bind_env_params(env.h, env.table_t.data_ptr()), env.lib)
    return env


def _table(M):
    """DELAY 0, 1, 3 by plant, HOLD 0.3, both noises non-zero (but on the last plant: a noise-free one among them)."""
    t = np.zeros((4, M), dtype=np.float32)
    t[abi.VMO_DELAY] = np.float32([0, 1, 3])[np.arange(M) % 3]
    t[abi.VMO_HOLD] = 0.3
    t[abi.VMO_NOISE_Q], t[abi.VMO_NOISE_QD] = 0.01, 0.05
    t[abi.VMO_NOISE_Q, M - 1] = t[abi.VMO_NOISE_QD, M - 1] = 0.0
    if M > 4:
        t[abi.VMO_NOISE_QD, 3] = 0.0                     # ... and one with noise on q alone
    return t


class Rig:
    """A plant and a predictor handle through the C ABI, and the controller's buffers."""

    def __init__(self, M, C=3, predictor_table=None):
        self.M, self.C = M, C
        self.lib = native.load()
        self.plant = _env(_cfg(M))
        self.predictor = _env(_cfg(M), predictor_table)
        d = self.dev = self.plant.dev
        self.table_host = _table(M)
        self.ocfg = mpc_observe.observe_cconfig(M, C, True, SEED, self.table_host)
        self.table = torch.as_tensor(self.table_host, device=d).contiguous()
        self.snap = torch.full((SLOTS, F.VF_COUNT, M), SENTINEL, device=d)
        self.act_log = torch.zeros((M, LOG, 2), device=d)
        self.age = torch.full((M,), 5, dtype=torch.int32, device=d)
        self.fresh = torch.ones(M, dtype=torch.uint8, device=d)
        self.lag = torch.full((M,), -9, dtype=torch.int32, device=d)
        self.actions = torch.full((M, 2), SENTINEL, device=d)
        self.plant_actions = torch.zeros((M, 2), device=d)

    def measure(self):
        p = self.plant
        rc = self.lib.vine_mpc_observe_measure(p.h, self.ocfg, self.table.data_ptr(), p.progress_t.data_ptr(),
                                               self.plant_actions.data_ptr(), self.snap.data_ptr(), self.act_log.data_ptr(),
                                               self.age.data_ptr(), self.fresh.data_ptr(), _stream(self.dev))
        assert rc == abi.OK, self.lib.vine_last_error()

    def _pin_args(self, predictor):
        r = predictor or self.predictor
        return [self.table.data_ptr(), self.plant.progress_t.data_ptr(), self.snap.data_ptr(), self.act_log.data_ptr(),
                self.age.data_ptr(), self.fresh.data_ptr(), self.actions.data_ptr(), r.rew_t.data_ptr(), r.reset_t.data_ptr(),
                r.progress_t.data_ptr(), self.lag.data_ptr(), _stream(self.dev)]

    def pin(self, predictor=None, plant=None):
        return self.lib.vine_mpc_observe_pin((plant or self.plant).h, (predictor or self.predictor).h, self.ocfg,
                                             *self._pin_args(predictor))

    def catchup(self, i, predictor=None):
        return self.lib.vine_mpc_observe_catchup(self.plant.h, (predictor or self.predictor).h, self.ocfg, int(i),
                                                 *self._pin_args(predictor))

    def state(self):
        return {"snap": self.snap.cpu().numpy(), "act_log": self.act_log.cpu().numpy(), "age": self.age.cpu().numpy(),
                "fresh": self.fresh.cpu().numpy()}

    def close(self):
        self.plant.close()
        self.predictor.close()


def _drive(rig, steps=STEPS, seed=3, each=None):
    """The plant stepped through random actions (beyond clipActions too) with the measurement behind every step.  Returns the
    plant's columns, progress and actions per step, and the controller state behind every measurement."""
    rng = np.random.default_rng(seed)
    acts = rng.uniform(-1.2, 1.2, (steps, rig.M, 2)).astype(np.float32)
    cols, progress, states = [], [], []
    for t in range(steps):
        rig.plant_actions.copy_(torch.as_tensor(acts[t]))
        rig.plant.step_t(rig.plant_actions, sync=False)
        rig.measure()
        torch.cuda.synchronize()
        assert rig.plant.step_count == t + 1
        cols.append(rig.plant.state_t.cpu().numpy())
        progress.append(rig.plant.progress_t.cpu().numpy())
        states.append(rig.state())
        if each is not None:
            each(t, cols, progress, states)
    return np.stack(cols), np.stack(progress), acts, states


# ------------------------------------------------------------------------------------------------------ the measurement
@pytest.mark.parametrize("M", [3, 257])
def test_measure_against_the_replay_and_the_tips_against_sysid_pin_and_float64(M):
    """Twelve plant steps, DELAY {0, 1, 3}, HOLD 0.3, both noises non-zero, the frame ring full of a sentinel and ``age`` of a
    wrong number.  Everything the launch writes against ``measure_replay`` in every bit; the tips a noisy frame derives are
    handed to the replay from the device (numpy does not reproduce float32 sincosf) and held to their own two checks: against
    the float64 kinematics within the recorder test's budget (tests/test_trajectory_gpu.py: POS_ULPS / VEL_ULPS ulps of the
    largest magnitude in the sums), and -- M = 3 -- against ``vine_sysid_pin`` fed the same q, qd, in every bit."""
    rig = Rig(M)
    try:
        cols, progress, acts, states = _drive(rig)
        table = rig.table_host
        step = {"t": 0}

        def device_tips(q, qd, plants):                      # the frame of step t stands in slot t mod SLOTS unless it was held
            t = step["t"]
            step["t"] += 1
            return states[t]["snap"][t % SLOTS][TIP][:, plants].T

        want = mpc_observe.measure_replay(table, SEED, np.arange(STEPS), cols, progress, acts, tip=device_tips,
                                          state={"snap": np.full((SLOTS, F.VF_COUNT, M), SENTINEL, np.float32),
                                                 "age": np.full(M, 5)})
        vc = rig.plant.cfg
        L, z1, phi0 = float(vc.link_length), float(vc.joint1_z), float(vc.phi0)
        noisy = np.flatnonzero((table[abi.VMO_NOISE_Q] != 0) | (table[abi.VMO_NOISE_QD] != 0))
        held_total, first_total, young, pinned_rows = 0, 0, 0, []
        for t in range(STEPS):
            w, got = want[t], states[t]
            assert np.all(got["snap"][:, RING] == SENTINEL), t              # a frame holds no delay ring
            stored = ~w["held"]                                              # (a held frame was formed but not stored)
            slot = got["snap"][t % SLOTS]
            # the noisy joint fields are numpy's own bits: one float32 multiply, one float32 add
            assert _same(slot[:12][:, stored], w["frame"][:12][:, stored]), t
            for k in ("age", "fresh", "act_log"):
                assert _same(got[k], w[k]), (t, k)
            assert _same(got["snap"][:, NOT_RING], w["snap"][:, NOT_RING]), t
            held_total += int(w["held"].sum())
            first_total += int(w["first"].sum())
            young += int((w["age"] < table[abi.VMO_DELAY]).sum())
            # the tips of the stored noisy frames against the float64 kinematics
            sel = noisy[stored[noisy]]
            q, qd = slot[F.VF_Q0:F.VF_Q0 + 6, sel].T.astype(np.float64), slot[F.VF_QD0:F.VF_QD0 + 6, sel].T.astype(np.float64)
            tip64, m_pos, m_vel = _fk64(q, qd, L, z1, phi0)
            tol = np.stack([POS_ULPS * _ulp32(m_pos)] * 2 + [VEL_ULPS * _ulp32(m_vel)] * 2, axis=1)
            assert np.all(np.abs(slot[TIP][:, sel].T.astype(np.float64) - tip64) <= tol), t
            assert not len(sel) or not np.array_equal(slot[:12][:, sel], cols[t][:12][:, sel])  # (the noise is there)
            quiet = np.setdiff1d(np.flatnonzero(stored), noisy)
            assert _same(slot[NOT_RING][:, quiet], cols[t][NOT_RING][:, quiet]), t              # a noise-free frame: the column's bits
            pinned_rows += [(t, p) for p in sel]
        assert first_total >= 2 * M and held_total >= M and young >= 1      # resets, held frames and young episodes occurred
        if M == 3:
            _tips_against_sysid_pin(rig, states, pinned_rows)
    finally:
        rig.close()


def _tips_against_sysid_pin(rig, states, rows):
    """``vine_sysid_pin`` on a log whose rows are the noisy joint states: the same q, qd, the same ``tip_fk_joint``."""
    lib, H = rig.lib, 1
    log = np.zeros((len(rows) + H + 1, abi.RECORD_FIELDS), dtype=np.float32)
    for r, (t, p) in enumerate(rows):
        log[r, F.VRF_Q0:F.VRF_Q0 + 12] = states[t]["snap"][t % SLOTS][:12, p]
    env = _env(_cfg(4), lane=True)
    try:
        log_t = torch.as_tensor(log, device=env.dev)
        scfg = sysid.sysid_config(lib, len(log), H)
        buf = [torch.zeros((4, 2), device=env.dev), torch.zeros(4, device=env.dev), torch.ones(4, dtype=torch.long, device=env.dev),
               torch.zeros(4, dtype=torch.long, device=env.dev), torch.zeros(2, dtype=torch.long, device=env.dev)]
        assert len(rows) >= 8
        for r, (t, p) in enumerate(rows):
            rc = lib.vine_sysid_pin(env.h, scfg, log_t.data_ptr(), r, *[b.data_ptr() for b in buf], _stream(env.dev))
            assert rc == abi.OK, lib.vine_last_error()
            torch.cuda.synchronize()
            st, frame = env.state_t.cpu().numpy()[:, 0], states[t]["snap"][t % SLOTS][:, p]
            for f in list(range(12)) + [F.VF_TIP_Y, F.VF_TIP_Z, F.VF_TIP_VY, F.VF_TIP_VZ, F.VF_CART_Y, F.VF_CART_VY, F.VF_PREV_TIP_Y,
                                        F.VF_PREV_TIP_Z, F.VF_PREV_CART_VEL] + list(range(F.VF_PREV_Q0, F.VF_PREV_Q0 + 6)):
                assert _same(st[f], frame[f]), (t, p, f)
    finally:
        env.close()


# --------------------------------------------------------------------------------------------- the pin and the catch-up node
@pytest.mark.parametrize("M", [3, 257])
def test_pin_and_catchup_against_the_replay(M):
    """Behind every one of twelve plant steps: the pin, then C = 3 x (a predictor step + the node), each against ``pin_replay``
    -- column, progress, reset, rew, lag and the next action in every bit; a lane that is not pinned keeps what its step left.
    The predictor has a table of its own with delays 0 .. 8; its rebuilt ring against what ``vine_mpc_fork`` rebuilds on a
    third handle from ``ring_history`` at the same step count.  Plants whose age < DELAY and plants with DELAY 0 are among
    them, and the catch-up schedule of every plant is ``catchup_schedule`` of its lag."""
    C, lib = 3, native.load()
    ptable = np.repeat(env_params.config_row(lib, _cfg(M))[:, None], M, axis=1)
    ptable[abi.VP_ACTION_DELAY] = np.arange(M) % 9
    ptable[abi.VP_RAIL_VELOCITY_SCALE] = 0.7 + 0.001 * np.arange(M)
    rig = Rig(M, C=C, predictor_table=ptable)
    ref = _env(_cfg(2 * M), np.repeat(ptable, 2, axis=1))
    seen = {"young": 0, "zero": 0, "lags": set()}
    try:
        mcfg = mpc.mpc_config(M, 2, 1, 0.05, [0.0, 0.0], SEED)
        d = rig.dev
        fork_buf = {"nominal": torch.zeros((M, 1, 2), device=d), "history": torch.zeros((M, F.MAX_DELAY, 2), device=d),
                    "tick": torch.zeros(M, dtype=torch.long, device=d), "actions": torch.zeros((2 * M, 2), device=d),
                    "cost": torch.zeros(2 * M, dtype=torch.float64, device=d), "alive": torch.zeros(2 * M, dtype=torch.uint8, device=d),
                    "window": torch.zeros(1, dtype=torch.long, device=d)}

        def check_ring(history):
            """The predictor's ring against the fork's from the same actions at the same step count."""
            fork_buf["history"].copy_(torch.as_tensor(np.ascontiguousarray(history)))
            ref.state_t[RING] = SENTINEL
            ref.step_count = rig.predictor.step_count
            b = fork_buf
            rc = lib.vine_mpc_fork(rig.plant.h, ref.h, mcfg, rig.plant.progress_t.data_ptr(), b["nominal"].data_ptr(),
                                   b["history"].data_ptr(), b["tick"].data_ptr(), b["actions"].data_ptr(), ref.rew_t.data_ptr(),
                                   ref.reset_t.data_ptr(), ref.progress_t.data_ptr(), b["cost"].data_ptr(), b["alive"].data_ptr(),
                                   b["window"].data_ptr(), _stream(d))
            assert rc == abi.OK, lib.vine_last_error()
            torch.cuda.synchronize()
            return ref.state_t[RING][:, ::2].cpu().numpy()

        def each(t, cols, progress, states):
            state, pred = states[-1], rig.predictor
            args = (rig.table_host, state, cols[-1], progress[-1], t + 1, C, True)
            pred.state_t[RING] = SENTINEL
            pred.reset_t.fill_(1)
            pred.rew_t.fill_(SENTINEL)
            rig.actions.fill_(SENTINEL)
            assert rig.pin() == abi.OK, lib.vine_last_error()
            torch.cuda.synchronize()
            want = mpc_observe.pin_replay(*args)
            st = pred.state_t.cpu().numpy()
            assert want["pinned"].all() and _same(st[NOT_RING], want["column"][NOT_RING]), t
            assert np.array_equal(pred.progress_t.cpu().numpy(), want["progress"]) and not pred.reset_t.any() and not pred.rew_t.any()
            assert np.array_equal(rig.lag.cpu().numpy(), want["lag"]) and _same(rig.actions.cpu().numpy(), want["actions"]), t
            ring = check_ring(want["ring_history"])
            assert _same(st[RING], ring) and (ring != SENTINEL).any(), t
            delay = rig.table_host[abi.VMO_DELAY].astype(np.int64)
            expect = np.minimum(delay, np.minimum(state["age"], F.MAX_DELAY))
            assert np.array_equal(want["lag"], expect), t
            seen["young"] += int((state["age"] < delay).sum())
            seen["zero"] += int((delay == 0).sum())
            seen["lags"] |= set(int(x) for x in want["lag"])
            schedules = [mpc_observe.catchup_schedule(C, int(x)) for x in want["lag"]]
            for i in range(1, C + 1):
                pred.step_t(rig.actions, sync=False)
                torch.cuda.synchronize()
                before, act_before = pred.state_t.cpu().numpy(), rig.actions.cpu().numpy()
                prog_before = pred.progress_t.cpu().numpy()
                pred.reset_t.fill_(1)
                assert rig.catchup(i) == abi.OK, lib.vine_last_error()
                torch.cuda.synchronize()
                want = mpc_observe.pin_replay(*args, step_index=i)
                pinned = want["pinned"]
                assert np.array_equal(pinned, [s[i]["pinned"] for s in schedules]), (t, i)
                st = pred.state_t.cpu().numpy()
                assert _same(st[NOT_RING][:, pinned], want["column"][NOT_RING][:, pinned]), (t, i)
                assert _same(st[:, ~pinned], before[:, ~pinned]), (t, i)                # a real step: the state stands
                assert np.array_equal(pred.progress_t.cpu().numpy()[pinned], want["progress"][pinned])
                assert np.array_equal(pred.progress_t.cpu().numpy()[~pinned], prog_before[~pinned])
                assert not pred.reset_t.any(), (t, i)
                ring = check_ring(want["ring_history"])
                rebuilt = (np.arange(2 * F.MAX_DELAY)[:, None] // 2 < ptable[abi.VP_ACTION_DELAY][None, :]) & pinned[None, :]
                assert _same(st[RING][rebuilt], ring[rebuilt]), (t, i)                       # slots 0 .. a - 1 of the pinned
                assert _same(rig.actions.cpu().numpy(), want["actions"] if want["writes_action"] else act_before), (t, i)
                for p in (0, 1, 2):                                                      # the schedule names the log's entry
                    a = schedules[p][i]["action"]
                    if a != "none":
                        assert _same(rig.actions.cpu().numpy()[p], state["act_log"][p, a] if a is not None else np.zeros(2, np.float32))

        _drive(rig, each=each)
        assert seen["young"] >= 1 and seen["zero"] >= 1 and {0, 1, 3} <= seen["lags"]
    finally:
        ref.close()
        rig.close()


def test_pin_refusals_name_the_reason():
    M = 3
    rig = Rig(M)
    lib, others = rig.lib, []
    try:
        def other(cfg):
            others.append(_env(cfg))
            return others[-1]

        def refused(rc, code, word, whole=False):
            assert rc == code and (lib.vine_last_error() == word if whole else word in lib.vine_last_error()), (rc, lib.vine_last_error())

        refused(rig.pin(predictor=other(_cfg(M + 1))), abi.ERR_INVALID_ARG, b"the predictor handle has 4 envs, not num_plants = 3")
        refused(rig.catchup(1, predictor=others[-1]), abi.ERR_INVALID_ARG, b"the predictor handle has 4 envs")
        refused(rig.pin(plant=others[-1]), abi.ERR_INVALID_ARG, b"the plant handle does not have num_plants envs")
        cfg = _cfg(M)
        cfg.set_flag(abi.FLAG_VINE_RANDOMIZE, True)
        refused(rig.pin(predictor=other(cfg)), abi.ERR_UNSUPPORTED, b"mpc observe: a predictor handle with vine_randomize is refused "
                b"(a replayed step must be a deterministic one)", whole=True)
        refused(rig.pin(predictor=other(_cfg(M, pipe=True))), abi.ERR_UNSUPPORTED,
                b"mpc observe: the predictor handle's CREATE_SHELF / CREATE_PIPE differ from the plant's", whole=True)
        cfg = _cfg(M)
        cfg.max_episode_length = 9
        refused(rig.pin(predictor=other(cfg)), abi.ERR_INVALID_ARG,
                b"mpc observe: the predictor handle's max_episode_length differs from the plant's", whole=True)
        if torch.cuda.device_count() > 1:
            from tests.hip_env import HipEnv
            others.append(HipEnv(_cfg(M), device_id=1))
            refused(rig.pin(predictor=others[-1]), abi.ERR_INVALID_ARG, b"another device")
        assert rig.pin() == abi.OK
        torch.cuda.synchronize()
        with pytest.raises(mpc_observe.ConfigError, match="below the table's largest DELAY"):
            mpc_observe.observe_cconfig(M, 2, True, 0, rig.table_host)
    finally:
        for o in others:
            o.close()
        rig.close()


# ------------------------------------------------------------------------------------------------------ the task classes
def _plant_cfg(M, pipe=False, seed=9, **env_over):
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % M])
    cfg["seed"] = seed
    cfg["task"]["vine_randomize"] = False
    cfg["env"].update(CREATE_PIPE=pipe, CREATE_SHELF=False, maxEpisodeLength=8)
    cfg["env"].update(env_over)
    return cfg


class Tasks:
    """A plant, its model and predictor tasks and the observing controller; ``plain``: also an identically seeded plant with a
    plain ``Controller``."""

    def __init__(self, M, observe, pipe=False, plain=False, K=2, H=2, **ctl):
        cfg = _plant_cfg(M, pipe)
        self.all = []
        make = lambda c: self.all.append(mpc.make_task(c)) or self.all[-1]          # noqa: E731
        # cost={}: the model keeps the plant's own reward weights -- an exact model, VF_AGG_REW included
        self.plant, self.model = make(cfg), make(mpc.model_config(cfg, M, K, cost={}))
        self.predictor = make(mpc.model_config(cfg, M, 1, cost={}))
        self.ctl = mpc_observe.ObservingController(self.plant, self.model, self.predictor, K, observe, H, seed=5, **ctl)
        if plain:
            self.plant2, self.model2 = make(cfg), make(mpc.model_config(cfg, M, K, cost={}))
            self.ctl2 = mpc.Controller(self.plant2, self.model2, K, H, seed=5, **ctl)

    def close(self):
        for t in reversed(self.all):
            t.close()


@pytest.mark.parametrize("M, d, pipe", [(3, 0, False), (3, 1, False), (3, 3, False), (3, 0, True), (3, 1, True), (3, 3, True),
                                        (257, 3, False), (257, 3, True)])
def test_an_exact_model_catches_up_with_its_plant_in_every_bit(M, d, pipe):
    """Exact model, no randomisation, HOLD 0, zero noise, a common DELAY d with C = 3.  After the catch-up of every one of
    twelve control steps each predictor column equals its plant's current column in every bit, on every field but the ring;
    ``plant_actions`` and ``nominal`` equal those of a plain ``Controller`` driving an identically seeded plant; and
    ``act_log[:, :MAX_DELAY]`` equals ``history`` after every control step."""
    T = Tasks(M, {"DELAY": d, "CATCHUP": 3}, pipe=pipe, plain=True, graph=False)
    try:
        ctl, ctl2 = T.ctl, T.ctl2
        assert ctl.C == 3 and not ctl.use_graph
        lags, resets = set(), 0
        for t in range(STEPS):
            ctl.predict()
            torch.cuda.synchronize()
            pst, st = T.plant.state.cpu().numpy(), T.predictor.state.cpu().numpy()
            assert _same(st[NOT_RING], pst[NOT_RING]), (t, [f for f in NOT_RING if not _same(st[f], pst[f])])
            assert np.array_equal(T.predictor.progress_buf.cpu().numpy(), T.plant.progress_buf.cpu().numpy()), t
            lags |= set(int(x) for x in ctl.lag.cpu().numpy())
            resets += int(T.plant.reset_buf.sum())
            mpc.Controller.control_step(ctl)
            ctl.measure()
            ctl2.control_step()
            torch.cuda.synchronize()
            assert _same(ctl.plant_actions.cpu().numpy(), ctl2.plant_actions.cpu().numpy()), t
            assert _same(ctl.nominal.cpu().numpy(), ctl2.nominal.cpu().numpy()), t
            assert _same(ctl.act_log[:, :F.MAX_DELAY].cpu().numpy(), ctl.history.cpu().numpy()), t
            assert _same(T.plant.state.cpu().numpy(), T.plant2.state.cpu().numpy()), t
        assert lags == set(range(d + 1)) and resets >= M                 # young episodes and resets were among them
        assert np.abs(ctl.nominal.cpu().numpy()).max() > 0               # (the nominal moved)
        assert ctl.launches["pin"] == STEPS and ctl.launches["catchup"] == ctl.launches["predictor_step"] == 3 * STEPS
        assert ctl.launches["measure"] == ctl.launches["fork"] == STEPS
    finally:
        T.close()


@pytest.mark.parametrize("M", [3, 257])
def test_without_compensation_the_stale_frame_is_planned_from(M):
    """COMPENSATE False, DELAY 3: behind the pin the predictor column is the plant's column of min(3, age) steps earlier
    (host-side copies), and the lag is 0.  Before the plant's first step it is the plant's own column."""
    T = Tasks(M, {"DELAY": 3, "COMPENSATE": False}, graph=False)
    try:
        ctl = T.ctl
        assert ctl.C == 3 and ctl.ocfg.compensate == 0
        past, stale = [], 0
        for t in range(STEPS):
            age, fresh = ctl.age.cpu().numpy(), ctl.fresh.cpu().numpy()
            ctl.predict()
            torch.cuda.synchronize()
            st = T.predictor.state.cpu().numpy()
            back = np.where(fresh != 0, 0, np.minimum(3, age))
            now = T.plant.state.cpu().numpy()
            for b in range(4):
                sel = back == b
                if not sel.any():
                    continue
                want = now if (b == 0 or not past) else past[-1 - b]
                assert _same(st[NOT_RING][:, sel], want[NOT_RING][:, sel]), (t, b)
            stale += int((back == 3).sum())
            assert not ctl.lag.any()
            assert np.array_equal(T.predictor.progress_buf.cpu().numpy(), T.plant.progress_buf.cpu().numpy() - back)
            mpc.Controller.control_step(ctl)
            ctl.measure()
            torch.cuda.synchronize()
            past.append(T.plant.state.cpu().numpy())
        assert stale >= 2 * M
    finally:
        T.close()


@pytest.mark.parametrize("C", [0, 3])
def test_captured_control_steps_against_eager_ones(C):
    """Two captured control steps replayed three times against six eager ones: every controller tensor and all three state
    blocks bit-identical.  C = 3: DELAY {0, 1, 3}, HOLD 0.3 and both noises; C = 0: no delay, the rest the same."""
    M = 3
    observe = {"DELAY": {"values": [0, 1, 3]} if C else 0, "HOLD": 0.3, "NOISE_Q": 0.002, "NOISE_QD": 0.01}
    runs = []
    for tag, kw in (("graph", dict(graph=True, graph_steps=2)), ("eager", dict(graph=False))):
        T = Tasks(M, observe, **kw)
        try:
            ctl = T.ctl
            assert ctl.use_graph == (tag == "graph") and ctl.C == C
            ctl.run(6)
            torch.cuda.synchronize()
            counts = {"fork": 6, "step": 12, "node": 12, "update": 6, "plant_step": 6, "pin": 6, "catchup": 6 * C,
                      "predictor_step": 6 * C, "measure": 6}
            if tag == "graph":
                assert ctl.graph_launches == {k: v // 3 for k, v in counts.items()}
            assert ctl.launches == counts
            assert (T.plant.step_count, T.model.step_count, T.predictor.step_count) == (6, 12, 6 * C)
            assert (T.plant.num_steps, T.model.num_steps, T.predictor.num_steps) == (6, 12, 6 * C)
            runs.append(([t.cpu().numpy().copy() for t in ctl.tensors()],
                         [t.state.cpu().numpy().copy() for t in (T.plant, T.model, T.predictor)]))
        finally:
            T.close()
    (ta, sa), (tb, sb) = runs
    for a, b in zip(ta + sa, tb + sb):
        assert _same(a, b)
    assert np.abs(ta[0]).max() > 0                                          # (the nominal moved)


def test_the_command_line_with_observe(tmp_path):
    """``mpc.py``'s main with ``observe=``: runs from the graph, reports the table and the mean lag; with a wrong model
    (``model_params=``) the predictor has the per-plant draw in its table, not repeated."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mpc_cli", os.path.join(REPO, "mpc.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    H = 4
    argv = ["plants=4", "samples=16", "horizon=%d" % H, "steps=12", "sigma=[0.5, 0.25]", "lambda=0.1", "out=%s" % tmp_path,
            "task.env.EPISODE_LOG=True", "task.env.maxEpisodeLength=8", "task.env.CREATE_PIPE=False",
            "task.task.vine_randomize=False", "seed=3", "observe={DELAY: {values: [1, 3]}, HOLD: 0.1, NOISE_Q: 0.002}"]
    out = cli.main(argv)
    assert out["graphed"] and np.isfinite(out["plant_return"]).all() and out["report"]["episodes"] >= 4
    assert out["launches"] == {"fork": 12, "step": 12 * H, "node": 12 * H, "update": 12, "plant_step": 12, "pin": 12,
                               "catchup": 36, "predictor_step": 36, "measure": 12}
    ob = out["observe"]
    assert ob["names"] == ["DELAY", "HOLD", "NOISE_Q", "NOISE_QD"] and ob["table"].shape == (4, 4) and ob["catchup"] == 3
    assert list(ob["table"][0]) == [1, 3, 1, 3] and ob["compensate"] and 0 <= ob["lag"] <= 2.0
    out2 = cli.main(argv + ["model_params={DAMPING: [0.01, 0.05]}", "steps=4"])
    assert out2["model_table_bound"] and np.isfinite(out2["plant_return"]).all() and out2["observe"]["catchup"] == 3
    out3 = cli.main(argv[:-1] + ["observe={DELAY: 3, COMPENSATE: False}", "steps=4"])
    assert out3["observe"]["lag"] == 0.0 and not out3["observe"]["compensate"]


def test_set_model_params_reaches_the_predictor_not_repeated():
    M, K = 3, 2
    cfg = _plant_cfg(M)
    mcfg, pcfg = mpc.model_config(cfg, M, K), mpc.model_config(cfg, M, 1)
    mcfg["env"]["ENV_PARAMS"] = pcfg["env"]["ENV_PARAMS"] = {"DAMPING": [0.01, 0.05]}
    tasks = [mpc.make_task(c) for c in (cfg, mcfg, pcfg)]
    try:
        ctl = mpc_observe.ObservingController(*tasks, K, {"DELAY": 1}, 2, graph=False)
        ctl.set_model_params({"DAMPING": np.array([0.01, 0.02, 0.03])})
        assert _same(tasks[1].env_params.cpu().numpy()[abi.VP_DAMPING], np.repeat(np.float32([0.01, 0.02, 0.03]), K))
        assert _same(tasks[2].env_params.cpu().numpy()[abi.VP_DAMPING], np.float32([0.01, 0.02, 0.03]))
        ctl.run(2)
        ctl.act_log.fill_(0.5)
        ctl.reset_plants([1])
        torch.cuda.synchronize()
        assert not ctl.act_log[1].any() and ctl.act_log[0].all() and list(ctl.fresh.cpu().numpy()) == [0, 1, 0]
        with pytest.raises(mpc_observe.ConfigError, match="the predictor task has 6 envs"):
            mpc_observe.ObservingController(tasks[0], tasks[1], tasks[1], K, {"DELAY": 1}, 2, graph=False)
    finally:
        for t in reversed(tasks):
            t.close()


def test_without_observe_nothing_changes():
    """``play`` without ``observe=``: the summed plant reward and the launch counts of tests/golden/mpc_play_no_adapt.json
    (recorded before MPC_ADAPT with the same call), bit for bit."""
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
        assert "observe" not in out
