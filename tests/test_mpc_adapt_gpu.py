"""MPC_ADAPT on the GPU (include/vine_mpc_adapt.h, utils/mpc_adapt.py): the anchor and the trace field by field; the pin's
table rows against ``candidates``, its copy against the anchor and its ring against the step kernel's own; exact recovery
(candidates that ARE the plant score 0.0); the score's sums and the estimate against numpy; the captured cycle against eager
launches; ``play`` without ``adapt`` against bits recorded before this feature existed; and the belief moving to the truth.

Shapes (M plants, K samples, W window, D dimensions): (5, 14, 6, 2) = 70 model envs, several plants in a wave; (2, 300, 3, 1)
= K above one workgroup of the estimate and no multiple of 256; (1, 2, 1, 1) every extent at its minimum.  Both handles carry
a parameter table, so both run the one-lane step kernel.  "Bit-identical" is literal: floats are compared as words."""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import base_cfg
from vine_robot_isaacgymenvs_amd import abi, load_task_config, native
from vine_robot_isaacgymenvs_amd.utils import env_params, mpc, mpc_adapt

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _nothing_left_for_a_later_capture():
    """The tasks of a test are reference cycles (a task and its observers), and so is the frame of a test that caught an
    exception; with their tensors and graphs they would otherwise wait for whichever collection comes next -- possibly on
    the autograd thread in the middle of a later test's graph capture.  They go here, where nothing is being captured."""
    yield
    import gc
    gc.collect()

F = abi
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7777.0
RING = slice(F.VF_FIFO0, F.VF_FIFO0 + 2 * F.MAX_DELAY)
NOT_RING = [f for f in range(F.VF_COUNT) if not F.VF_FIFO0 <= f < F.VF_FIFO0 + 2 * F.MAX_DELAY]
JOINTS = slice(F.VF_Q0, F.VF_Q0 + 12)
SHAPES = [(5, 14, 6, 2), (2, 300, 3, 1), (1, 2, 1, 1)]
PARAMS = {1: {"DAMPING": [0.005, 0.1]}, 2: {"DAMPING": [0.005, 0.1], "FPAM_K": [0.7, 1.3]}}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)))


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _cfg(n, pipe=False, **over):
    cfg = base_cfg(n, 0, False, max_episode_length=100, action_delay=1, **over)
    for f in (abi.FLAG_USE_TARGET_REACHED_RESET, abi.FLAG_USE_TIP_LIMIT_HIT_RESET, abi.FLAG_USE_NONZERO_CONTACT_FORCE_RESET,
              abi.FLAG_CREATE_SHELF, abi.FLAG_CREATE_PIPE):
        cfg.set_flag(f, False)
    cfg.set_flag(abi.FLAG_CREATE_PIPE, pipe)
    return cfg


def _env(cfg, table=None):
    from tests.hip_env import HipEnv
    env = HipEnv(cfg)
    if table is not None:
        env_params.check_table(env.lib, env.cfg, table)
        env.table_t = torch.as_tensor(np.ascontiguousarray(table, np.float32)).to(env.dev).contiguous()
        torch.cuda.synchronize(env.dev)
        native.check(env.lib.vine_bind_env_params(env.h, env.table_t.data_ptr()), env.lib)
    return env


def _plant_values(M):
    """The plants' own DAMPING and FPAM_K factor, spread over the ranges of PARAMS."""
    return np.linspace(0.01, 0.09, M) if M > 1 else np.array([0.04]), np.linspace(0.8, 1.2, M) if M > 1 else np.array([1.1])


def _tables(M, K, pipe=False, D=2):
    """``(base_row, plant_table [VP_COUNT, M], model_table [VP_COUNT, M * K], truth [M, 2])``: the plants differ in DAMPING and
    (where it is a dimension, D = 2) in FPAM_K; the model holds the configuration's row in every column."""
    lib = native.load()
    base = env_params.config_row(lib, _cfg(M, pipe))
    plant = np.repeat(base[:, None], M, axis=1)
    damping, factor = _plant_values(M)
    env_params.set_rows(plant, base, "DAMPING", damping)
    if D == 2:
        env_params.set_rows(plant, base, "FPAM_K", factor)
    truth = np.stack([plant[abi.VP_DAMPING].astype(np.float64), factor], axis=1)      # (the damping the float32 row holds)
    return base, plant, np.repeat(base[:, None], M * K, axis=1), truth


class Rig:
    """A plant and a model handle through the C ABI, both with a table bound, and the adaptation's buffers full of sentinels."""

    def __init__(self, M, K, W, D, pipe=False, every=None, model_table=None, seed=77, **spec):
        self.M, self.K, self.W, self.D, self.N = M, K, W, D, M * K
        self.lib = native.load()
        self.base, plant_table, table, self.truth = _tables(M, K, pipe, D)
        self.plant = _env(_cfg(M, pipe), plant_table)
        self.model = _env(_cfg(M * K, pipe), table if model_table is None else model_table)
        d = self.dev = self.plant.dev
        full = dict(params=PARAMS[D], window=W, every=W if every is None else every)
        full.update(spec)
        self.seed = seed
        self.acfg, self.names = mpc_adapt.adapt_config(full, M, K, self.base, seed)
        self.dims = mpc_adapt.dims_of(self.acfg)
        f32, f64, i64, u8 = torch.float32, torch.float64, torch.int64, torch.uint8
        self.history = torch.zeros((M, F.MAX_DELAY, 2), device=d)
        self.plant_actions = torch.zeros((M, 2), device=d)
        self.mean = torch.zeros((M, D), dtype=f64, device=d)
        self.std = torch.zeros((M, D), dtype=f64, device=d)
        self.prior_mean = torch.full((M, D), 0.5, dtype=f64, device=d)
        self.prior_std = torch.full((M, D), 0.25, dtype=f64, device=d)
        self.passes = torch.zeros(M, dtype=i64, device=d)
        self.anchor_state = torch.full((F.VF_COUNT, M), SENTINEL, dtype=f32, device=d)
        self.anchor_history = torch.full((M, F.MAX_DELAY, 2), SENTINEL, dtype=f32, device=d)
        self.anchor_progress = torch.full((M,), -5, dtype=i64, device=d)
        self.anchor_count = torch.full((1,), -99, dtype=i64, device=d)
        self.trace_actions = torch.full((M, W, 2), SENTINEL, dtype=f32, device=d)
        self.trace_rows = torch.full((M, W, 12), SENTINEL, dtype=f32, device=d)
        self.trace_len = torch.full((M,), 77, dtype=torch.int32, device=d)
        self.trace_open = torch.full((M,), 9, dtype=u8, device=d)
        self.episode_ended = torch.full((M,), 9, dtype=u8, device=d)
        self.err = torch.full((self.N,), SENTINEL, dtype=f64, device=d)
        self.alive = torch.full((self.N,), 9, dtype=u8, device=d)
        self.window = torch.full((1,), -99, dtype=i64, device=d)
        self.actions = torch.full((self.N, 2), SENTINEL, device=d)
        self.returns = torch.zeros(M, dtype=f64, device=d)
        self.weights = torch.full((self.N,), SENTINEL, dtype=f64, device=d)

    def warm_plant(self, steps=10, seed=3, scale=0.8):
        """The plant stepped through ``steps`` random actions, the last eight into the history, most recent first.  The rail
        component is never positive: a reset leaves the cart at y = 0.215 of a limit of 0.3, and a random walk from there
        reaches the limit within a dozen steps now and then; this way the cart moves inward and only a planted run does."""
        rng = np.random.default_rng(seed)
        acts = rng.uniform(-scale, scale, (steps, self.M, 2)).astype(np.float32)
        acts[:, :, 0] = -np.abs(acts[:, :, 0])
        for a in acts:
            self.plant.step(a, sync=False)
        torch.cuda.synchronize()
        self.history.copy_(torch.as_tensor(np.ascontiguousarray(acts[::-1][:F.MAX_DELAY].transpose(1, 0, 2))))
        return acts

    def plant_step(self, action):
        """One plant step on ``action`` [M, 2] as the controller does it: the action enters plant_actions and the history."""
        a = torch.as_tensor(np.asarray(action, np.float32)).to(self.dev)
        self.plant_actions.copy_(a)
        self.history.copy_(torch.cat([a[:, None], self.history[:, :-1]], dim=1))
        self.plant.step_t(self.plant_actions, sync=False)

    def believe_the_truth(self, std=(0.01, 0.05)):
        self.mean.copy_(torch.as_tensor(self.truth[:, :self.D]))
        self.std.copy_(torch.as_tensor(np.broadcast_to(np.asarray(std[:self.D], dtype=np.float64), (self.M, self.D)).copy()))

    def theta(self):
        return mpc_adapt.candidates(self.mean.cpu().numpy(), self.std.cpu().numpy(), self.dims, self.seed, self.K,
                                    self.passes.cpu().numpy())

    def anchor(self, acfg=None):
        p = self.plant
        return self.lib.vine_mpc_adapt_anchor(
            p.h, acfg or self.acfg, p.progress_t.data_ptr(), p.reset_t.data_ptr(), self.history.data_ptr(),
            self.anchor_state.data_ptr(), self.anchor_history.data_ptr(), self.anchor_progress.data_ptr(),
            self.anchor_count.data_ptr(), self.trace_len.data_ptr(), self.trace_open.data_ptr(), self.episode_ended.data_ptr(),
            _stream(self.dev))

    def trace(self, acfg=None):
        p = self.plant
        return self.lib.vine_mpc_adapt_trace(
            p.h, acfg or self.acfg, self.plant_actions.data_ptr(), p.reset_t.data_ptr(), p.rew_t.data_ptr(),
            self.anchor_count.data_ptr(), self.trace_actions.data_ptr(), self.trace_rows.data_ptr(), self.trace_len.data_ptr(),
            self.trace_open.data_ptr(), self.episode_ended.data_ptr(), self.returns.data_ptr(), _stream(self.dev))

    def pin(self, model=None, acfg=None):
        m = model or self.model
        return self.lib.vine_mpc_adapt_pin(
            m.h, acfg or self.acfg, self.mean.data_ptr(), self.std.data_ptr(), self.passes.data_ptr(),
            self.anchor_state.data_ptr(), self.anchor_history.data_ptr(), self.anchor_progress.data_ptr(),
            self.trace_actions.data_ptr(), self.actions.data_ptr(), m.rew_t.data_ptr(), m.reset_t.data_ptr(),
            m.progress_t.data_ptr(), self.err.data_ptr(), self.alive.data_ptr(), self.window.data_ptr(), _stream(self.dev))

    def score(self, model=None, acfg=None):
        m = model or self.model
        return self.lib.vine_mpc_adapt_scheduled(
            m.h, acfg or self.acfg, self.trace_actions.data_ptr(), self.trace_rows.data_ptr(), self.trace_len.data_ptr(),
            self.window.data_ptr(), self.actions.data_ptr(), m.reset_t.data_ptr(), self.err.data_ptr(), self.alive.data_ptr(),
            _stream(self.dev))

    def estimate(self, model=None, acfg=None):
        m = model or self.model
        return self.lib.vine_mpc_adapt_estimate(
            m.h, acfg or self.acfg, self.err.data_ptr(), self.trace_len.data_ptr(), self.episode_ended.data_ptr(),
            self.mean.data_ptr(), self.std.data_ptr(), self.prior_mean.data_ptr(), self.prior_std.data_ptr(),
            self.passes.data_ptr(), self.weights.data_ptr(), _stream(self.dev))

    def ok(self, rc):
        assert rc == abi.OK, self.lib.vine_last_error()

    def run_away(self, env, e):
        """Past RAIL_SOFT_LIMIT: the next step of env ``e`` raises its reset."""
        y = float(env.cfg.rail_soft_limit) + 0.05
        for f in (F.VF_Q0, F.VF_CART_Y, F.VF_PREV_Q0):
            env.state_t[f, e] = y

    def traced_window(self, steps=None, seed=21, runaway=None, toward_limit=None, pending=None, scale=0.7):
        """anchor, then ``steps`` (default W) x (plant step on a random action + trace node), with host snapshots behind every
        step.  ``runaway = (plant, s)``: that plant is put past the rail limit in front of step s (its samples, pinned at the
        anchor, do not follow it there).  ``toward_limit``: a plant put 5 cm inside the rail limit IN FRONT OF the anchor and
        driven at it with rail action +1, so that it crosses two to four steps later (1 m/s at most, 8 m/s^2, 33 ms a step)
        and its samples can cross with it.  ``pending``: a plant whose reset flag is raised at the anchor."""
        steps = self.W if steps is None else steps
        if pending is not None:
            self.plant.reset_t[pending] = 1
        if toward_limit is not None:
            y = float(self.plant.cfg.rail_soft_limit) - 0.05
            for f in (F.VF_Q0, F.VF_CART_Y, F.VF_PREV_Q0):
                self.plant.state_t[f, toward_limit] = y
        snap = {"state": self.plant.state_t.cpu().numpy().copy(), "history": self.history.cpu().numpy().copy(),
                "progress": self.plant.progress_t.cpu().numpy().copy(), "count": self.plant.step_count,
                "reset": self.plant.reset_t.cpu().numpy().copy(), "rows": [], "actions": [], "resets": [], "rews": []}
        self.ok(self.anchor())
        acts = np.random.default_rng(seed).uniform(-scale, scale, (steps, self.M, 2)).astype(np.float32)
        acts[:, :, 0] *= 0.5                                                   # (the carts stay where the warm-up left them)
        if toward_limit is not None:
            acts[:, toward_limit, 0] = 1.0
        for s in range(1, steps + 1):
            if runaway is not None and runaway[1] == s:
                self.run_away(self.plant, runaway[0])
            self.plant_step(acts[s - 1])
            self.ok(self.trace())
            torch.cuda.synchronize()
            snap["rows"].append(self.plant.state_t[JOINTS].cpu().numpy().T.copy())
            snap["actions"].append(acts[s - 1])
            snap["resets"].append(self.plant.reset_t.cpu().numpy().copy())
            snap["rews"].append(self.plant.rew_t.cpu().numpy().copy())
        return snap

    def replay(self, plant_nan=None, runaway=None):
        """pin, then W x (model step + score node) with snapshots of the twelve joint fields, the reset words and err behind
        every step.  ``runaway``: a model env put past the rail limit behind the pin.  ``plant_nan = (k, env)``: a NaN in that
        env's q2 while the score node of step k runs (taken out again before the next step)."""
        self.model.step_count = 7
        self.ok(self.pin())
        if runaway is not None:
            self.run_away(self.model, runaway)
        states, resets, errs = [], [], []
        for k in range(1, self.W + 1):
            self.model.step_t(self.actions, sync=False)
            kept = None
            if plant_nan is not None and plant_nan[0] == k:
                kept = self.model.state_t[F.VF_Q0 + 2, plant_nan[1]].clone()
                self.model.state_t[F.VF_Q0 + 2, plant_nan[1]] = float("nan")
            states.append(self.model.state_t[JOINTS].cpu().numpy().copy())
            resets.append(self.model.reset_t.cpu().numpy().copy())
            self.ok(self.score())
            if kept is not None:
                self.model.state_t[F.VF_Q0 + 2, plant_nan[1]] = kept
            torch.cuda.synchronize()
            errs.append(self.err.cpu().numpy().copy())
        return np.stack(states), np.stack(resets), errs

    def close(self):
        self.plant.close()
        self.model.close()


# ------------------------------------------------------------------------------------------------- the anchor and the trace
def test_anchor_and_trace_field_by_field():
    """(5, 14, 6, 2), E = 8.  Plant 1 has its reset raised at the anchor: not traced.  Plant 3 runs past the rail limit in step 3:
    that row is stored, the trace closes, episode_ended is set.  The two steps behind the window are not traced."""
    M, K, W, D = SHAPES[0]
    rig = Rig(M, K, W, D, every=8)
    try:
        rig.warm_plant(10)
        snap = rig.traced_window(steps=8, runaway=(3, 3), pending=1)
        assert _same(rig.anchor_state.cpu().numpy(), snap["state"])
        assert _same(rig.anchor_history.cpu().numpy(), snap["history"])
        assert np.array_equal(rig.anchor_progress.cpu().numpy(), snap["progress"])
        assert int(rig.anchor_count[0]) == snap["count"] == 10 and rig.plant.step_count == 18
        resets = np.stack(snap["resets"])
        assert resets[2, 3] == 1 and not np.delete(resets, 3, axis=1).any()        # (only the planted run raised a reset)
        want_len = np.array([W, 0, W, 3, W])
        assert np.array_equal(rig.trace_len.cpu().numpy(), want_len) and rig.trace_len.dtype == torch.int32
        assert np.array_equal(rig.trace_open.cpu().numpy(), [1, 0, 1, 0, 1])
        assert np.array_equal(rig.episode_ended.cpu().numpy(), [0, 0, 0, 1, 0])
        rows, acts = rig.trace_rows.cpu().numpy(), rig.trace_actions.cpu().numpy()
        for p in range(M):
            for s in range(W):
                if s < want_len[p]:
                    assert _same(rows[p, s], snap["rows"][s][p]) and _same(acts[p, s], snap["actions"][s][p]), (p, s)
                else:
                    assert np.all(rows[p, s] == np.float32(SENTINEL)) and np.all(acts[p, s] == np.float32(SENTINEL)), (p, s)
        # the optional sum of the plant's reward: float64 += float32 per step, as play() sums it on the host
        total = np.zeros(M)
        for r in snap["rews"]:
            total += r
        assert _same(rig.returns.cpu().numpy(), total)
        # a second anchor starts the next cycle: lengths and flags anew, the rows stay until they are overwritten
        rig.ok(rig.anchor())
        torch.cuda.synchronize()
        assert not rig.trace_len.any() and not rig.episode_ended.any() and int(rig.anchor_count[0]) == 18
        assert np.array_equal(rig.trace_open.cpu().numpy(), (rig.plant.reset_t.cpu().numpy() == 0).astype(np.uint8))
        assert _same(rig.trace_rows.cpu().numpy(), rows)
        # a trace node in front of the cycle's first step (s = 0) touches nothing
        rig.ok(rig.trace())
        torch.cuda.synchronize()
        assert not rig.trace_len.any() and _same(rig.returns.cpu().numpy(), total)
    finally:
        rig.close()


@pytest.mark.parametrize("shape", SHAPES[1:], ids=["2x300x3x1", "1x2x1x1"])
def test_anchor_and_trace_at_the_other_shapes(shape):
    M, K, W, D = shape
    rig = Rig(M, K, W, D)
    try:
        rig.warm_plant(9, seed=M + K)
        snap = rig.traced_window()
        assert _same(rig.anchor_state.cpu().numpy(), snap["state"]) and int(rig.anchor_count[0]) == 9
        assert np.array_equal(rig.trace_len.cpu().numpy(), [W] * M) and not rig.episode_ended.any() and rig.trace_open.all()
        assert _same(rig.trace_rows.cpu().numpy(), np.stack(snap["rows"], axis=1))
        assert _same(rig.trace_actions.cpu().numpy(), np.stack(snap["actions"], axis=1))
    finally:
        rig.close()


def test_refusals_that_need_a_handle():
    M, K, W, D = 2, 4, 3, 1
    rig = Rig(M, K, W, D)
    bare = _env(_cfg(M * K))                                                   # no table bound
    other = _env(_cfg(M * K + 1), np.repeat(rig.base[:, None], M * K + 1, axis=1))
    try:
        lib = rig.lib
        for fn in (rig.pin, rig.score, rig.estimate):
            lib.vine_set_step_count(None, -1)
            assert fn(model=bare) == abi.ERR_UNSUPPORTED and b"no per-env parameter table bound" in lib.vine_last_error()
            assert fn(model=other) == abi.ERR_INVALID_ARG and b"num_plants * samples" in lib.vine_last_error()
        wrong, _ = mpc_adapt.adapt_config(dict(params=PARAMS[1], window=W), M + 1, K, rig.base)
        for fn in (rig.anchor, rig.trace):
            assert fn(acfg=wrong) == abi.ERR_INVALID_ARG and b"num_plants envs" in lib.vine_last_error()
        for fn in (rig.anchor, rig.trace, rig.pin, rig.score, rig.estimate):
            rig.ok(fn())
        torch.cuda.synchronize()
    finally:
        rig.close()
        bare.close()
        other.close()


# ---------------------------------------------------------------------------------------------------------------- the pin
def test_pin_rows_copy_and_the_ring_against_the_step_kernels_own():
    """(5, 14, 6, 2) with RAIL_VELOCITY_SCALE and FPAM_K as the dimensions: the ring's commands depend on the lane's OWN
    candidate of the first, which the pin must read behind its write.  Model delays 0..8 inside one wave through the table;
    the model's block full of a sentinel, its step count at 5 while the plant's is 10.  A reference handle bound to the table
    the pin left steps through the plant's last eight actions and ends at step count 16: its slot (16 - k) mod d holds the
    command of the action handed k steps ago, and the pinned handle must hold the same words in slot (5 - k) mod d."""
    M, K, W, D = SHAPES[0]
    N = M * K
    base, _, table, _ = _tables(M, K)
    delays = np.arange(N) % 9
    table[abi.VP_ACTION_DELAY] = delays
    table[abi.VP_RAIL_P_GAIN] = 1.0 + 0.01 * np.arange(N)                      # a row outside the dimensions, all different
    rig = Rig(M, K, W, D, model_table=table, params={"RAIL_VELOCITY_SCALE": [0.5, 1.5], "FPAM_K": [0.7, 1.3]})
    ref = None
    try:
        acts = rig.warm_plant(10, scale=1.3)
        rig.plant.reset_t[2] = 1                                               # (copied or not, the pin clears the sample's flag)
        rig.ok(rig.anchor())
        rng = np.random.default_rng(5)
        rig.mean.copy_(torch.as_tensor(np.stack([rng.uniform(0.7, 1.3, M), rng.uniform(0.8, 1.2, M)], axis=1)))
        rig.std.copy_(torch.as_tensor(np.stack([rng.uniform(0.05, 0.4, M), rng.uniform(0.05, 0.4, M)], axis=1)))
        rig.passes.copy_(torch.as_tensor([0, 3, (1 << 32) + 1, 7, 123456789]))
        rig.trace_actions.copy_(torch.as_tensor(rng.uniform(-1, 1, (M, W, 2)).astype(np.float32)))
        rig.model.state_t.fill_(SENTINEL)
        rig.model.step_count = 5
        rig.model.rew_t.fill_(SENTINEL)
        rig.model.reset_t.fill_(1)
        rig.model.progress_t.fill_(-5)
        before = rig.model.table_t.cpu().numpy().copy()
        rig.ok(rig.pin())
        torch.cuda.synchronize()
        assert rig.model.step_count == 5 and rig.plant.step_count == 10
        # the table: the dimensions' rows are the candidates', bit for bit; every other row keeps its bits
        theta = rig.theta()
        assert np.array_equal(theta[:, 0], rig.mean.cpu().numpy()) and (theta == 1.5).any() and (theta[..., 0] == 0.5).any()
        after = rig.model.table_t.cpu().numpy()
        want = mpc_adapt.table_rows(theta.reshape(N, D), rig.dims, base)
        assert sorted(want) == [abi.VP_RAIL_VELOCITY_SCALE] + list(range(abi.VP_FPAM_K0, abi.VP_FPAM_K0 + 5))
        for r in range(abi.VP_COUNT):
            assert _same(after[r], want[r] if r in want else before[r]), r
        assert len(np.unique(after[abi.VP_FPAM_K0 + 2])) > N // 2
        # the copy
        ast, st = rig.anchor_state.cpu().numpy(), rig.model.state_t.cpu().numpy()
        plant_of = np.arange(N) // K
        assert _same(ast, rig.plant.state_t.cpu().numpy())
        for f in NOT_RING:
            assert _same(st[f], ast[f][plant_of]), f
        assert np.array_equal(rig.model.progress_t.cpu().numpy(), rig.plant.progress_t.cpu().numpy()[plant_of])
        assert not rig.model.reset_t.any() and not rig.model.rew_t.any() and not rig.err.any()
        assert np.all(rig.alive.cpu().numpy() == 1) and int(rig.window[0]) == 5
        assert _same(rig.actions.cpu().numpy(), rig.trace_actions.cpu().numpy()[plant_of, 0])
        # the ring, against a handle that stepped with the table the pin left
        ref = _env(_cfg(N), after)
        ref.step_count = 16 - F.MAX_DELAY
        for a in acts[-F.MAX_DELAY:]:
            ref.step(np.repeat(a, K, axis=0), sync=False)
        torch.cuda.synchronize()
        assert ref.step_count == 16
        ref_ring, ring = ref.state_t[RING].cpu().numpy(), st[RING]
        for e in range(N):
            d = int(delays[e])
            for k in range(1, d + 1):
                for w in (0, 1):
                    assert _same(ring[2 * ((5 - k) % d) + w, e], ref_ring[2 * ((16 - k) % d) + w, e]), (e, k, w)
            assert np.all(ring[2 * d:, e] == np.float32(SENTINEL)), e
        # the rail command of two samples of one plant differs only through their own candidate of RAIL_VELOCITY_SCALE
        e0, e1 = 1, 10                                                         # plant 0, delays 1 and 1 (10 % 9)
        assert after[abi.VP_RAIL_VELOCITY_SCALE, e0] != after[abi.VP_RAIL_VELOCITY_SCALE, e1]
        assert not _same(ring[2 * ((5 - 1) % 1), e0], ring[2 * ((5 - 1) % 1), e1])
    finally:
        rig.close()
        if ref is not None:
            ref.close()


# --------------------------------------------------------------------------------------------------------- exact recovery
@pytest.mark.parametrize("pipe", [False, True], ids=["free", "pipe"])
def test_candidates_that_are_the_plant_score_zero(pipe):
    """(5, 14, 6, 2): the belief's mean is every plant's true DAMPING and FPAM_K factor, so candidate 0 IS the plant and must
    score err == 0.0 exactly over the window; every candidate whose table rows differ scores more.  Plant 3 is driven over the
    rail limit inside the window: its trace closes there, its candidates compare that many steps and nothing behind them, and
    candidate 0 crosses with it.  Plant 1's reset was raised at the anchor: no trace, every err stays 0."""
    M, K, W, D = SHAPES[0]
    rig = Rig(M, K, W, D, pipe=pipe)
    try:
        rig.warm_plant(11, seed=5, scale=0.6)
        rig.believe_the_truth()
        rig.traced_window(toward_limit=3, pending=1)
        t3 = int(rig.trace_len[3])
        assert np.array_equal(rig.trace_len.cpu().numpy(), [W, 0, W, t3, W]) and 1 < t3 < W, rig.trace_len
        assert np.array_equal(rig.episode_ended.cpu().numpy(), [0, 0, 0, 1, 0])
        before = rig.model.table_t.cpu().numpy().copy()
        states, resets, errs = rig.replay()
        err = errs[-1].reshape(M, K)
        after = rig.model.table_t.cpu().numpy()
        plant_rows = rig.plant.table_t.cpu().numpy()
        assert _same(after[:, ::K], plant_rows)                                # candidate 0 holds the plant's column
        rows = [abi.VP_DAMPING] + list(range(abi.VP_FPAM_K0, abi.VP_FPAM_K0 + 5))
        differs = (_bits(after[rows]) != _bits(np.repeat(plant_rows[rows], K, axis=1))).any(axis=0).reshape(M, K)
        assert differs[:, 1:].sum() >= M * (K - 1) - 2 and not differs[:, 0].any()
        assert not _same(after[rows], before[rows])
        for p in (0, 2, 3, 4):
            assert err[p, 0] == 0.0, (p, err[p, 0])
            assert np.all(err[p][differs[p]] > 0.0) and np.all(err[p][~differs[p]] == 0.0), p
        assert not err[1].any()
        # plant 3 compares t3 steps: its sums stop moving behind score node t3
        lanes = slice(3 * K, 4 * K)
        for k in range(t3, W):
            assert _same(errs[k][lanes], errs[t3 - 1][lanes]), k
        assert not _same(errs[t3 - 2][lanes], errs[t3 - 1][lanes])
        # ... and the candidate that is the plant crosses the limit with it, in step t3, and stays alive
        assert resets[t3 - 1][3 * K] == 1 and not resets[:t3 - 1, 3 * K].any()
        assert np.all(rig.alive.cpu().numpy()[lanes][~differs[3]] == 1)
    finally:
        rig.close()


# --------------------------------------------------------------------------------------------------------- the score's sums
def test_score_sums_against_numpy():
    """(5, 14, 6, 2), weights on the six q and on qd2.  The device's sums against ``mpc_adapt.score`` over snapshots of the
    model's state, within 1e-12 relative (each step's term is formed from the same float32 words in float64; the orders of
    the additions are the same, so in fact they agree far closer).  A candidate driven past the rail limit behind the pin
    raises its reset in step 1, before its plant: +inf, dead, and every other sum is what a run without it gives, bit for
    bit.  A NaN in a compared field while score node 2 runs: +inf, dead.  Plant 3's trace closes inside the window (it is driven
    over the rail limit), plant 1 has none."""
    M, K, W, D = SHAPES[0]
    RUNAWAY, NAN_ENV = 33, 52
    spec = dict(weights={**{"q%d" % i: 1.0 for i in range(6)}, "qd2": 0.5})
    rig, base = Rig(M, K, W, D, **spec), Rig(M, K, W, D, **spec)
    try:
        for r in (rig, base):
            r.warm_plant(10)
            r.mean.copy_(torch.as_tensor(np.tile([0.04, 1.0], (M, 1))))
            r.std.copy_(torch.as_tensor(np.tile([0.02, 0.1], (M, 1))))
            r.traced_window(toward_limit=3, pending=1)
        t3 = int(rig.trace_len[3])
        assert 1 < t3 < W
        states, resets, errs = rig.replay(plant_nan=(2, NAN_ENV), runaway=RUNAWAY)
        w = np.array(list(rig.acfg.weights), dtype=np.float32)
        assert (w != 0).sum() == 7
        want, alive = mpc_adapt.score(states, resets, rig.trace_rows.cpu().numpy(), rig.trace_len.cpu().numpy(), w, K)
        got = errs[-1]
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
        print("score sums: max relative difference %.3g" % (np.abs(got[fin] - want[fin]) / np.maximum(want[fin], 1e-300)).max())
        assert np.all(np.abs(got[fin] - want[fin]) <= 1e-12 * want[fin])
        assert np.array_equal(rig.alive.cpu().numpy(), alive)
        assert resets[0][RUNAWAY] == 1 and np.isposinf(got[RUNAWAY]) and alive[RUNAWAY] == 0
        assert np.isposinf(got[NAN_ENV]) and alive[NAN_ENV] == 0 and np.isfinite(errs[0][NAN_ENV]) and errs[0][NAN_ENV] > 0
        assert np.isposinf(errs[1][NAN_ENV])
        assert np.isfinite(np.delete(got, [RUNAWAY, NAN_ENV])).all()
        _, _, errs0 = base.replay()
        others = np.setdiff1d(np.arange(M * K), [RUNAWAY, NAN_ENV])
        assert _same(got[others], errs0[-1][others]) and np.isfinite(errs0[-1]).all()
        # the actions behind each node: the traced ones, the last one repeated; a plant without a trace keeps the pin's
        acts = rig.actions.cpu().numpy().reshape(M, K, 2)
        ta, tl = rig.trace_actions.cpu().numpy(), rig.trace_len.cpu().numpy()
        for p in range(M):
            assert _same(acts[p], np.broadcast_to(ta[p, min(W, tl[p] - 1) if tl[p] else 0], (K, 2))), p
        # one more node outside the window touches nothing
        rig.model.step_t(rig.actions, sync=False)
        rig.ok(rig.score())
        torch.cuda.synchronize()
        assert _same(rig.err.cpu().numpy(), got) and _same(rig.actions.cpu().numpy().reshape(M, K, 2), acts)
    finally:
        rig.close()
        base.close()


@pytest.mark.parametrize("shape", SHAPES[1:], ids=["2x300x3x1", "1x2x1x1"])
def test_pin_and_score_at_the_other_shapes(shape):
    M, K, W, D = shape
    rig = Rig(M, K, W, D)
    try:
        rig.warm_plant(9, seed=M + K)
        rig.believe_the_truth()
        rig.passes.copy_(torch.as_tensor([(1 << 40) + 5, 2][:M]))
        rig.traced_window()
        rig.model.state_t.fill_(SENTINEL)
        states, resets, errs = rig.replay()
        theta = rig.theta()
        after = rig.model.table_t.cpu().numpy()
        assert _same(after[abi.VP_DAMPING], theta[..., 0].reshape(-1).astype(np.float32))
        want, alive = mpc_adapt.score(states, resets, rig.trace_rows.cpu().numpy(), rig.trace_len.cpu().numpy(),
                                      list(rig.acfg.weights), K)
        got = errs[-1]
        assert np.isfinite(got).all() and np.all(np.abs(got - want) <= 1e-12 * want) and rig.alive.all()
        assert np.all(got.reshape(M, K)[:, 0] == 0.0) and int(rig.window[0]) == 7
        same_row = _bits(after[abi.VP_DAMPING].reshape(M, K)) == _bits(after[abi.VP_DAMPING].reshape(M, K)[:, :1])
        assert np.all(got.reshape(M, K)[~same_row] > 0.0) and (~same_row).sum() >= M * (K - 1) - 1
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------ the estimate
@pytest.mark.parametrize("forget", [False, True], ids=["keep", "forget"])
@pytest.mark.parametrize("shape", SHAPES, ids=["5x14x6x2", "2x300x3x1", "1x2x1x1"])
def test_estimate_against_numpy(shape, forget):
    """Errors made by hand on the device; ``mpc_adapt.estimate`` is fed the device's own inputs.  Weights, mean and std within
    1e-12 relative (the exponent is formed from the same float64 values up to the order of the sum behind ebar, at most 300
    terms; the device's exp and sqrt are within an ulp; the weighted sums differ in order).  The branches that compute
    nothing -- no finite error, a trace shorter than min_steps, forgetting -- are exact.  The planning rows of all K samples
    are the rounding of the new mean; every other row keeps its bits; passes is incremented; two runs give the same bits."""
    M, K, W, D = shape
    rig = Rig(M, K, W, D)
    try:
        rig.acfg.forget_on_reset = int(forget)
        rng = np.random.default_rng(M * 1000 + K)
        err = rng.uniform(0.0, 0.6, (M, K))
        err[0, 0] = np.inf                                                     # (the belief itself is out: the mean must move)
        tl, ended = np.full(M, W, dtype=np.int32), np.zeros(M, dtype=np.uint8)
        if M >= 2:
            err[1, :] = np.inf                                                 # no finite error: the belief stays
        if M >= 3:
            tl[2] = rig.acfg.min_steps - 1                                     # too short a trace: the belief stays
            ended[3] = 1                                                       # forgets, or is estimated like any other
            err[4, 1:] += 50.0                                                 # one candidate (the belief) far below the rest
        lo = np.array([d[2] for d in rig.dims])
        hi = np.array([d[3] for d in rig.dims])
        mean = lo + rng.uniform(0.2, 0.8, (M, D)) * (hi - lo)
        std = rng.uniform(0.05, 0.3, (M, D)) * (hi - lo)
        prior_mean, prior_std = lo + 0.5 * (hi - lo) + np.zeros((M, D)), 0.25 * (hi - lo) + np.zeros((M, D))
        passes = rng.integers(0, 1 << 34, M)
        table = rig.model.table_t.cpu().numpy().copy()
        table[abi.VP_RAIL_P_GAIN] = 1.0 + 0.01 * np.arange(M * K)
        outs = []
        for _ in range(2):
            for t, v in ((rig.err, err.reshape(-1)), (rig.trace_len, tl), (rig.episode_ended, ended), (rig.mean, mean),
                         (rig.std, std), (rig.prior_mean, prior_mean), (rig.prior_std, prior_std), (rig.passes, passes),
                         (rig.model.table_t, table)):
                t.copy_(torch.as_tensor(v))
            rig.ok(rig.estimate())
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy().copy() for t in (rig.mean, rig.std, rig.weights, rig.passes, rig.model.table_t)])
        for a, b in zip(*outs):
            assert _same(a, b)
        got_mean, got_std, got_w, got_passes, got_table = outs[0]
        theta = mpc_adapt.candidates(mean, std, rig.dims, rig.seed, K, passes)
        r = mpc_adapt.estimate(err.reshape(-1), theta, mean, std, prior_mean, prior_std, tl, ended, rig.dims,
                               rig.acfg.min_steps, rig.acfg.temperature, rig.acfg.rate, forget)
        w = got_w.reshape(M, K)
        assert np.all(np.abs(w - r["weights"]) <= 1e-12 * r["weights"])
        assert np.all(np.abs(got_mean - r["mean"]) <= 1e-12 * np.abs(r["mean"]))
        assert np.all(np.abs(got_std - r["std"]) <= 1e-12 * r["std"])
        assert np.array_equal(got_passes, passes + 1)
        assert r["estimated"][0] and w[0].max() == 1.0 and (w[0] == 0.0).sum() >= 1
        assert not _same(got_mean[0], mean[0])
        if M >= 2:
            assert not r["estimated"][1] and not w[1].any() and _same(got_mean[1], mean[1]) and _same(got_std[1], std[1])
        if M >= 3:
            assert not r["estimated"][2] and not w[2].any() and _same(got_mean[2], mean[2]) and _same(got_std[2], std[2])
            if forget:
                assert r["forgot"][3] and not w[3].any()
                assert _same(got_mean[3], prior_mean[3]) and _same(got_std[3], prior_std[3])
            else:
                assert r["estimated"][3] and w[3].max() == 1.0 and not _same(got_mean[3], mean[3])
            # the temperature is relative to the spread of the errors: tau = 0.1 * (ebar - beta) is about 0.1 * 50 * 13 / 14
            # here, so the thirteen others keep exp(-10 * 14 / 13) = 2e-5 each, whatever the 50 is
            assert w[4, 0] == 1.0 and 1e-5 < w[4, 1:].min() and w[4, 1:].max() < 3e-5
        # the planning rows: the candidates' rounding of the DEVICE's new mean over all K samples; the other rows untouched
        plan = np.minimum(np.maximum(got_mean, lo), hi)
        want = mpc_adapt.table_rows(np.repeat(plan, K, axis=0), rig.dims, rig.base)
        for row in range(abi.VP_COUNT):
            assert _same(got_table[row], want[row] if row in want else table[row]), row
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------ the task classes
DAMPINGS = [0.01, 0.03, 0.07, 0.095]


def _plant_cfg(M, seed=9, pipe=False, **env_over):
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % M])
    cfg["seed"] = seed
    cfg["task"]["vine_randomize"] = False
    cfg["env"].update(CREATE_PIPE=pipe, CREATE_SHELF=False, ENV_PARAMS={"DAMPING": {"values": DAMPINGS[:M]}})
    cfg["env"].update(env_over)
    return cfg


def _adaptive(M, K, H, adapt, plant_over=None, **ctl):
    cfg = _plant_cfg(M, **(plant_over or {}))
    mcfg = mpc.model_config(cfg, M, K)
    mcfg["env"]["ENV_PARAMS"] = {"FPAM_K": 1.0}                                # a table that holds the configuration's own row
    plant, model = mpc.make_task(cfg), mpc.make_task(mcfg)
    return plant, model, mpc_adapt.AdaptiveController(plant, model, K, adapt, H, **ctl)


def test_captured_cycles_against_eager_ones():
    """Two captured cycles replayed three times against six eager ones, and two control steps more that no cycle holds: the
    belief, the model's table, the traces, every controller tensor and both state blocks bit-identical.  Episodes of ten
    steps, so that traces close and resets are consumed inside the graph."""
    M, K, H = 4, 16, 6
    adapt = {"params": {"DAMPING": [0.005, 0.1], "FPAM_K": [0.7, 1.3]}, "window": 4, "every": 5, "min_steps": 2}
    runs = []
    for tag, kw in (("graph", dict(graph=True, graph_cycles=2)), ("eager", dict(graph=False))):
        plant, model, ctl = _adaptive(M, K, H, adapt, plant_over=dict(maxEpisodeLength=10), seed=5, keep_weights=True, **kw)
        try:
            assert ctl.use_graph == (tag == "graph") and (ctl.W, ctl.E, ctl.D) == (4, 5, 2)
            assert plant.step_kernel_name == model.step_kernel_name == "vine_step_kernel"
            ctl.run(32)
            torch.cuda.synchronize()
            counts = {"fork": 32, "step": 32 * H, "node": 32 * H, "update": 32, "plant_step": 32, "anchor": 7, "trace": 32,
                      "pin": 6, "adapt_step": 6 * 4, "score": 6 * 4, "estimate": 6}
            if tag == "graph":
                assert ctl.graph_launches == {k: v // 3 for k, v in dict(counts, fork=30, step=30 * H, node=30 * H, update=30,
                                                                          plant_step=30, anchor=6, trace=30).items()}
            assert ctl.launches == counts and ctl.phase == 2
            assert plant.step_count == 32 and model.step_count == 32 * H + 6 * 4 and np.all(ctl.passes.cpu().numpy() == 6)
            assert (plant.num_steps, model.num_steps) == (32, 32 * H + 6 * 4)  # replayed or eager: the steps the handles took
            runs.append(([t.cpu().numpy().copy() for t in ctl.tensors()], plant.state.cpu().numpy().copy(),
                         model.state.cpu().numpy().copy(), ctl.mean.cpu().numpy().copy()))
        finally:
            model.close()
            plant.close()
    (ta, pa, ma, mean), (tb, pb, mb, _) = runs
    for a, b in zip(ta, tb):
        assert _same(a, b)
    assert _same(pa, pb) and _same(ma, mb)
    assert mean.shape == (M, 2) and np.isfinite(mean).all() and not np.all(mean[:, 0] == np.float64(np.float32(0.02)))


def test_without_adapt_nothing_changes():
    """``play`` without ``adapt``: the summed plant reward and the launch counts of a short run, against what the commit before
    this feature gave (tests/golden/mpc_play_no_adapt.json, recorded there with the same call), bit for bit; and a plain
    ``Controller`` launches what it launched."""
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
        assert out["graphed"] == want["graphed"] and out["model_table_bound"] == want["model_table_bound"]
        assert "adapt" not in out


def test_play_with_adapt_and_set_model_params(tmp_path):
    """``play(adapt=...)`` through ``mpc.py``'s main: whole cycles from the graph, the report's extra block; and
    ``set_model_params`` refuses an adapted name and refreshes the mirror's adapted rows from the device."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mpc_cli", os.path.join(REPO, "mpc.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    argv = ["plants=4", "samples=32", "horizon=6", "steps=20", "out=%s" % tmp_path, "task.env.CREATE_PIPE=False",
            "task.task.vine_randomize=False", "seed=3", "task.env.ENV_PARAMS={DAMPING: {values: [0.01, 0.03, 0.07, 0.095]}}",
            "adapt={params: {DAMPING: [0.005, 0.1]}, window: 4, every: 4}"]
    out = cli.main(argv)
    a = out["adapt"]
    assert a["names"] == ["DAMPING"] and a["mean"].shape == a["std"].shape == a["truth"].shape == (4, 1)
    assert np.allclose(a["truth"][:, 0], DAMPINGS, rtol=1e-6) and np.all(a["passes"] == 5)
    assert np.all(a["prior_mean"] == np.float64(np.float32(0.02)))             # the model's own DAMPING
    assert out["launches"]["estimate"] == 5 and out["launches"]["trace"] == 20 and out["graphed"] and out["model_table_bound"]
    assert set(a["prior_error"]) == set(a["final_error"]) == {"DAMPING"} and np.isfinite(out["plant_return"]).all()
    plant, model, ctl = _adaptive(4, 8, 3, {"params": {"DAMPING": [0.005, 0.1]}, "window": 2, "every": 2}, graph=False)
    try:
        ctl.run(4)
        with pytest.raises(ValueError, match="DAMPING is adapted on the device"):
            ctl.set_model_params({"DAMPING": 0.05})
        assert not _same(model._env_params_host[abi.VP_DAMPING], model.env_params[abi.VP_DAMPING].cpu().numpy())     # stale
        ctl.set_model_params({"RAIL_P_GAIN": np.array([1.0, 2.0, 3.0, 4.0])})
        table = model.env_params.cpu().numpy()
        assert _same(model._env_params_host, table)
        assert _same(table[abi.VP_RAIL_P_GAIN], np.repeat(np.float32([1, 2, 3, 4]), 8))
        mean, _ = ctl.belief()
        assert _same(table[abi.VP_DAMPING], np.repeat(mean[:, 0].astype(np.float32), 8))      # the planning value, untouched
    finally:
        model.close()
        plant.close()


def test_it_adapts():
    """M = 4 plants with DAMPING 0.01, 0.03, 0.07 and 0.095 in the range [0.005, 0.1]; the prior sits at mid-range, 0.0525; K =
    64 candidates, H = 8, W = E = 8, P = 10 passes (80 control steps), the defaults otherwise.  std_floor is 0.01 * 0.095, so
    every plant's prior error (0.0425, 0.0225, 0.0175, 0.0425) exceeds twice it.  Condition: each final |mean - truth| is at
    most half the prior's.  scripts/mpc_adapt_oracle_check.py drove the numpy statements with float64 oracle traces for these
    values first; profiles/mpc_adapt/it_adapts.txt holds its ratios and the device's."""
    M, K, H, P = 4, 64, 8, 10
    adapt = {"params": {"DAMPING": [0.005, 0.1]}, "window": 8, "every": 8}
    cfg = _plant_cfg(M, seed=1, USE_TARGET_REACHED_RESET=False)
    mcfg = mpc.model_config(cfg, M, K)
    mcfg["env"]["ENV_PARAMS"] = {"DAMPING": 0.0525}
    plant, model = mpc.make_task(cfg), mpc.make_task(mcfg)
    try:
        ctl = mpc_adapt.AdaptiveController(plant, model, K, adapt, H, seed=1)
        prior = ctl.prior_mean.cpu().numpy()[:, 0]
        truth = ctl.truth()[:, 0]
        assert np.all(prior == np.float64(np.float32(0.0525))) and np.allclose(truth, DAMPINGS, rtol=1e-6)
        floor = ctl.dims[0][4]
        assert np.all(np.abs(prior - truth) > 2 * floor)
        ctl.run(P * ctl.E)
        mean, std = ctl.belief()
        ratio = np.abs(mean[:, 0] - truth) / np.abs(prior - truth)
        print("it adapts: truth %s, final mean %s, final std %s, |mean - truth| / |prior - truth| %s, passes %s" % (
            truth, mean[:, 0], std[:, 0], ratio, ctl.passes.cpu().numpy()))
        assert np.all(ctl.passes.cpu().numpy() == P)
        assert np.all(ratio <= 0.5), ratio
    finally:
        model.close()
        plant.close()
