"""MPC_POLICY on the GPU (include/vine_mpc_policy.h, utils/mpc_policy.py): the four launches against the numpy statements and
against ``vine_policy_head_rms``, the closed loop against itself (with zero noise the controller IS the policy), the captured
graph against eager launches, ``play`` and the command line.

A freshly initialised network (``torch.manual_seed``) and ``maxEpisodeLength=8`` throughout.  Shapes (M plants, K samples, H
steps) are the smallest the kernels allow with N = M K a multiple of 512: (256, 2, 3), (2, 256, 3), (3, 512, 2) = 1536 rows, no
power of two and an odd M, and (128, 4, 1).  "Bit for bit" is literal: floats are compared as words."""
import json
import os

import numpy as np
import pytest
import torch

from vine_robot_isaacgymenvs_amd import abi, load_config
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_policy

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _nothing_left_for_a_later_capture():
    """The tasks of a test are reference cycles (a task and its observers), and so is the frame of a test that caught an
    exception; with their tensors and graphs they would otherwise wait for whichever collection comes next -- possibly on
    the autograd thread in the middle of a later test's graph capture.  They go here, where nothing is being captured."""
    yield
    import gc
    gc.collect()


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7777.0
SHAPES = [(256, 2, 3), (2, 256, 3), (3, 512, 2), (128, 4, 1)]
IDS = ["256x2x3", "2x256x3", "3x512x2", "128x4x1"]
U = abi.MPC_POLICY_UNITS


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _np(t):
    return t.detach().cpu().numpy().copy()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class Rig:
    """A plant task, its model task, the network and the controller."""

    def __init__(self, M, K, H, pipe=False, cost=None, plant_over=None, net_seed=0, task_seed=9, max_len=8, **ctl):
        cfg = load_config(overrides=["num_envs=%d" % M] + (["task.env.maxEpisodeLength=%d" % max_len] if max_len else []))
        task = cfg["task"]
        task["seed"] = task_seed
        task["task"]["vine_randomize"] = False
        task["env"].update(CREATE_PIPE=bool(pipe), CREATE_SHELF=False)
        task["env"].update(plant_over or {})
        self.params = cfg["train"]["params"]
        self.plant = self.model = None
        try:
            self.plant = mpc.make_task(task)
            self.model = mpc.make_task(mpc.model_config(task, M, K, cost))
            torch.manual_seed(net_seed)
            self.net = mpc_policy.PolicyProposal(self.params, M * K, int(self.plant.num_obs))
            self.ctl = mpc_policy.PolicyController(self.plant, self.model, K, self.net, H, **ctl)
        except BaseException:
            self.close()
            raise
        self.M, self.K, self.H, self.N = M, K, H, M * K
        self.dev, self.lib = self.plant.device, self.plant._lib
        self.clip = float(self.model.clip_actions)

    def set_k(self, k):
        """The horizon step the next launch reads: the model's step count minus ``window[0]``."""
        self.ctl.window.fill_(int(self.model.step_count) - int(k))

    def close(self):
        if self.model is not None:
            self.model.close()
        if self.plant is not None:
            self.plant.close()


def _random_head(rig, seed=1):
    """Head operands of order one through ``vine_rollout_head_prep``, as tests/test_eval_step.py makes them; value
    statistics of order one."""
    dev = rig.dev
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    p = dict(gamma=1.0 + 0.1 * rnd(U), beta=0.1 * rnd(U), w_mu=0.1 * rnd(2, U), b_mu=0.1 * rnd(2), w_v=0.1 * rnd(1, U),
             b_v=0.1 * rnd(1), logstd=torch.tensor([-0.3, 0.2], device=dev), hw=torch.empty(3 * U, device=dev),
             hc=torch.empty(3, device=dev), vmean=torch.tensor([0.37], device=dev, dtype=torch.float64),
             vvar=torch.tensor([2.3], device=dev, dtype=torch.float64), counter=torch.tensor([3], device=dev, dtype=torch.int64))
    assert rig.lib.vine_rollout_head_prep(p["gamma"].data_ptr(), p["beta"].data_ptr(), p["w_mu"].data_ptr(), p["b_mu"].data_ptr(),
                                          p["w_v"].data_ptr(), p["b_v"].data_ptr(), p["hw"].data_ptr(), p["hc"].data_ptr(),
                                          _stream(dev)) == 0
    return p, rnd


def _head_rms(rig, p, y):
    """``vine_policy_head_rms`` on the same rows: ``(mu [N, 2], value [N])``."""
    N, dev = y.shape[0], rig.dev
    s = dict(mu=torch.empty(N, 2, device=dev), sigma=torch.empty(N, 2, device=dev), value=torch.empty(N, 1, device=dev),
             action=torch.empty(N, 2, device=dev), nlp=torch.empty(N, device=dev))
    assert rig.lib.vine_policy_head_rms(N, 2, U, y.data_ptr(), p["w_mu"].data_ptr(), p["b_mu"].data_ptr(), p["w_v"].data_ptr(),
                                        p["b_v"].data_ptr(), p["logstd"].data_ptr(), p["vmean"].data_ptr(), p["vvar"].data_ptr(),
                                        1e-5, 12345, p["counter"].data_ptr(), s["mu"].data_ptr(), s["sigma"].data_ptr(),
                                        s["value"].data_ptr(), s["action"].data_ptr(), s["nlp"].data_ptr(), p["gamma"].data_ptr(),
                                        p["beta"].data_ptr(), 1e-5, _stream(dev)) == 0
    torch.cuda.synchronize()
    return _np(s["mu"]), _np(s["value"]).reshape(N)


def _act(rig, p, y, h, c, mu_out):
    ctl = rig.ctl
    rc = rig.lib.vine_mpc_policy_act(rig.model._handle, ctl.mcfg, ctl.pcfg, y.data_ptr(), p["hw"].data_ptr(), p["hc"].data_ptr(),
                                     ctl.window.data_ptr(), rig.plant.reset_buf.data_ptr(), h.data_ptr(), c.data_ptr(),
                                     ctl.actions.data_ptr(), ctl.mu0.data_ptr(), ctl.plant_h.data_ptr(), ctl.plant_c.data_ptr(),
                                     mu_out.data_ptr() if mu_out is not None else None, _stream(rig.dev))
    assert rc == abi.OK, rig.lib.vine_last_error()
    torch.cuda.synchronize()


def _terminal(rig, p, y, value_out, stats=True):
    ctl = rig.ctl
    rc = rig.lib.vine_mpc_policy_terminal(rig.model._handle, ctl.mcfg, ctl.pcfg, y.data_ptr(), p["hw"].data_ptr(),
                                          p["hc"].data_ptr(), p["vmean"].data_ptr() if stats else None,
                                          p["vvar"].data_ptr() if stats else None, ctl.window.data_ptr(), ctl.cost.data_ptr(),
                                          ctl.alive.data_ptr(), value_out.data_ptr() if value_out is not None else None,
                                          _stream(rig.dev))
    assert rc == abi.OK, rig.lib.vine_last_error()
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------- 1. the fork
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fork_copies_the_plants_rows_and_nothing_else(shape):
    """Into buffers full of a sentinel (three rows longer than N, the operand buffer 352 columns wide with h behind column
    96): every sample's row of the observation buffer, h, c and the operand copy is its plant's row bit for bit; the columns
    in front of h and the rows beyond N keep the sentinel."""
    M, K, H = shape
    rig = Rig(M, K, H, graph=False)
    try:
        N, dev, ctl, W = rig.N, rig.dev, rig.ctl, int(rig.plant.num_obs)
        g = torch.Generator(device=dev).manual_seed(M + K)
        plant_obs = torch.randn(M, W, device=dev, generator=g)
        plant_h, plant_c = torch.randn(M, U, device=dev, generator=g), torch.randn(M, U, device=dev, generator=g)
        obs = torch.full((N + 3, W), SENTINEL, device=dev)
        h, c = torch.full((N + 3, U), SENTINEL, device=dev), torch.full((N + 3, U), SENTINEL, device=dev)
        op = torch.full((N + 3, 352), SENTINEL, device=dev)
        rc = rig.lib.vine_mpc_policy_fork(rig.plant._handle, rig.model._handle, ctl.mcfg, ctl.pcfg, plant_obs.data_ptr(), W,
                                          obs.data_ptr(), W, plant_h.data_ptr(), plant_c.data_ptr(), h.data_ptr(), c.data_ptr(),
                                          op.data_ptr() + 4 * 96, 352, _stream(dev))
        assert rc == abi.OK, rig.lib.vine_last_error()
        torch.cuda.synchronize()
        plant_of = np.arange(N) // K
        assert _same(_np(obs)[:N], _np(plant_obs)[plant_of])
        assert _same(_np(h)[:N], _np(plant_h)[plant_of]) and _same(_np(c)[:N], _np(plant_c)[plant_of])
        assert _same(_np(op)[:N, 96:], _np(plant_h)[plant_of])
        assert np.all(_np(op)[:, :96] == np.float32(SENTINEL))
        for t in (obs, h, c, op):
            assert np.all(_np(t)[N:] == np.float32(SENTINEL))
        # the controller's own call writes the buffer the next inference reads, whatever `cur` was left at
        rig.net._fast["cur"] = 1
        ctl.plant_h.copy_(plant_h)
        ctl.policy_fork()
        torch.cuda.synchronize()
        assert rig.net._fast["cur"] == 0 and _same(_np(rig.net._fast["xh2"][0])[:, 96:], _np(plant_h)[plant_of])
        assert _same(_np(rig.net.rnn_states[0][0]), _np(plant_h)[plant_of])
    finally:
        rig.close()


def test_handle_refusals_name_the_reason():
    """What only a handle shows: N != M K, and a model whose clip_actions is above 1 (no inner clamp is applied to mu)."""
    rig = Rig(2, 256, 3, graph=False)
    try:
        ctl, lib = rig.ctl, rig.lib
        good = ctl.mcfg
        ctl.mcfg = mpc.mpc_config(4, 256, 3)
        for fn in (ctl.policy_fork, lambda: ctl.policy_act(rig.net.rnn_states[0][0]), ctl.policy_compose,
                   lambda: ctl.policy_terminal(rig.net.rnn_states[0][0])):
            with pytest.raises(ValueError, match="num_plants \\* samples|num_plants envs"):
                fn()
        ctl.mcfg = good
    finally:
        rig.close()
    with pytest.raises(NotImplementedError, match="clip_actions above 1"):
        wide = Rig(2, 256, 3, graph=False, plant_over={"clipActions": 1.5})
        try:
            wide.ctl.policy_fork()
        finally:
            wide.close()


# --------------------------------------------------------------------------------------------------------------- 2. the act
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_act_against_the_head_kernel_the_float64_statement_and_numpy(shape):
    """Random rows ``y``.  mu against ``vine_policy_head_rms``'s ``mu_out`` at rtol = atol = 2e-6 (what tests/test_eval_step.py
    holds the two head kernels to); the value (through the terminal launch's ``value_out``, statistics of order one) against
    its ``value_out`` at the same 2e-6; mu against the float64 ``head`` statement within the worst-case bound of a float32 dot
    product of 256 terms in any order, 256 * 2^-24 * (rstd * sum_u |hw_u| (|y_u| + |mean|) + |hc|); the action buffer bit for
    bit against ``float32(clamp(mu_device + d))`` formed in numpy from the device's own mu, with rows whose sum leaves
    +-clip at both ends."""
    M, K, H = shape
    rig = Rig(M, K, H, graph=False)
    try:
        N, dev, ctl = rig.N, rig.dev, rig.ctl
        p, rnd = _random_head(rig)
        y = (0.5 * rnd(N, U) + 0.1).contiguous()
        d = (0.6 * rnd(N, 2)).contiguous()
        d[0], d[1] = torch.tensor([5.0, -5.0], device=dev), torch.tensor([-5.0, 5.0], device=dev)
        d[N - 1] = 0.0
        ctl.actions.copy_(d)
        mu_out = torch.full((N, 2), SENTINEL, device=dev)
        h, c = rnd(N, U), rnd(N, U)
        rig.set_k(min(1, H - 1))
        _act(rig, p, y, h, c, mu_out)
        mu, got = _np(mu_out), _np(ctl.actions)
        want = mpc_policy.act(mu, _np(d), rig.clip)
        assert _same(got, want)
        assert rig.clip == 1.0 and (got == 1.0).any() and (got == -1.0).any() and (np.abs(got) < 1.0).any()
        assert _same(got[N - 1], np.clip(mu[N - 1], -1.0, 1.0))
        ref_mu, ref_v = _head_rms(rig, p, y)
        print("mu against vine_policy_head_rms: max |diff| %.3g" % np.abs(mu - ref_mu).max())
        np.testing.assert_allclose(mu, ref_mu, rtol=2e-6, atol=2e-6)
        y64, hw, hc = _np(y).astype(np.float64), _np(p["hw"]).astype(np.float64).reshape(3, U), _np(p["hc"]).astype(np.float64)
        ref = mpc_policy.head(y64, hw, hc, 1e-5)
        mean = y64.mean(1, keepdims=True)
        rstd = 1.0 / np.sqrt(((y64 - mean) ** 2).mean(1) + 1e-5)
        bound = 256 * 2.0 ** -24 * (rstd[:, None] * ((np.abs(y64) + np.abs(mean)) @ np.abs(hw).T) + np.abs(hc))
        err = np.abs(mu - ref[:, :2])
        print("mu against the float64 statement: max |diff| %.3g, smallest bound %.3g" % (err.max(), bound[:, :2].min()))
        assert np.all(err <= bound[:, :2])
        # the value row, through the terminal launch
        value = torch.full((N,), SENTINEL, device=dev)
        ctl.alive.fill_(0)
        rig.set_k(H)
        _terminal(rig, p, y, value)
        v = _np(value)
        print("value against vine_policy_head_rms: max |diff| %.3g at |v| up to %.3g" % (np.abs(v - ref_v).max(), np.abs(v).max()))
        np.testing.assert_allclose(v, ref_v, rtol=2e-6, atol=2e-6)
        raw = np.clip(ref[:, 2], -5.0, 5.0) * np.sqrt(np.float64(np.float32(2.3)) + 1e-5) + 0.37
        assert np.all(np.abs(v - raw) <= np.sqrt(2.3) * bound[:, 2] + 2.0 ** -22 * (np.abs(raw) + 1.0))
        # outside 0 .. H - 1 the act touches nothing
        before = _np(ctl.actions)
        mu_out.fill_(SENTINEL)
        for k in (-1, H):
            rig.set_k(k)
            _act(rig, p, y, h, c, mu_out)
        assert _same(_np(ctl.actions), before) and np.all(_np(mu_out) == np.float32(SENTINEL))
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------- 3. the keep, the compose
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_keep_and_compose_against_numpy(shape):
    """k == 0: ``mu0``, ``plant_h``, ``plant_c`` are sample 0's rows bit for bit, zeros for a plant whose reset is raised; k > 0
    (where H allows one): the sentinel stays.  The composition: every other plant's ``plant_actions`` and ``history[p][0]`` are
    the composed action bit for bit (the clamp at both ends among them), the raised plant keeps action (0, 0) and its
    history front."""
    M, K, H = shape
    rig = Rig(M, K, H, graph=False)
    try:
        N, dev, ctl = rig.N, rig.dev, rig.ctl
        p, rnd = _random_head(rig, seed=2)
        y, h, c = (0.5 * rnd(N, U)).contiguous(), rnd(N, U), rnd(N, U)
        raised = np.zeros(M, dtype=np.int64)
        raised[[1, M - 1]] = 1
        rig.plant.reset_buf.copy_(torch.as_tensor(raised))
        mu_out = torch.empty((N, 2), device=dev)
        for k in ([1, 0] if H > 1 else [0]):
            for t in (ctl.mu0, ctl.plant_h, ctl.plant_c):
                t.fill_(SENTINEL)
            ctl.actions.copy_(0.3 * rnd(N, 2))
            rig.set_k(k)
            _act(rig, p, y, h, c, mu_out)
            if k > 0:
                for t in (ctl.mu0, ctl.plant_h, ctl.plant_c):
                    assert np.all(_np(t) == np.float32(SENTINEL))
        mu0, ph, pc = mpc_policy.keep(_np(mu_out), _np(h), _np(c), K, raised)
        assert _same(_np(ctl.mu0), mu0) and _same(_np(ctl.plant_h), ph) and _same(_np(ctl.plant_c), pc)
        assert _same(mu0[0], _np(mu_out)[0]) and not mu0[1].any() and not ph[M - 1].any() and ph[0].any()
        # the composition behind an update that wrote the residual's first entry
        residual = _np(0.5 * rnd(M, 2))
        residual[0] = [9.0, -9.0]
        residual[raised != 0] = 0.0
        history = _np(rnd(M, abi.MAX_DELAY, 2))
        history[:, 0] = residual
        ctl.plant_actions.copy_(torch.as_tensor(residual))
        ctl.history.copy_(torch.as_tensor(history))
        ctl.policy_compose()
        torch.cuda.synchronize()
        a, hist = mpc_policy.compose(mu0, residual, history, rig.clip, raised)
        assert _same(_np(ctl.plant_actions), a) and _same(_np(ctl.history), hist)
        assert not a[1].any() and _same(hist[1, 0], np.zeros(2, np.float32)) and _same(hist[:, 1:], history[:, 1:])
        assert _same(a[0], np.float32([1.0, -1.0]))                               # the clamp at both ends
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------- 4. closed-loop fidelity
@pytest.mark.parametrize("pipe", [False, True], ids=["free", "pipe"])
def test_with_zero_noise_the_controller_is_the_policy(pipe):
    """sigma = 0, zero residual, exact model, (2, 256, 3), four control steps without a reset, behind the plant step that
    consumes the reset a fresh plant starts with.  The mu a plant's sample 0
    computed at horizon step k of control step t equals ``mu0`` of control step t + k in every bit (the same kernels at the
    same N on the plant's own observation and LSTM state); the plant's action is ``clamp(mu0)``; all K samples of a plant
    agree in every bit.  Beside it the first ``mu0`` against the stock PyTorch model on the reset observation and zero state at
    atol 2e-4, the tolerance test_device_player_graph_replay_equals_eager_and_counts_episodes uses for that comparison."""
    M, K, H, T = 2, 256, 3, 4            # (a sample's progress reaches T - 1 + H = 6; the episode times out at 7)
    rig = Rig(M, K, H, pipe=pipe, sigma=0.0, graph=False, keep_mu=True)
    try:
        ctl, plant = rig.ctl, rig.plant
        plant.step_into(ctl.plant_actions, ctl.plant_obs)                  # one plant step on action zero consumes the reset
        torch.cuda.synchronize()
        assert not plant.reset_buf.any()
        obs0 = ctl.plant_obs.clone()
        mus, mu0s, acts = [], [], []
        with torch.no_grad():
            for t in range(T):
                ctl.fork()
                ctl.policy_fork()
                row = []
                for k in range(H):
                    ctl.policy_act(ctl.infer())
                    row.append(_np(ctl.mu).reshape(M, K, 2))
                    if k == 0:
                        mu0s.append(_np(ctl.mu0))
                    mpc.Controller.model_step(ctl)
                mus.append(row)
                assert int(ctl.alive.sum()) == M * K and not rig.model.reset_buf.any()
                ctl.update()
                ctl.policy_compose()
                acts.append(_np(ctl.plant_actions))
                plant.step_into(ctl.plant_actions, ctl.plant_obs)
                torch.cuda.synchronize()
                assert not plant.reset_buf.any() and not ctl.nominal.any()
        for t in range(T):
            assert _same(acts[t], mpc_policy.act(mu0s[t], np.zeros((M, 2), np.float32), rig.clip)), t
            assert _same(_np(ctl.history)[:, T - 1 - t], acts[t]), t
            for k in range(H):
                assert _same(mus[t][k], np.broadcast_to(mus[t][k][:, :1], (M, K, 2))), (t, k)
                if t + k < T:
                    assert _same(mus[t][k][:, 0], mu0s[t + k]), (t, k)
        assert len({mu0s[t].tobytes() for t in range(T)}) == T                     # (the policy's mean moved with the plant)
        with torch.no_grad():
            res = rig.net.model({"is_train": False, "prev_actions": None, "obs": obs0,
                                 "rnn_states": rig.net.model.get_default_rnn_state(M, rig.dev)})
        np.testing.assert_allclose(mu0s[0], _np(res["mus"]), rtol=0, atol=2e-4)
    finally:
        rig.close()


# --------------------------------------------------------------------------------------------------------- 5. the terminal
def test_terminal_against_numpy_and_the_launch_counts():
    """(3, 512, 2).  The cost behind the terminal launch bit for bit against the numpy statement from the device's own V; a
    dead sample untouched; a NaN planted in ``y`` gives +inf and clears ``alive``; at k != H nothing moves.  With
    ``terminal_value=0`` a control step issues H inferences and no terminal launch, else H + 1 and one."""
    M, K, H = SHAPES[2]
    rig = Rig(M, K, H, graph=False, terminal_value=0.75)
    try:
        N, dev, ctl = rig.N, rig.dev, rig.ctl
        p, rnd = _random_head(rig, seed=3)
        y = (0.5 * rnd(N, U)).contiguous()
        NAN_ENV, DEAD = 700, [5, 513, N - 1]
        y[NAN_ENV, 17] = float("nan")
        cost = torch.rand(N, device=dev, dtype=torch.float64)
        alive = torch.ones(N, device=dev, dtype=torch.uint8)
        alive[DEAD] = 0
        cost[DEAD[1]] = float("inf")
        value = torch.full((N,), SENTINEL, device=dev)
        for stats in (True, False):
            ctl.cost.copy_(cost)
            ctl.alive.copy_(alive)
            for k in (0, H - 1, H + 1):
                rig.set_k(k)
                _terminal(rig, p, y, None, stats)
            assert _same(_np(ctl.cost), _np(cost)) and _same(_np(ctl.alive), _np(alive))
            rig.set_k(H)
            _terminal(rig, p, y, value, stats)
            v = _np(value)
            want_cost, want_alive = mpc_policy.terminal(_np(cost), _np(alive), v, 0.75)
            assert _same(_np(ctl.cost), want_cost) and np.array_equal(_np(ctl.alive), want_alive)
            assert np.isnan(v[NAN_ENV]) and np.isposinf(want_cost[NAN_ENV]) and want_alive[NAN_ENV] == 0
            assert _same(want_cost[DEAD], _np(cost)[DEAD]) and not want_alive[DEAD].any()
            moved = np.setdiff1d(np.arange(N), DEAD + [NAN_ENV])
            assert np.all(want_cost[moved] != _np(cost)[moved]) and want_alive[moved].all()
            if stats:
                with_stats = v
            else:
                # without statistics V is the head's own row; with them, that row un-normalised (the device fuses the
                # multiply and the add: one rounding of a product of at most 5 * sqrt(2.3) apart)
                raw = mpc_policy.unnormalize_value(np.delete(v, NAN_ENV), 0.37, 2.3, 1e-5)
                assert np.all(np.abs(np.delete(with_stats, NAN_ENV) - raw) <= 2.0 ** -23 * (np.abs(raw) + 5.0 * np.sqrt(2.3)))
        ctl.run(1)
        assert ctl.launches["infer"] == H + 1 and ctl.launches["policy_terminal"] == 1 and ctl.launches["policy_act"] == H
    finally:
        rig.close()
    rig = Rig(M, K, H, graph=False)
    try:
        rig.ctl.run(2)
        torch.cuda.synchronize()
        assert rig.ctl.launches == {"fork": 2, "step": 2 * H, "node": 2 * H, "update": 2, "plant_step": 2, "policy_fork": 2,
                                    "infer": 2 * H, "policy_act": 2 * H, "policy_terminal": 0, "policy_compose": 2}
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------------------- 6. the capture
@pytest.mark.parametrize("H", [2, 3], ids=["even-H", "odd-H"])
def test_captured_control_steps_against_eager_ones(H):
    """Two captured control steps replayed three times against six eager ones, with noise and a terminal value: every
    controller tensor (the network's state and both operand buffers among them), both handles' state blocks, ``plant_h`` /
    ``plant_c`` and the step counts are bit-identical, for an even and an odd H (the operand buffers alternate per step;
    every control step starts on the first)."""
    M, K = 2, 256
    runs = []
    for tag, kw in (("graph", dict(graph=True, graph_steps=2)), ("eager", dict(graph=False))):
        rig = Rig(M, K, H, sigma=[0.5, 0.25], seed=5, terminal_value=0.5, **kw)
        try:
            ctl = rig.ctl
            assert ctl.use_graph == (tag == "graph")
            ctl.run(6)
            torch.cuda.synchronize()
            want = {"fork": 1, "step": H, "node": H, "update": 1, "plant_step": 1, "policy_fork": 1, "infer": H + 1,
                    "policy_act": H, "policy_terminal": 1, "policy_compose": 1}
            if tag == "graph":
                assert ctl.graph_launches == {k: 2 * v for k, v in want.items()}
            assert ctl.launches == {k: 6 * v for k, v in want.items()}
            assert rig.plant.step_count == 6 and rig.model.step_count == 6 * H and int(ctl.tick[0]) == 6
            assert (rig.plant.num_steps, rig.model.num_steps) == (6, 6 * H)      # replayed or eager: the steps the handles took
            runs.append(([_np(t) for t in ctl.tensors()], _np(rig.plant.state), _np(rig.model.state), _np(ctl.plant_h),
                         _np(ctl.plant_c)))
        finally:
            rig.close()
    (ta, pa, ma, ha, ca), (tb, pb, mb, hb, cb) = runs
    assert len(ta) == len(tb) >= 17
    for i, (a, b) in enumerate(zip(ta, tb)):
        assert _same(a, b), i
    assert _same(pa, pb) and _same(ma, mb) and _same(ha, hb) and _same(ca, cb)
    assert np.abs(ta[0]).max() > 0 and np.abs(ha).max() > 0                      # (the residual and the policy's state moved)


# ------------------------------------------------------------------------------------------------------------ 7. it plans
def test_it_plans():
    """DESIGN.md section 24's "it controls" configuration (free space, the Position and Rail Limit reward weights 1 and every
    other weight 0 on both handles, no target-reached reset, ACTION_DELAY 1, the configuration's own episode length, H = 12,
    lambda 0.05, 60 control steps from one plant step on action zero) with the freshly initialised network as the policy.  The
    policy alone (sigma = 0) against ``policy=`` with section 24's sigma 0.5: on every plant the summed reward with planning must
    be higher.  K = 128 in both runs: N = 4 K must be a multiple of 512, so the K = 2 that would do for the policy alone is
    refused, and with sigma = 0 every sample is the policy whatever K is.  The float64 oracle with the numpy statements and the
    PyTorch network in float64 (scripts/mpc_policy_oracle_check.py) satisfies the inequality at this K -- planned / alone =
    0.035, 0.023, 0.026, 0.040 of a negative reward -- so K was not raised; profiles/mpc_policy/it_plans.txt holds both sets."""
    M, K, H = 4, 128, 12
    weights = {k: 0.0 for k in load_config(overrides=["num_envs=%d" % M])["task"]["env"] if k.endswith("_REWARD_WEIGHT")}
    weights.update(POSITION_REWARD_WEIGHT=1.0, RAIL_LIMIT_REWARD_WEIGHT=1.0)
    over = dict(weights, USE_TARGET_REACHED_RESET=False, ACTION_DELAY=1)
    totals = {}
    for sigma in (0.5, 0.0):
        rig = Rig(M, K, H, cost=weights, plant_over=over, max_len=None, sigma=sigma, lam=0.05, seed=1)
        try:
            ctl, plant = rig.ctl, rig.plant
            plant.step_into(ctl.plant_actions, ctl.plant_obs)              # one plant step on action zero
            total = torch.zeros(M, dtype=torch.float64, device=plant.device)
            for _ in range(60):
                ctl.run(1)
                total += plant.rew_buf
            totals[sigma] = _np(total)
            if sigma == 0.0:
                assert not ctl.nominal.any()                               # the residual stayed zero: the policy alone
        finally:
            rig.close()
    print("summed plant reward: policy + planning %s; policy alone %s; ratio %s" % (
        totals[0.5], totals[0.0], totals[0.5] / totals[0.0]))
    assert np.all(totals[0.5] > totals[0.0]), (totals[0.5], totals[0.0])


# ------------------------------------------------------------------------------------------------- 8., 9. play, mpc.py
def test_the_command_line_with_a_policy(tmp_path):
    """``mpc.py``'s main with ``policy=`` on a checkpoint saved here: the header names it, the result holds the path and the
    launch counts, with and without a terminal value."""
    import importlib.util
    from vine_robot_isaacgymenvs_amd.learning.network import ModelA2CContinuousLogStd
    spec = importlib.util.spec_from_file_location("mpc_cli", os.path.join(REPO, "mpc.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["task.env.maxEpisodeLength=8", "task.env.CREATE_PIPE=False", "task.task.vine_randomize=False", "seed=3"]
    cfg = load_config(overrides=["num_envs=2"] + base)
    params = cfg["train"]["params"]
    torch.manual_seed(4)
    from vine_robot_isaacgymenvs_amd.tasks.vine5link_moving_base import ObservationType, num_observations
    width = num_observations(ObservationType[cfg["task"]["env"]["OBSERVATION_TYPE"]])
    model = ModelA2CContinuousLogStd(params["network"], 2, (width,),
                                     params["config"].get("normalize_value", False), params["config"]["normalize_input"])
    ckpt = str(tmp_path / "policy.pth")
    torch.save({"model": model.state_dict()}, ckpt)
    H = 3
    argv = ["plants=2", "samples=256", "horizon=%d" % H, "steps=6", "sigma=[0.5, 0.25]", "lambda=0.1", "out=%s" % tmp_path,
            "task.env.EPISODE_LOG=True", "policy=%s" % ckpt] + base
    out = cli.main(argv)
    assert out["policy"] == ckpt and out["graphed"] and np.isfinite(out["plant_return"]).all()
    assert out["launches"] == {"fork": 6, "step": 6 * H, "node": 6 * H, "update": 6, "plant_step": 6, "policy_fork": 6,
                               "infer": 6 * H, "policy_act": 6 * H, "policy_terminal": 0, "policy_compose": 6}
    out2 = cli.main(argv + ["terminal_value=0.5"])
    assert out2["launches"]["infer"] == 6 * (H + 1) and out2["launches"]["policy_terminal"] == 6
    assert np.isfinite(out2["plant_return"]).all()
    from vine_robot_isaacgymenvs_amd.utils.config import ConfigError
    with pytest.raises(ConfigError, match="multiple of 512"):
        cli.main(["plants=2", "samples=64", "policy=%s" % ckpt] + base)


def test_without_a_policy_nothing_changes():
    """``play`` without ``policy=``: the summed plant reward and the launch counts of tests/golden/mpc_play_no_adapt.json
    (recorded before MPC_ADAPT with the same call), bit for bit."""
    with open(os.path.join(REPO, "tests", "golden", "mpc_play_no_adapt.json")) as f:
        want = json.load(f)["plain"]
    from vine_robot_isaacgymenvs_amd import load_task_config
    c = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=4"])
    c["seed"] = 9
    c["task"]["vine_randomize"] = False
    c["env"].update(CREATE_PIPE=False, CREATE_SHELF=False, maxEpisodeLength=10)
    out = mpc.play(c, samples=16, horizon=6, steps=12, lam=0.05, sigma=[0.5, 0.25], seed=3)
    assert [int(x) for x in out["plant_return"].view(np.uint64)] == want["plant_return_bits"]
    assert out["launches"] == want["launches"] == {"fork": 12, "step": 72, "node": 72, "update": 12, "plant_step": 12}
    assert "policy" not in out and "adapt" not in out
