"""MPC_NOISE on the GPU (include/vine_mpc_noise.h, utils/mpc_noise.py): the drawn table bit for bit against numpy and between
guard rows; the node's actions bit for bit at every step of the window and nothing outside it; the update against
``noise_replay`` with every branch; ``NoiseController`` with BETA 0 against the plain controller, bit for bit after every
control step; the captured graph against eager launches; the command line.

Shapes (M plants, K samples, H steps) are those of tests/test_mpc_gpu.py: (5, 14, 12) = 70 model envs, two waves, the second
partial, K < 64; (2, 300, 3) = K above one workgroup of the update and no multiple of 256; (1, 2, 1) the degenerate end.
"Bit-identical" is literal: floats are compared as words."""
import numpy as np
import pytest
import torch

from tests.test_env_sensor_gpu import guarded
from tests.test_mpc_gpu import SENTINEL, SHAPES, Rig, _pair, _plant_cfg, _same, _stream
from vine_robot_isaacgymenvs_amd import abi
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_noise

pytestmark = pytest.mark.gpu

F = abi
IDS = ["5x14x12", "2x300x3", "1x2x1"]
UNWRITTEN = -5555.0
ADAPT = {"RATE": 0.25, "SIGMA_MIN": [0.05, 0.1], "SIGMA_MAX": [1.0, 0.9]}
TICKS = [(1 << 33) + 9, 0, 4, 2, (1 << 40) + 5]          # plant 0's, so at every shape, above 2^32: the counter's high word is used


class NoiseRig(Rig):
    """``Rig`` of tests/test_mpc_gpu.py with the table between guard rows and the amplitudes."""

    def __init__(self, M, K, H, beta=(0.8, 0.5), adapt=None, **kw):
        super().__init__(M, K, H, **kw)
        self.spec = mpc_noise.noise_config({"BETA": list(beta), "ADAPT": adapt})
        self.ncfg = mpc_noise.noise_struct(self.spec, self.mcfg)
        self.eps_whole, self.eps, self.guard = guarded((H, self.N, 2), torch.float32, self.dev, fill=UNWRITTEN)
        self.sigma_p = torch.tensor(self.sigma, dtype=torch.float32, device=self.dev).repeat(M, 1).contiguous()
        self.tick.copy_(torch.as_tensor(TICKS[:M]))

    def check(self, rc):
        assert rc == abi.OK, self.lib.vine_last_error()

    def draw(self):
        self.check(self.lib.vine_mpc_noise_draw(self.model.h, self.mcfg, self.ncfg, self.tick.data_ptr(), self.eps.data_ptr(),
                                                _stream(self.dev)))

    def noise_node(self):
        self.check(self.lib.vine_mpc_noise_scheduled(self.model.h, self.mcfg, self.ncfg, self.nominal.data_ptr(),
                                                     self.window.data_ptr(), self.eps.data_ptr(), self.sigma_p.data_ptr(),
                                                     self.actions.data_ptr(), _stream(self.dev)))

    def noise_update(self):
        self.check(self.lib.vine_mpc_noise_update(
            self.model.h, self.mcfg, self.ncfg, self.cost.data_ptr(), self.plant.reset_t.data_ptr(), self.eps.data_ptr(),
            self.nominal.data_ptr(), self.history.data_ptr(), self.tick.data_ptr(), self.plant_actions.data_ptr(),
            self.sigma_p.data_ptr(), self.weights.data_ptr(), _stream(self.dev)))

    def table(self):
        """[M, K, H, 2]: the numpy statement of the table at the rig's ticks."""
        return mpc_noise.colored_deviate(self.seed, self.M, self.K, self.tick.cpu().numpy(), self.H, self.spec["BETA"])

    def guards_stand(self):
        whole = self.eps_whole.cpu().numpy()
        pad = (len(whole) - self.H * self.N * 2) // 2
        return np.all(whole[:pad] == np.float32(self.guard)) and np.all(whole[-pad:] == np.float32(self.guard))


# -------------------------------------------------------------------------------------------------------------- the draw
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_draw_bit_for_bit_between_guard_rows(shape):
    M, K, H = shape
    rig = NoiseRig(M, K, H)
    try:
        rig.draw()
        torch.cuda.synchronize()
        got = rig.eps.cpu().numpy()
        want = rig.table()
        assert _same(got, mpc_noise.table_layout(want))
        assert not np.any(got == np.float32(UNWRITTEN)) and rig.guards_stand()          # all of [H][N][2] and nothing else
        assert not got.reshape(H, M, K, 2)[:, :, 0].any()                               # sample 0 of every plant
        assert np.count_nonzero(got.reshape(H, M, K, 2)[:, :, 1:]) >= 2 * H * M * (K - 1) - 4
        # the same launch with BETA 0: the base deviate's words
        rig.ncfg.beta[0] = rig.ncfg.beta[1] = 0.0
        rig.draw()
        torch.cuda.synchronize()
        z = mpc.noise_deviate(rig.seed, M, K, rig.tick.cpu().numpy(), H)
        assert _same(rig.eps.cpu().numpy(), mpc_noise.table_layout(z)) and rig.guards_stand()
        if H > 1 and K > 2:
            assert not _same(got, rig.eps.cpu().numpy())
    finally:
        rig.close()


# -------------------------------------------------------------------------------------------------------------- the node
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_node_bit_for_bit_inside_the_window_and_nothing_outside(shape):
    """The table is numpy's own; sigma_p differs per plant; the nominal reaches close to clipActions, so samples are driven into
    the clamp on both sides.  The model's step count is set, not stepped to: k = c - window[0] for c = window - 1 .. window + H."""
    M, K, H = shape
    rig = NoiseRig(M, K, H)
    try:
        rng = np.random.default_rng(7 * M + K)
        nominal = rng.uniform(-0.95, 0.95, (M, H, 2)).astype(np.float32) * np.float32(rig.clip)
        sigma_p = rng.uniform(0.1, 0.9, (M, 2)).astype(np.float32)
        table = rig.table()
        rig.nominal.copy_(torch.as_tensor(nominal))
        rig.sigma_p.copy_(torch.as_tensor(sigma_p))
        rig.eps.copy_(torch.as_tensor(mpc_noise.table_layout(table)))
        u = mpc_noise.colored_actions(nominal, sigma_p, table, rig.clip).reshape(M * K, H, 2)
        if K > 2:                                                          # the clamp is reached, and not by every sample
            assert np.abs(u).max() == np.float32(rig.clip) and (np.abs(u) < np.float32(rig.clip)).any()
        W = 40
        rig.window.fill_(W)
        for k in range(-1, H + 1):
            rig.model.step_count = W + k
            rig.actions.fill_(SENTINEL)
            rig.noise_node()
            torch.cuda.synchronize()
            got = rig.actions.cpu().numpy()
            if 0 <= k < H:
                assert _same(got, u[:, k]), k
            else:
                assert np.all(got == np.float32(SENTINEL)), k
        assert rig.model.step_count == W + H and _same(rig.eps.cpu().numpy(), mpc_noise.table_layout(table))
        # sample 0 is the (clamped) nominal itself
        assert _same(u.reshape(M, K, H, 2)[:, 0], np.clip(nominal, -np.float32(rig.clip), np.float32(rig.clip)))
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------ the update
@pytest.mark.parametrize("adapt", [ADAPT, None], ids=["adapt", "fixed"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_update_against_the_replay(shape, adapt):
    """The cases and tolerances of tests/test_mpc_gpu.py test_update_against_the_replay: weights within 1e-12 relative; the new
    nominal and the plant's action within one float32 ulp at clipActions; sigma_p within one float32 ulp of its value (one
    float32 rounding of two float64 values that agree far below it: the new sum has at most K * H positive terms); history,
    tick, the reset branch, the branch without a finite cost, a planted +inf cost and ``adapt`` off exact; two runs the same
    bits."""
    M, K, H = shape
    rig = NoiseRig(M, K, H, adapt=adapt, sigma=(0.5, 0.75))
    try:
        rng = np.random.default_rng(M * 1000 + K)
        cost = rng.uniform(0.0, 0.6, (M, K))
        planted = int(rng.integers(0, K))
        cost[0, planted] = np.inf
        reset = np.zeros(M, dtype=np.int64)
        if M >= 2:
            cost[1, :] = np.inf                                           # no finite cost: the nominal and sigma_p stay
        if M >= 3:
            reset[2] = 1                                                   # the plant's next step only consumes its reset
            cost[3, 1:] += 50.0                                            # one sample far below the rest
        nominal = rng.uniform(-0.9, 0.9, (M, H, 2)).astype(np.float32)
        history = rng.uniform(-1, 1, (M, F.MAX_DELAY, 2)).astype(np.float32)
        sigma_p = rng.uniform(0.2, 0.8, (M, 2)).astype(np.float32)
        tick = rng.integers(0, 1 << 34, M)
        rig.tick.copy_(torch.as_tensor(tick))
        rig.draw()
        torch.cuda.synchronize()
        table = rig.table()
        assert _same(rig.eps.cpu().numpy(), mpc_noise.table_layout(table))
        outs = []
        for _ in range(2):
            rig.cost.copy_(torch.as_tensor(cost.reshape(-1)))
            rig.nominal.copy_(torch.as_tensor(nominal))
            rig.history.copy_(torch.as_tensor(history))
            rig.tick.copy_(torch.as_tensor(tick))
            rig.sigma_p.copy_(torch.as_tensor(sigma_p))
            rig.plant.reset_t.copy_(torch.as_tensor(reset))
            rig.noise_update()
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy().copy() for t in (rig.nominal, rig.plant_actions, rig.history, rig.tick, rig.weights,
                                                          rig.sigma_p)])
        for a, b in zip(*outs):
            assert _same(a, b)
        got_nominal, got_act, got_history, got_tick, got_w, got_sigma = outs[0]
        r = mpc_noise.noise_replay(nominal, cost.reshape(-1), rig.sigma, rig.lam, rig.seed, tick, rig.clip, rig.spec["BETA"],
                                   sigma_p=sigma_p, adapt=rig.spec["ADAPT"], plant_reset=reset, history=history)
        w = got_w.reshape(M, K)
        assert np.all(np.abs(w - r["weights"]) <= 1e-12 * r["weights"])
        ulp = 2.0 ** -23 * rig.clip
        assert np.abs(got_nominal.astype(np.float64) - r["nominal"]).max() <= ulp
        assert np.abs(got_act.astype(np.float64) - r["plant_actions"]).max() <= ulp
        assert _same(got_history[:, 1:], history[:, :-1]) and _same(got_history[:, 0], got_act)
        assert np.array_equal(got_tick, tick + 1)
        assert w[0, planted] == 0.0 and w[0].max() == 1.0 and (w[0] == 0.0).sum() == 1
        assert _same(rig.eps.cpu().numpy(), mpc_noise.table_layout(table)) and rig.guards_stand()      # the table is read only
        if adapt is None:
            assert _same(got_sigma, sigma_p)                               # never written
        else:
            err = np.abs(got_sigma.astype(np.float64) - r["sigma"].astype(np.float64))
            print("sigma_p: largest error %.3g, in ulps of the value %.3g" % (err.max(), (err / np.spacing(r["sigma"])).max()))
            assert np.all(err <= np.spacing(np.maximum(got_sigma, r["sigma"])))
            assert not _same(got_sigma[0], sigma_p[0])                     # (it moved)
            lo, hi = np.float32(ADAPT["SIGMA_MIN"]), np.float32(ADAPT["SIGMA_MAX"])
            assert np.all(got_sigma >= lo) and np.all(got_sigma <= hi)
        if M >= 2:                                                         # all infinite: exact
            assert not w[1].any() and _same(got_act[1], nominal[1, 0]) and _same(got_nominal[1, :-1], nominal[1, 1:])
            assert _same(got_nominal[1, -1], nominal[1, -1]) and _same(got_sigma[1], sigma_p[1])
        if M >= 3:
            assert _same(got_act[2], np.zeros(2, np.float32)) and _same(got_nominal[2], np.zeros((H, 2), np.float32))
            assert _same(got_sigma[2], np.float32(rig.sigma) if adapt is not None else sigma_p[2])
            assert _same(got_act[3], r["u"][3, 0, 0]) and w[3, 0] == 1.0 and not w[3, 1:].any()
            if adapt is not None:                                          # sample 0 alone: no spread at all, the old variance decays
                want = np.sqrt(0.75) * sigma_p[3].astype(np.float64)
                assert np.all(np.abs(got_sigma[3] - np.clip(want, lo, hi)) <= np.spacing(got_sigma[3]))
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------ the task classes
def _noise_pair(M, K, H, noise, cost=None, plant_over=None, **ctl):
    cfg = _plant_cfg(M, **(plant_over or {}))
    plant = mpc.make_task(cfg)
    model = mpc.make_task(mpc.model_config(cfg, M, K, cost))
    return plant, model, mpc_noise.NoiseController(plant, model, K, noise, H, **ctl)


def test_beta_zero_without_adapt_is_the_plain_controller_bit_for_bit():
    """(5, 14, 12), episodes of four steps so that resets are consumed: ``NoiseController`` with BETA 0 and no ADAPT beside a plain
    ``mpc.Controller`` on the same plants and seed, six control steps, every tensor below equal in every bit after every
    step.  Pins the node's window arithmetic and the update's restatement."""
    M, K, H = SHAPES[0]
    over = dict(maxEpisodeLength=4)
    plant_a, model_a, base = _pair(M, K, H, plant_over=over, seed=5, sigma=[0.5, 0.25], graph=False)
    plant_b, model_b, ctl = _noise_pair(M, K, H, {"BETA": 0.0}, plant_over=over, seed=5, sigma=[0.5, 0.25], graph=False)
    try:
        names = ("actions", "cost", "alive", "nominal", "plant_actions", "history", "tick")
        consumed = 0
        for step in range(6):
            consumed += int((plant_a.reset_buf != 0).sum())
            base.run(1)
            ctl.run(1)
            torch.cuda.synchronize()
            for name in names:
                assert _same(getattr(base, name).cpu().numpy(), getattr(ctl, name).cpu().numpy()), (step, name)
            assert _same(plant_a.state.cpu().numpy(), plant_b.state.cpu().numpy()), step
            assert _same(model_a.state.cpu().numpy(), model_b.state.cpu().numpy()), step
        assert consumed > 0 and np.abs(ctl.nominal.cpu().numpy()).max() > 0                   # resets were consumed; it moved
        assert _same(ctl.sigma_p.cpu().numpy(), np.tile(np.float32([0.5, 0.25]), (M, 1)))
        assert ctl.launches == dict(base.launches, draw=6, noise=6 * (H + 1))
        z = mpc.noise_deviate(5, M, K, ctl.tick.cpu().numpy() - 1, H)
        assert _same(ctl.eps.cpu().numpy(), mpc_noise.table_layout(z))
    finally:
        for t in (model_a, plant_a, model_b, plant_b):
            t.close()


def test_captured_control_steps_against_eager_ones(tmp_path):
    """BETA 0.8 and ADAPT on: four captured control steps replayed five times against twenty eager ones; every controller
    tensor, ``eps`` and ``sigma_p`` included, and both state blocks bit-identical.  Episodes of ten steps, so that resets are
    consumed and ``sigma_p`` rows go back to the configuration's."""
    M, K, H = 4, 16, 6
    noise = {"BETA": [0.8, 0.6], "ADAPT": {"RATE": 0.2, "SIGMA_MIN": 0.05, "SIGMA_MAX": 1.0}}
    runs = []
    for tag, kw in (("graph", dict(graph=True, graph_steps=4)), ("eager", dict(graph=False))):
        plant, model, ctl = _noise_pair(M, K, H, noise, plant_over=dict(maxEpisodeLength=10), seed=5, keep_weights=True, **kw)
        try:
            assert ctl.use_graph == (tag == "graph")
            assert any(t is ctl.eps for t in ctl.tensors()) and any(t is ctl.sigma_p for t in ctl.tensors())
            ctl.run(20)
            torch.cuda.synchronize()
            if tag == "graph":
                assert ctl.graph_launches == {"fork": 4, "step": 4 * H, "node": 4 * H, "update": 4, "plant_step": 4, "draw": 4,
                                              "noise": 4 * (H + 1)}
            assert ctl.launches == {"fork": 20, "step": 20 * H, "node": 20 * H, "update": 20, "plant_step": 20, "draw": 20,
                                    "noise": 20 * (H + 1)}
            assert plant.step_count == 20 and model.step_count == 20 * H and int(ctl.tick[0]) == 20
            sigma = ctl.sigma_p.cpu().numpy()
            assert np.all(sigma >= np.float32(0.05)) and np.all(sigma <= 1.0) and not np.all(sigma == np.float32(0.5))
            runs.append(([t.cpu().numpy().copy() for t in ctl.tensors()], plant.state.cpu().numpy().copy(),
                         model.state.cpu().numpy().copy()))
            ctl.sigma_p.fill_(0.9)
            ctl.reset_plants([1])
            torch.cuda.synchronize()
            assert _same(ctl.sigma_p[1].cpu().numpy(), np.float32([0.5, 0.5])) and float(ctl.sigma_p[0, 0]) == np.float32(0.9)
        finally:
            model.close()
            plant.close()
    (ta, pa, ma), (tb, pb, mb) = runs
    assert len(ta) == len(tb) >= 13
    for a, b in zip(ta, tb):
        assert _same(a, b)
    assert _same(pa, pb) and _same(ma, mb)
    assert np.abs(ta[0]).max() > 0                                         # (the nominal moved)


def test_it_matters():
    """The setting of tests/test_mpc_gpu.py test_it_controls -- free space, the Position and Rail Limit reward weights 1 and every
    other weight 0 on both handles, no target-reached reset, ACTION_DELAY 1; (4, 64, 12), sigma 0.5, lambda 0.05, 60 control
    steps from one plant step on action zero, seed 1 -- with BETA 0.8 beside BETA 0 (the white noise of include/vine_mpc.h, word
    for word), no ADAPT.  The summed plant reward with BETA 0.8 must exceed that with BETA 0 on each of the four plants: the
    float64 oracle with the numpy statements gave that ordering on every plant at each of four seeds, BETA 0.8 ahead by 4.7 % to
    8.7 % per plant at this seed (profiles/mpc_noise/it_matters_oracle.txt).  Only the ordering is asserted."""
    M, K, H = 4, 64, 12
    weights = {k: 0.0 for k in _plant_cfg(M)["env"] if k.endswith("_REWARD_WEIGHT")}
    weights.update(POSITION_REWARD_WEIGHT=1.0, RAIL_LIMIT_REWARD_WEIGHT=1.0)
    over = dict(weights, USE_TARGET_REACHED_RESET=False, ACTION_DELAY=1)
    totals = {}
    for beta in (0.8, 0.0):
        plant, model, ctl = _noise_pair(M, K, H, {"BETA": beta}, cost=weights, plant_over=over, sigma=0.5, lam=0.05, seed=1)
        try:
            plant.step_into(ctl.plant_actions, ctl.plant_obs)              # one plant step on action zero
            total = torch.zeros(M, dtype=torch.float64, device=plant.device)
            for _ in range(60):
                ctl.run(1)
                total += plant.rew_buf
            totals[beta] = total.cpu().numpy()
        finally:
            model.close()
            plant.close()
    print("summed plant reward: BETA 0.8 %s; BETA 0 %s" % (totals[0.8], totals[0.0]))
    assert np.all(totals[0.8] > totals[0.0]), (totals[0.8], totals[0.0])


def test_the_command_line_with_noise(tmp_path):
    import importlib.util
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mpc_cli", os.path.join(repo, "mpc.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    argv = ["plants=4", "samples=64", "horizon=12", "steps=24", "sigma=[0.5, 0.25]", "lambda=0.1", "out=%s" % tmp_path,
            "task.env.EPISODE_LOG=True", "task.env.maxEpisodeLength=10", "task.env.CREATE_PIPE=False",
            "task.task.vine_randomize=False", "seed=3"]
    out = cli.main(argv + ["noise={BETA: [0.9, 0.7], ADAPT: {RATE: 0.2, SIGMA_MIN: 0.05, SIGMA_MAX: 1.0}}"])
    assert out["graphed"] and out["launches"] == {"fork": 24, "step": 24 * 12, "node": 24 * 12, "update": 24, "plant_step": 24,
                                                  "draw": 24, "noise": 24 * 13}
    assert out["report"]["episodes"] >= 4 and np.isfinite(out["plant_return"]).all()
    noise = out["noise"]
    assert noise["BETA"] == [0.9, 0.7] and noise["ADAPT"] == {"RATE": 0.2, "SIGMA_MIN": [0.05, 0.05], "SIGMA_MAX": [1.0, 1.0]}
    for a in range(2):
        assert 0.05 <= noise["sigma_min"][a] <= noise["sigma_mean"][a] <= noise["sigma_max"][a] <= 1.0
    out = cli.main(argv + ["noise={BETA: 0.8}", "steps=6"])
    assert out["noise"]["ADAPT"] is None and out["noise"]["sigma_min"] == out["noise"]["sigma_max"] == [0.5, 0.25]
    plain = cli.main(argv + ["steps=6"])
    assert "noise" not in plain and set(plain["launches"]) == {"fork", "step", "node", "update", "plant_step"}
