"""MPC_ENSEMBLE on the GPU (include/vine_mpc_ensemble.h, utils/mpc_ensemble.py): the node's actions bit for bit at every step of
the window and nothing outside it; the update with one member against ``vine_mpc_update``, bit for bit; the update with several
against ``ensemble_replay`` with every branch and every risk; ``EnsembleController`` with identical members against the plain
controller of as many samples as it has sequences, bit for bit after every control step; the captured graph against eager
launches; ``play`` through the command line.

Shapes (M plants, K samples, H steps) are those of tests/test_mpc_gpu.py with a number of members E that divides K:
(5, 14, 12) with E = 2 -- 7 groups, K < 64; (2, 300, 3) with E = 3 and E = 4 -- 100 and 75 groups, K above one workgroup and no
multiple of 256; (1, 2, 1) with E = 2 -- one group, the degenerate end; and every shape with E = 1.  The update also runs at
(1, 2052, 2) with E = 2 and E = 1 -- 1026 and 2052 groups: above 1024 groups per plant the launch function takes the update's other
instantiation.  Plant 0's tick lies above 2^32.  "Bit-identical" is literal: floats are compared as words."""
import numpy as np
import pytest
import torch

from tests.test_env_sensor_gpu import guarded
from tests.test_mpc_gpu import SENTINEL, SHAPES, Rig, _plant_cfg, _same, _stream
from vine_robot_isaacgymenvs_amd import abi
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_ensemble

pytestmark = pytest.mark.gpu

F = abi
TICKS = [(1 << 33) + 9, 0, 4, 2, (1 << 40) + 5]          # plant 0's, so at every shape, above 2^32: the counter's high word is used
SEVERAL = [(SHAPES[0], 2), (SHAPES[1], 3), (SHAPES[1], 4), (SHAPES[2], 2)]
ONE = [(shape, 1) for shape in SHAPES]
# more than 1024 groups per plant: the update is launched as its second instantiation, which holds no weight in registers
BEYOND = (1, 2052, 2)
RISKS = [("mean", None), ("max", None), ("entropic", 0.7)]


def _id(case):
    (M, K, H), E = case
    return "%dx%dx%d-E%d" % (M, K, H, E)


# The largest relative deviation of the device's ENTROPIC group cost from group_costs' float64 over the update's cases, measured
# on an MI355X (profiles/mpc_ensemble/entropic_error.txt), and the bound asserted: four times that -- each term carries one exp
# rounding and the sum one log rounding, and other inputs round otherwise -- and never looser than 1e-12.
ENTROPIC_MEASURED = 2.195e-15
ENTROPIC_BOUND = min(4.0 * ENTROPIC_MEASURED, 1e-12)


class EnsembleRig(Rig):
    """``Rig`` of tests/test_mpc_gpu.py with the ensemble's configuration, and the buffers the two launches write between guard
    elements."""

    def __init__(self, M, K, H, E, risk="mean", theta=None, **kw):
        super().__init__(M, K, H, **kw)
        self.E, self.G = E, K // E
        self.spec = {"params": {"DAMPING": 0.02}, "MEMBERS": E, "RISK": risk}
        if theta is not None:
            self.spec["THETA"] = theta
        self.ecfg = mpc_ensemble.ensemble_struct(self.spec, self.mcfg)
        self.actions_whole, self.actions, self.guard = guarded((self.N, 2), torch.float32, self.dev, fill=SENTINEL)
        self.weights_whole, self.weights, _ = guarded((self.N,), torch.float64, self.dev, fill=SENTINEL)
        self.gcost_whole, self.group_cost, _ = guarded((M * self.G,), torch.float64, self.dev, fill=SENTINEL)
        self.tick.copy_(torch.as_tensor(TICKS[:M]))

    def check(self, rc):
        assert rc == abi.OK, self.lib.vine_last_error()

    def ensemble_node(self):
        self.check(self.lib.vine_mpc_ensemble_scheduled(self.model.h, self.mcfg, self.ecfg, self.nominal.data_ptr(),
                                                        self.tick.data_ptr(), self.window.data_ptr(), self.actions.data_ptr(),
                                                        _stream(self.dev)))

    def ensemble_update(self, weights=True, group_cost=True):
        self.check(self.lib.vine_mpc_ensemble_update(
            self.model.h, self.mcfg, self.ecfg, self.cost.data_ptr(), self.plant.reset_t.data_ptr(), self.nominal.data_ptr(),
            self.history.data_ptr(), self.tick.data_ptr(), self.plant_actions.data_ptr(),
            self.weights.data_ptr() if weights else None, self.group_cost.data_ptr() if group_cost else None, _stream(self.dev)))

    def guards_stand(self):
        for whole, view in ((self.actions_whole, self.actions), (self.weights_whole, self.weights), (self.gcost_whole, self.group_cost)):
            w = whole.cpu().numpy()
            pad = (len(w) - view.numel()) // 2
            if not (np.all(w[:pad] == w.dtype.type(self.guard)) and np.all(w[-pad:] == w.dtype.type(self.guard))):
                return False
        return True


# -------------------------------------------------------------------------------------------------------------- the node
@pytest.mark.parametrize("case", SEVERAL + ONE, ids=_id)
def test_node_bit_for_bit_inside_the_window_and_nothing_outside(case):
    """The nominal reaches close to clipActions, so groups are driven into the clamp on both sides.  The model's step count is
    set, not stepped to: k = c - window[0] for c = window - 1 .. window + H.  With E = 1 the base node's words are in the buffer
    when the launch runs, and stay."""
    (M, K, H), E = case
    rig = EnsembleRig(M, K, H, E)
    try:
        G = K // E
        rng = np.random.default_rng(7 * M + K)
        nominal = rng.uniform(-0.95, 0.95, (M, H, 2)).astype(np.float32) * np.float32(rig.clip)
        rig.nominal.copy_(torch.as_tensor(nominal))
        tick = rig.tick.cpu().numpy()
        ug = mpc_ensemble.group_actions(nominal, rig.sigma, rig.seed, K, E, tick, rig.clip)
        u = mpc_ensemble.member_actions(ug, E).reshape(M * K, H, 2)
        clip = np.float32(rig.clip)
        if G * H >= 36:                                                    # the clamp is reached on both sides, and not by every group
            assert ug.max() == clip and ug.min() == -clip and (np.abs(ug) < clip).any()
        W = 40
        rig.window.fill_(W)
        for k in range(-1, H + 1):
            rig.model.step_count = W + k
            rig.actions.fill_(SENTINEL)
            if E == 1 and 1 <= k < H:                                      # the base node's words first
                rig.node()
                torch.cuda.synchronize()
                left = rig.actions.cpu().numpy().copy()
                assert _same(left, u[:, k]), k
            rig.ensemble_node()
            torch.cuda.synchronize()
            got = rig.actions.cpu().numpy()
            if 0 <= k < H:
                assert _same(got, u[:, k]), k
                members = got.reshape(M, G, E, 2)
                assert all(_same(members[:, :, m], members[:, :, 0]) for m in range(E)), k      # a group's members: identical words
                assert _same(members[:, 0, 0], np.clip(nominal[:, k], -clip, clip)), k              # group 0: the clamped nominal
            else:
                assert np.all(got == np.float32(SENTINEL)), k
            assert rig.guards_stand(), k
        assert rig.model.step_count == W + H and _same(rig.nominal.cpu().numpy(), nominal)
        if E > 1 and G > 1:                                                # the counter is the group's index, not the leader's env
            assert not _same(ug[:, 1], mpc.sample_actions(nominal, rig.sigma, rig.seed, K, tick, rig.clip)[:, E])
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------ the update
def _update_inputs(M, K, H, E):
    """The cases of tests/test_mpc_gpu.py test_update_against_the_replay, by groups: a planted +inf in one member of one group of
    plant 0; plant 1 without a finite cost; plant 2's reset consumed; plant 3's group 0 far below the rest."""
    G = K // E
    rng = np.random.default_rng(M * 1000 + K + E)
    cost = rng.uniform(0.0, 0.6, (M, K))
    planted = None
    if G > 1:
        planted = (int(rng.integers(1, G - 1)) if G > 2 else 1, int(rng.integers(0, E)))
        cost[0, planted[0] * E + planted[1]] = np.inf
    reset = np.zeros(M, dtype=np.int64)
    if M >= 2:
        cost[1, :] = np.inf
    if M >= 3:
        reset[2] = 1
        cost[3, E:] += 50.0
    nominal = rng.uniform(-0.9, 0.9, (M, H, 2)).astype(np.float32)
    history = rng.uniform(-1, 1, (M, F.MAX_DELAY, 2)).astype(np.float32)
    tick = rng.integers(0, 1 << 34, M)
    tick[0] = TICKS[0]
    return cost, planted, reset, nominal, history, tick


def _load(rig, cost, reset, nominal, history, tick):
    rig.cost.copy_(torch.as_tensor(cost.reshape(-1)))
    rig.nominal.copy_(torch.as_tensor(nominal))
    rig.history.copy_(torch.as_tensor(history))
    rig.tick.copy_(torch.as_tensor(tick))
    rig.plant.reset_t.copy_(torch.as_tensor(reset))
    rig.plant_actions.fill_(SENTINEL)
    rig.weights.fill_(SENTINEL)


@pytest.mark.parametrize("risk,theta", RISKS, ids=[r for r, _ in RISKS])
@pytest.mark.parametrize("shape", SHAPES + [BEYOND], ids=["5x14x12", "2x300x3", "1x2x1", "1x2052x2"])
def test_update_with_one_member_is_the_base_update_bit_for_bit(shape, risk, theta):
    M, K, H = shape
    rig = EnsembleRig(M, K, H, 1, risk, theta, sigma=(0.5, 0.75))
    try:
        cost, _, reset, nominal, history, tick = _update_inputs(M, K, H, 1)
        outs = []
        for launch in (rig.update, rig.ensemble_update):
            _load(rig, cost, reset, nominal, history, tick)
            launch()
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy().copy() for t in (rig.nominal, rig.plant_actions, rig.history, rig.tick, rig.weights)])
        for name, a, b in zip(("nominal", "plant_actions", "history", "tick", "weights"), *outs):
            assert _same(a, b), name
        assert _same(rig.group_cost.cpu().numpy(), cost.reshape(-1)) and rig.guards_stand()
        assert outs[1][4].max() == 1.0 and np.isfinite(outs[1][0]).all()
    finally:
        rig.close()


@pytest.mark.parametrize("risk,theta", RISKS, ids=[r for r, _ in RISKS])
@pytest.mark.parametrize("case", SEVERAL + [(BEYOND, 2)], ids=_id)
def test_update_against_the_replay(case, risk, theta):
    """The replay is fed the device's own inputs.  ``group_cost`` exact for MEAN and MAX (the same operations in the same order)
    and within ENTROPIC_BOUND relative for ENTROPIC; the weights within 1e-12 relative of weights recomputed in numpy from the
    DEVICE's group costs (the tolerance of tests/test_mpc_gpu.py; this keeps the two comparisons apart); the new nominal and the
    plant's action within one float32 ulp at clipActions; history, tick, the reset branch, the branch without a finite group cost
    and the planted +inf exact; two runs the same bits; the optional outputs may be left out."""
    (M, K, H), E = case
    G = K // E
    rig = EnsembleRig(M, K, H, E, risk, theta, sigma=(0.5, 0.75))
    try:
        cost, planted, reset, nominal, history, tick = _update_inputs(M, K, H, E)
        outs = []
        for given in (True, True, False):
            _load(rig, cost, reset, nominal, history, tick)
            rig.ensemble_update(weights=given, group_cost=given)
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy().copy() for t in (rig.nominal, rig.plant_actions, rig.history, rig.tick, rig.weights,
                                                          rig.group_cost)])
        for a, b in zip(outs[0], outs[1]):
            assert _same(a, b)
        for a, b in zip(outs[0][:4], outs[2][:4]):                         # without the optional outputs: the same update
            assert _same(a, b)
        assert np.all(outs[2][4] == SENTINEL) and rig.guards_stand()
        got_nominal, got_act, got_history, got_tick, got_w, got_c = outs[0]
        got_c = got_c.reshape(M, G)
        r = mpc_ensemble.ensemble_replay(nominal, cost.reshape(-1), rig.sigma, rig.lam, rig.seed, tick, rig.clip, E, risk, theta,
                                         reset, history)
        want_c = r["group_cost"]
        assert np.array_equal(np.isfinite(got_c), np.isfinite(want_c)) and np.all(np.isposinf(got_c[~np.isfinite(want_c)]))
        fin = np.isfinite(want_c)
        if risk == "entropic":
            dev = (np.abs(got_c[fin] - want_c[fin]) / np.abs(want_c[fin])).max() if fin.any() else 0.0
            print("ENTROPIC group_cost: largest relative deviation from the float64 replay %.3e (%s)" % (dev, _id(case)))
            assert dev <= ENTROPIC_BOUND
        else:
            assert _same(got_c, want_c)
        own = mpc_ensemble.ensemble_replay(nominal, cost.reshape(-1), rig.sigma, rig.lam, rig.seed, tick, rig.clip, E, risk, theta,
                                           reset, history, group_cost=got_c)
        w = got_w.reshape(M, K)
        assert np.all(np.abs(w - own["member_weights"]) <= 1e-12 * own["member_weights"])
        assert all(_same(w.reshape(M, G, E)[:, :, m], w.reshape(M, G, E)[:, :, 0]) for m in range(E))
        ulp = 2.0 ** -23 * rig.clip
        assert np.abs(got_nominal.astype(np.float64) - r["nominal"]).max() <= ulp
        assert np.abs(got_act.astype(np.float64) - r["plant_actions"]).max() <= ulp
        assert _same(got_history[:, 1:], history[:, :-1]) and _same(got_history[:, 0], got_act)
        assert np.array_equal(got_tick, tick + 1)
        wg = w.reshape(M, G, E)[:, :, 0]
        if planted is not None:                                            # its group's weight is 0 and its neighbours' are not
            g = planted[0]
            assert np.isposinf(got_c[0, g]) and wg[0, g] == 0.0 and wg[0, g - 1] > 0.0 and (g + 1 >= G or wg[0, g + 1] > 0.0)
            assert wg[0].max() == 1.0 and (wg[0] == 0.0).sum() == 1
        if M >= 2:                                                         # no finite group cost: exact
            assert not w[1].any() and _same(got_act[1], nominal[1, 0]) and _same(got_nominal[1, :-1], nominal[1, 1:])
            assert _same(got_nominal[1, -1], nominal[1, -1]) and np.all(np.isposinf(got_c[1]))
        if M >= 3:
            assert _same(got_act[2], np.zeros(2, np.float32)) and _same(got_nominal[2], np.zeros((H, 2), np.float32))
            assert _same(got_act[3], r["u"][3, 0, 0]) and wg[3, 0] == 1.0 and not wg[3, 1:].any()
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------ the task classes
def _ensemble_pair(M, K, H, ensemble, members=None, cost=None, plant_over=None, **ctl):
    """A plant, a model whose tables the spec's ``params`` bind, and the controller; ``members``: ``{name: [M, E]}`` to set."""
    cfg = _plant_cfg(M, **(plant_over or {}))
    plant = mpc.make_task(cfg)
    mcfg = mpc.model_config(cfg, M, K, cost)
    mcfg["env"]["ENV_PARAMS"] = dict(ensemble["params"])
    model = mpc.make_task(mcfg)
    c = mpc_ensemble.EnsembleController(plant, model, K, ensemble, H, **ctl)
    if members is not None:
        c.set_members(members)
    return plant, model, c


def test_identical_members_are_the_plain_controller_bit_for_bit():
    """M = 2, K = 14, E = 2, H = 3, RISK mean and every member's DAMPING one number, beside ``mpc.Controller`` with samples = 7 whose
    model has that DAMPING in its table: the same seed and plants.  Both models step on the same kernel.  After each of four
    eager control steps the plant's action, the nominal and the plant's state are equal in every bit: the counter's first word
    is the group's index, (c + c) / 2 is c, and a sequence's members are the plain controller's sample twice."""
    M, K, E, H, damping = 2, 14, 2, 3, 0.03
    G = K // E
    spec = {"params": {"DAMPING": damping}, "MEMBERS": E, "RISK": "mean"}
    plant_a, model_a, ctl = _ensemble_pair(M, K, H, spec, members={"DAMPING": np.full((M, E), damping)}, seed=5, sigma=[0.5, 0.25],
                                           graph=False, keep_weights=True)
    cfg = _plant_cfg(M)
    mcfg = mpc.model_config(cfg, M, G)
    mcfg["env"]["ENV_PARAMS"] = {"DAMPING": damping}
    plant_b, model_b = mpc.make_task(cfg), mpc.make_task(mcfg)
    try:
        base = mpc.Controller(plant_b, model_b, G, H, seed=5, sigma=[0.5, 0.25], graph=False, keep_weights=True)
        base.set_model_params({"DAMPING": damping})
        assert model_a.step_kernel_name == model_b.step_kernel_name and model_a.env_params is not None
        for step in range(4):
            base.run(1)
            ctl.run(1)
            torch.cuda.synchronize()
            members = model_a.state.cpu().numpy().reshape(F.VF_COUNT, M, G, E)
            plain = model_b.state.cpu().numpy().reshape(F.VF_COUNT, M, G)
            for m in range(E):                                             # a sequence's members are the plain sample
                assert _same(members[..., m], plain), (step, m)
            assert _same(ctl.cost.cpu().numpy().reshape(M, G, E)[:, :, 0], base.cost.cpu().numpy().reshape(M, G)), step
            assert _same(ctl.group_cost.cpu().numpy(), base.cost.cpu().numpy()), step
            for name in ("plant_actions", "nominal", "history", "tick"):
                assert _same(getattr(base, name).cpu().numpy(), getattr(ctl, name).cpu().numpy()), (step, name)
            assert _same(plant_a.state.cpu().numpy(), plant_b.state.cpu().numpy()), step
        assert np.abs(ctl.nominal.cpu().numpy()).max() > 0                 # (it moved)
        assert ctl.launches == dict(base.launches, ensemble=4 * (H + 1))
    finally:
        for t in (model_a, plant_a, model_b, plant_b):
            t.close()


def test_captured_control_steps_against_eager_ones():
    """E = 4, RISK entropic, members that differ in DAMPING and ACTION_DELAY: three captured control steps (one per replay) against
    three eager ones; every controller tensor and both state blocks bit-identical."""
    M, K, H, E = 4, 16, 6, 4
    spec = {"params": {"DAMPING": [0.005, 0.1], "ACTION_DELAY": {"values": [0, 2]}}, "MEMBERS": E, "RISK": "entropic", "THETA": 0.5}
    rng = np.random.default_rng(4)
    members = {"DAMPING": rng.uniform(0.005, 0.1, (M, E)), "ACTION_DELAY": rng.integers(0, 2, (M, E)) * 2.0}
    runs = []
    for tag, kw in (("graph", dict(graph=True)), ("eager", dict(graph=False))):
        plant, model, ctl = _ensemble_pair(M, K, H, spec, members=members, plant_over=dict(maxEpisodeLength=10), seed=5,
                                           keep_weights=True, **kw)
        try:
            assert ctl.use_graph == (tag == "graph") and any(t is ctl.group_cost for t in ctl.tensors())
            ctl.run(3)
            torch.cuda.synchronize()
            if tag == "graph":
                assert ctl.graph_launches == {"fork": 1, "step": H, "node": H, "update": 1, "plant_step": 1, "ensemble": H + 1}
            assert ctl.launches == {"fork": 3, "step": 3 * H, "node": 3 * H, "update": 3, "plant_step": 3, "ensemble": 3 * (H + 1)}
            assert plant.step_count == 3 and model.step_count == 3 * H and int(ctl.tick[0]) == 3
            table = model.env_params.cpu().numpy()
            assert _same(table[abi.VP_DAMPING].reshape(M, K // E, E), np.broadcast_to(np.float32(members["DAMPING"])[:, None], (M, K // E, E)))
            c = ctl.cost.cpu().numpy().reshape(M, K // E, E)
            assert np.isfinite(c).all() and (c.max(axis=2) > c.min(axis=2)).any()       # the members disagree
            runs.append(([t.cpu().numpy().copy() for t in ctl.tensors()], plant.state.cpu().numpy().copy(),
                         model.state.cpu().numpy().copy()))
        finally:
            model.close()
            plant.close()
    (ta, pa, ma), (tb, pb, mb) = runs
    assert len(ta) == len(tb) >= 12
    for a, b in zip(ta, tb):
        assert _same(a, b)
    assert _same(pa, pb) and _same(ma, mb)
    assert np.abs(ta[0]).max() > 0                                         # (the nominal moved)


def test_play_and_the_command_line_with_an_ensemble(tmp_path):
    import importlib.util
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mpc_cli", os.path.join(repo, "mpc.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    M, K, H, E = 2, 16, 3, 4
    argv = ["plants=%d" % M, "samples=%d" % K, "horizon=%d" % H, "steps=4", "out=%s" % tmp_path, "task.env.CREATE_PIPE=False",
            "task.task.vine_randomize=False", "seed=3"]
    out = cli.main(argv + ["ensemble={params: {DAMPING: [0.005, 0.1], ACTION_DELAY: {values: [0, 2]}}, MEMBERS: 4, RISK: max}"])
    assert out["graphed"] and out["model_table_bound"] and np.isfinite(out["plant_return"]).all()
    assert out["launches"] == {"fork": 4, "step": 4 * H, "node": 4 * H, "update": 4, "plant_step": 4, "ensemble": 4 * (H + 1)}
    ens = out["ensemble"]
    assert (ens["MEMBERS"], ens["RISK"], ens["THETA"], ens["SEED"]) == (E, "max", None, 4)
    assert ens["params"] == {"DAMPING": [0.005, 0.1], "ACTION_DELAY": {"values": [0.0, 2.0]}}
    assert set(ens["members"]) == set(ens["values"]) == {"DAMPING", "ACTION_DELAY"}
    for name, values in ens["values"].items():
        assert values.shape == (M, E)
        st = ens["members"][name]
        assert st["min"] == values.min() and st["max"] == values.max() and np.isclose(st["mean"], values.mean())
        # the model's table, read back from the device: each plant's E values tiled over its K / E groups
        assert _same(ens["model_table"][name].reshape(M, K // E, E), np.broadcast_to(np.float32(values)[:, None], (M, K // E, E))), name
    assert 0.005 <= ens["members"]["DAMPING"]["min"] < ens["members"]["DAMPING"]["max"] <= 0.1
    assert set(np.unique(ens["values"]["ACTION_DELAY"])) <= {0.0, 2.0} and ens["disagreement"] >= 0.0
    plain = cli.main(argv)
    assert "ensemble" not in plain and set(plain["launches"]) == {"fork", "step", "node", "update", "plant_step"}
