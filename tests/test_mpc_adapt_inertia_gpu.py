"""MPC_ADAPT masses on the GPU (include/vine_mpc_adapt_inertia.h, utils/mpc_adapt_inertia.py): the inertia pin's columns against
``inertia_rows(mass_candidates(...))`` with guards on either side of the table; exact recovery (candidates that ARE the plant,
masses included, score 0.0); the mass estimate against ``mass_estimate``; a degenerate mass belief beside the plain adaptive
controller, bit for bit (what keeps the restated estimate from drifting); the captured cycle against eager launches; ``mpc.py``
with ``masses``; and the mass belief moving to the truth.

Shapes (M plants, K samples, W window, D table dimensions, Dm mass dimensions): (5, 14, 6, 1, 3) = 70 model envs, a partial
wave; (2, 300, 3, 1, 1) = a lane stride beyond 256; (1, 2, 1, 1, 1) every extent at its minimum.  Both handles carry both
tables.  "Bit-identical" is literal: floats are compared as words."""
import os

import numpy as np
import pytest
import torch

from tests import test_mpc_adapt_gpu as base_tests
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params, mpc, mpc_adapt
from vine_robot_isaacgymenvs_amd.utils import mpc_adapt_inertia as mai

pytestmark = pytest.mark.gpu

REPO = base_tests.REPO
SENTINEL = base_tests.SENTINEL
_bits, _same, _stream, _cfg = base_tests._bits, base_tests._same, base_tests._stream, base_tests._cfg
SHAPES = [(5, 14, 6, 1, 3), (2, 300, 3, 1, 1), (1, 2, 1, 1, 1)]
IDS = ["5x14x6x1x3", "2x300x3x1x1", "1x2x1x1x1"]
GUARD = 96                                   # floats of sentinel on either side of the model's inertia table
PLANT_MASSES = (1.3, 0.8, 1.5)               # x the configuration's cart mass, LINK_MASS, TIP_LINK_MASS


@pytest.fixture(autouse=True)
def _nothing_left_for_a_later_capture():
    yield
    import gc
    gc.collect()


def _masses(Dm, c):
    if Dm == 3:
        return {"CART_MASS": [0.5 * c, 2.0 * c], "LINK_MASS": [0.7, 1.4], "TIP_LINK_MASS": [0.7, 1.6]}
    return {"LINK_MASS": [0.7, 1.4]}


class MassRig(base_tests.Rig):
    """``Rig`` with an inertia table on both handles -- the plant's carries PLANT_MASSES, the model's the configuration's row,
    inside one buffer with GUARD floats of sentinel on either side -- and the mass belief's buffers."""

    def __init__(self, M, K, W, D, Dm, pipe=False, **spec):
        super().__init__(M, K, W, D, pipe=pipe, **spec)
        lib, d, N = self.lib, self.dev, self.N
        self.Dm = Dm
        self.vcfg = _cfg(N, pipe)
        self.ibase = env_params.inertia_config_row(lib, self.vcfg)
        c = float(self.ibase[abi.VI_CART_MASS])
        self.cart = float(np.float32(PLANT_MASSES[0] * c))
        self.derive = lambda t: env_params.derive_inertia(lib, self.vcfg, t)
        plant = np.repeat(self.ibase[:, None], M, axis=1)
        env_params.set_inertia_rows(plant, self.ibase, {"CART_MASS": np.full(M, self.cart), "LINK_MASS": np.full(M, PLANT_MASSES[1]),
                                                        "TIP_LINK_MASS": np.full(M, PLANT_MASSES[2])})
        self.plant_inertia = env_params.check_inertia_table(lib, self.plant.cfg, env_params.derive_inertia(lib, self.plant.cfg, plant))
        self.plant.inertia_t = torch.as_tensor(self.plant_inertia).to(d).contiguous()
        self.buffer = torch.full((abi.VI_COUNT * N + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=d)
        self.inertia_t = self.buffer[GUARD:GUARD + abi.VI_COUNT * N].view(abi.VI_COUNT, N)
        self.inertia_t.copy_(torch.as_tensor(np.repeat(self.ibase[:, None], N, axis=1)))
        torch.cuda.synchronize(d)
        native.check(lib.vine_bind_env_inertia(self.plant.h, self.plant.inertia_t.data_ptr()), lib)
        native.check(lib.vine_bind_env_inertia(self.model.h, self.inertia_t.data_ptr()), lib)
        full = dict(masses=_masses(Dm, c), floor=spec.get("floor", mpc_adapt.DEFAULTS["floor"]))
        self.icfg, self.mass_names = mai.masses_config(full, self.ibase, self.vcfg.link_length, self.vcfg.link_com, self.vcfg.gravity)
        self.mdims = mai.mass_dims_of(self.icfg)
        self.mass_truth = np.tile(np.array([self.cart, PLANT_MASSES[1], PLANT_MASSES[2]])[[m[0] for m in self.mdims]], (M, 1))
        f64 = torch.float64
        self.mass_mean = torch.zeros((M, Dm), dtype=f64, device=d)
        self.mass_std = torch.zeros((M, Dm), dtype=f64, device=d)
        self.mass_prior_mean = torch.full((M, Dm), 1.0, dtype=f64, device=d)
        self.mass_prior_std = torch.full((M, Dm), 0.2, dtype=f64, device=d)
        self.mass_weights = torch.full((N,), SENTINEL, dtype=f64, device=d)
        self.with_masses = True

    def inertia_pin(self):
        return self.lib.vine_mpc_adapt_inertia_pin(
            self.model.h, self.acfg, self.icfg, self.inertia_t.data_ptr(), self.mass_mean.data_ptr(), self.mass_std.data_ptr(),
            self.passes.data_ptr(), _stream(self.dev))

    def inertia_estimate(self):
        return self.lib.vine_mpc_adapt_inertia_estimate(
            self.model.h, self.acfg, self.icfg, self.inertia_t.data_ptr(), self.err.data_ptr(), self.trace_len.data_ptr(),
            self.episode_ended.data_ptr(), self.mass_mean.data_ptr(), self.mass_std.data_ptr(), self.mass_prior_mean.data_ptr(),
            self.mass_prior_std.data_ptr(), self.passes.data_ptr(), self.mass_weights.data_ptr(), _stream(self.dev))

    def pin(self, model=None, acfg=None):
        rc = super().pin(model, acfg)
        return rc if rc != abi.OK or not self.with_masses else self.inertia_pin()

    def mass_theta(self):
        return mai.mass_candidates(self.mass_mean.cpu().numpy(), self.mass_std.cpu().numpy(), self.mdims, self.seed, self.K,
                                   self.passes.cpu().numpy())

    def guards(self):
        b = self.buffer.cpu().numpy()
        return np.concatenate([b[:GUARD], b[-GUARD:]])

    def close(self):
        for env in (self.plant, self.model):      # the tables outlive their binding
            self.lib.vine_bind_env_inertia(env.h, None)
        super().close()


# ---------------------------------------------------------------------------------------------------------------- the pin
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_inertia_pin_columns_guards_and_what_the_base_pin_leaves(shape):
    """The inertia table and its guards full of a sentinel; the belief wide enough that candidates meet both ends of a range.
    All 31 rows of every column are ``inertia_rows(mass_candidates(...))`` bit for bit, the guards keep the sentinel, every
    column passes ``vine_env_inertia_check``; the parameter table and the state block are what ``vine_mpc_adapt_pin`` alone
    leaves."""
    M, K, W, D, Dm = shape
    rig = MassRig(M, K, W, D, Dm)
    try:
        N = M * K
        rig.warm_plant(9, seed=M + K)
        rig.ok(rig.anchor())
        rng = np.random.default_rng(M * 100 + K)
        lo = np.array([m[1] for m in rig.mdims])
        hi = np.array([m[2] for m in rig.mdims])
        rig.mass_mean.copy_(torch.as_tensor(lo + rng.uniform(0.2, 0.8, (M, Dm)) * (hi - lo)))
        rig.mass_std.copy_(torch.as_tensor(rng.uniform(0.2, 0.6, (M, Dm)) * (hi - lo)))
        rig.mean.copy_(torch.as_tensor(np.full((M, D), 0.04)))
        rig.std.copy_(torch.as_tensor(np.full((M, D), 0.02)))
        rig.passes.copy_(torch.as_tensor([0, 3, (1 << 32) + 1, 7, 123456789][:M]))
        rig.trace_actions.copy_(torch.as_tensor(rng.uniform(-1, 1, (M, W, 2)).astype(np.float32)))
        left = []
        for with_masses in (False, True):
            rig.with_masses = with_masses
            rig.model.state_t.fill_(SENTINEL)
            rig.model.table_t.copy_(torch.as_tensor(np.repeat(rig.base[:, None], N, axis=1)))
            rig.buffer.fill_(SENTINEL)
            rig.model.step_count = 5
            rig.ok(rig.pin())
            torch.cuda.synchronize()
            left.append((rig.model.table_t.cpu().numpy().copy(), rig.model.state_t.cpu().numpy().copy(),
                         rig.inertia_t.cpu().numpy().copy(), rig.err.cpu().numpy().copy(), rig.actions.cpu().numpy().copy()))
        (table0, state0, inertia0, err0, act0), (table1, state1, got, err1, act1) = left
        assert np.all(inertia0 == np.float32(SENTINEL))                        # the base pin does not touch the inertia table
        assert _same(table0, table1) and _same(state0, state1) and _same(err0, err1) and _same(act0, act1)
        theta = rig.mass_theta()
        assert np.array_equal(theta[:, 0], rig.mass_mean.cpu().numpy())
        if K > 2:
            assert (theta == hi).any() and (theta == lo).any()
        want = mai.inertia_rows(theta, rig.mdims, rig.ibase, rig.derive)
        assert want.shape == got.shape == (abi.VI_COUNT, N)
        for r in range(abi.VI_COUNT):
            assert _same(got[r], want[r]), r
        assert np.all(rig.guards() == np.float32(SENTINEL))
        env_params.check_inertia_table(rig.lib, rig.vcfg, got)
        assert len(np.unique(got[abi.VI_ADIAG0 + 2])) >= min(N - M, N // 2)
    finally:
        rig.close()


def test_refusals_that_need_a_handle():
    M, K, W, D, Dm = 2, 4, 3, 1, 1
    rig = MassRig(M, K, W, D, Dm)
    bare = base_tests._env(_cfg(M * K), np.repeat(rig.base[:, None], M * K, axis=1))      # a parameter table, no inertia table
    try:
        lib = rig.lib
        kept, rig.model = rig.model, bare
        for fn in (rig.inertia_pin, rig.inertia_estimate):
            assert fn() == abi.ERR_UNSUPPORTED and b"no inertia table bound" in lib.vine_last_error()
        rig.model = kept
        elsewhere = torch.zeros((abi.VI_COUNT, M * K), device=rig.dev)
        inside, rig.inertia_t = rig.inertia_t, elsewhere
        for fn in (rig.inertia_pin, rig.inertia_estimate):
            assert fn() == abi.ERR_UNSUPPORTED and b"is not the table bound" in lib.vine_last_error()
        rig.inertia_t = inside
        wrong, _ = mpc_adapt.adapt_config(dict(params=base_tests.PARAMS[1], window=W), M + 1, K, rig.base)
        kept, rig.acfg = rig.acfg, wrong
        for fn in (rig.inertia_pin, rig.inertia_estimate):
            assert fn() == abi.ERR_INVALID_ARG and b"num_plants * samples" in lib.vine_last_error()
        rig.acfg = kept
        rig.mass_mean.fill_(1.0)
        for fn in (rig.inertia_pin, rig.inertia_estimate):
            rig.ok(fn())
        torch.cuda.synchronize()
    finally:
        rig.close()
        bare.close()


# --------------------------------------------------------------------------------------------------------- exact recovery
@pytest.mark.parametrize("pipe", [False, True], ids=["free", "pipe"])
def test_candidates_that_are_the_plant_masses_included_score_zero(pipe):
    """(5, 14, 6, 1, 3): the plants carry 1.3 x the cart's mass, LINK_MASS 0.8 and TIP_LINK_MASS 1.5 beside their own DAMPING,
    and the belief's mean is the truth in all four dimensions, so candidate 0 IS the plant -- its inertia column holds the
    plant's bits, derived rows included -- and scores err == 0.0 exactly; every candidate whose rows differ scores more."""
    M, K, W, D, Dm = SHAPES[0]
    rig = MassRig(M, K, W, D, Dm, pipe=pipe)
    try:
        rig.warm_plant(11, seed=5, scale=0.6)
        rig.believe_the_truth()
        rig.mass_mean.copy_(torch.as_tensor(rig.mass_truth))
        rig.mass_std.copy_(torch.as_tensor(np.tile([0.1 * rig.cart, 0.05, 0.05], (M, 1))))
        rig.traced_window()
        assert np.array_equal(rig.trace_len.cpu().numpy(), [W] * M)
        states, resets, errs = rig.replay()
        err = errs[-1].reshape(M, K)
        table, inertia = rig.model.table_t.cpu().numpy(), rig.inertia_t.cpu().numpy()
        assert _same(table[:, ::K], rig.plant.table_t.cpu().numpy())
        assert _same(inertia[:, ::K], rig.plant_inertia)                       # candidate 0 holds the plant's masses, all 31 rows
        differs = ((_bits(inertia) != _bits(np.repeat(rig.plant_inertia, K, axis=1))).any(axis=0)
                   | (_bits(table[abi.VP_DAMPING]) != _bits(np.repeat(rig.plant.table_t.cpu().numpy()[abi.VP_DAMPING], K)))
                   ).reshape(M, K)
        assert differs[:, 1:].all() and not differs[:, 0].any()
        print("exact recovery (%s): err of candidate 0 %s, smallest other err %.3g" % (
            "pipe" if pipe else "free", err[:, 0], err[:, 1:].min()))
        assert np.all(err[:, 0] == 0.0), err[:, 0]
        assert np.all(err[differs] > 0.0)
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------ the estimate
@pytest.mark.parametrize("forget", [False, True], ids=["keep", "forget"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mass_estimate_against_numpy(shape, forget):
    """Errors made by hand on the device (a planted +inf and, where K allows, a planted NaN among them); ``mass_estimate`` is fed
    the device's own inputs.  Weights, mean and std within 1e-12 relative (the bound of the base estimate's test: the same
    float64 sums in another order, exp and sqrt within an ulp); the branches that compute nothing are exact; the planning
    columns of all K samples are ``inertia_rows`` of the device's new mean; passes is not written; two runs give the same bits."""
    M, K, W, D, Dm = shape
    rig = MassRig(M, K, W, D, Dm)
    try:
        rig.acfg.forget_on_reset = int(forget)
        rng = np.random.default_rng(M * 1000 + K)
        err = rng.uniform(0.0, 0.6, (M, K))
        err[0, 0] = np.inf
        if K > 2:
            err[0, 2] = np.nan
        tl, ended = np.full(M, W, dtype=np.int32), np.zeros(M, dtype=np.uint8)
        if M >= 2:
            err[1, :] = np.inf
        if M >= 3:
            tl[2] = rig.acfg.min_steps - 1
            ended[3] = 1
            err[4, 1:] += 50.0
        lo = np.array([m[1] for m in rig.mdims])
        hi = np.array([m[2] for m in rig.mdims])
        mean = lo + rng.uniform(0.2, 0.8, (M, Dm)) * (hi - lo)
        std = rng.uniform(0.05, 0.3, (M, Dm)) * (hi - lo)
        prior_mean, prior_std = lo + 0.5 * (hi - lo) + np.zeros((M, Dm)), 0.25 * (hi - lo) + np.zeros((M, Dm))
        passes = rng.integers(0, 1 << 34, M)
        outs = []
        for _ in range(2):
            for t, v in ((rig.err, err.reshape(-1)), (rig.trace_len, tl), (rig.episode_ended, ended), (rig.mass_mean, mean),
                         (rig.mass_std, std), (rig.mass_prior_mean, prior_mean), (rig.mass_prior_std, prior_std),
                         (rig.passes, passes)):
                t.copy_(torch.as_tensor(v))
            rig.buffer.fill_(SENTINEL)
            rig.mass_weights.fill_(SENTINEL)
            rig.ok(rig.inertia_estimate())
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy().copy() for t in (rig.mass_mean, rig.mass_std, rig.mass_weights, rig.passes, rig.inertia_t)])
        for a, b in zip(*outs):
            assert _same(a, b)
        got_mean, got_std, got_w, got_passes, got_table = outs[0]
        theta = mai.mass_candidates(mean, std, rig.mdims, rig.seed, K, passes)
        r = mai.mass_estimate(err.reshape(-1), theta, mean, std, prior_mean, prior_std, tl, ended, rig.mdims,
                              rig.acfg.min_steps, rig.acfg.temperature, rig.acfg.rate, forget)
        w = got_w.reshape(M, K)
        print("mass estimate %s: weights %s, mean %s, std %s (bit-identical?)" % (
            shape, _same(w, r["weights"]), _same(got_mean, r["mean"]), _same(got_std, r["std"])))
        assert np.all(np.abs(w - r["weights"]) <= 1e-12 * r["weights"])
        assert np.all(np.abs(got_mean - r["mean"]) <= 1e-12 * np.abs(r["mean"]))
        assert np.all(np.abs(got_std - r["std"]) <= 1e-12 * r["std"])
        assert np.array_equal(got_passes, passes)                              # the base estimate behind it increments them
        if K > 2:
            assert r["estimated"][0] and w[0].max() == 1.0 and w[0, 0] == 0.0 and w[0, 2] == 0.0
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
            assert w[4, 0] == 1.0 and 1e-5 < w[4, 1:].min() and w[4, 1:].max() < 3e-5
        plan = np.minimum(np.maximum(got_mean, lo), hi)
        want = mai.inertia_rows(np.repeat(plan, K, axis=0), rig.mdims, rig.ibase, rig.derive)
        for row in range(abi.VI_COUNT):
            assert _same(got_table[row], want[row]), row
        assert np.all(rig.guards() == np.float32(SENTINEL))
        env_params.check_inertia_table(rig.lib, rig.vcfg, got_table)
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------ the task classes
DAMPINGS = [0.01, 0.03, 0.07, 0.095, 0.05]
LINKS = [0.75, 0.9, 1.15, 1.35]


def _tasks(M, K, plant_params, model_params, plant_set=None, **plant_env):
    """A plant task of M envs and a model task of M * K.  ``plant_set``: per-plant values set behind the draw (the ``values``
    lists of one spec count the env index in a mixed radix, so two of them would not vary together over four plants)."""
    cfg = base_tests._plant_cfg(min(M, 4), **plant_env)
    cfg["env"]["numEnvs"] = M
    cfg["env"]["ENV_PARAMS"] = plant_params
    mcfg = mpc.model_config(cfg, M, K)
    mcfg["env"]["ENV_PARAMS"] = model_params
    plant, model = mpc.make_task(cfg), mpc.make_task(mcfg)
    if plant_set:
        plant.set_env_params({k: np.asarray(v, dtype=np.float64) for k, v in plant_set.items()})
    return plant, model


def test_a_degenerate_mass_belief_is_the_plain_adaptive_controller():
    """What keeps the restated estimate from drifting.  (5, 14, 6, 1), three cycles: ``AdaptiveInertiaController`` with
    ``CART_MASS [c, c]`` and ``LINK_MASS [1, 1]`` (c the configuration's) beside an ``AdaptiveController`` on the same plants and
    seed, both models bound to the configuration's inertia row.  After every control step every shared controller tensor, both
    state blocks and the parameter table are equal in every bit, and the model's inertia table is the configuration's row."""
    M, K, H, W = 5, 14, 4, 6
    params = {"DAMPING": {"values": DAMPINGS}}
    row = {"FPAM_K": 1.0, "LINK_MASS": 1.0}
    adapt = {"params": {"DAMPING": [0.005, 0.1]}, "window": W, "every": W}
    pa, ma = _tasks(M, K, params, dict(row))
    pb, mb = _tasks(M, K, params, dict(row))
    try:
        base = env_params.inertia_config_row(ma._lib, ma._vcfg)
        c = float(base[abi.VI_CART_MASS])
        plain = mpc_adapt.AdaptiveController(pa, ma, K, adapt, H, seed=5, graph=False)
        both = mai.AdaptiveInertiaController(pb, mb, K, dict(adapt, masses={"CART_MASS": [c, c], "LINK_MASS": [1.0, 1.0]}), H,
                                             seed=5, graph=False)
        assert both.names == ["DAMPING"] and both.mass_names == ["CART_MASS", "LINK_MASS"] and not both.placeholder
        shared = len(plain.tensors())
        for step in range(3 * W):
            plain.run(1)
            both.run(1)
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(plain.tensors(), both.tensors()[:shared])):
                assert _same(a.cpu().numpy(), b.cpu().numpy()), (step, i)
            assert _same(pa.state.cpu().numpy(), pb.state.cpu().numpy()) and _same(ma.state.cpu().numpy(), mb.state.cpu().numpy())
            assert _same(ma.env_params.cpu().numpy(), mb.env_params.cpu().numpy()), step
            assert _same(mb.env_inertia.cpu().numpy(), np.repeat(base[:, None], M * K, axis=1)), step
        assert np.all(both.passes.cpu().numpy() == 3) and both.launches["inertia_pin"] == both.launches["inertia_estimate"] == 3
        assert {k: v for k, v in both.launches.items() if not k.startswith("inertia_")} == plain.launches
        assert not _same(plain.mean.cpu().numpy(), plain.prior_mean.cpu().numpy())          # (the belief did move)
        mean, std = both.mass_belief()
        # (a weighted mean of K equal values is that value up to an ulp, so sqrt(v) is of the order of an ulp, not 0)
        assert np.all(mean == [c, 1.0]) and np.all(std <= 4 * np.finfo(np.float64).eps)
    finally:
        for t in (ma, pa, mb, pb):
            t.close()


def test_captured_cycles_against_eager_ones_with_masses():
    """Two captured cycles replayed three times against six eager ones, and two control steps more, with ``masses`` on: every
    controller tensor (the mass belief and both of the model's tables among them) and both state blocks bit-identical."""
    M, K, H = 4, 16, 6
    adapt = {"params": {"DAMPING": [0.005, 0.1]}, "masses": {"LINK_MASS": [0.7, 1.4], "CART_MASS": [0.3, 1.0]},
             "window": 4, "every": 5, "min_steps": 2}
    params = {"LINK_MASS": {"values": LINKS}}
    runs = []
    for tag, kw in (("graph", dict(graph=True, graph_cycles=2)), ("eager", dict(graph=False))):
        plant, model = _tasks(M, K, params, {"FPAM_K": 1.0, "LINK_MASS": 1.0}, plant_set={"DAMPING": DAMPINGS[:4]},
                              maxEpisodeLength=10)
        try:
            assert len(np.unique(plant.env_params[abi.VP_DAMPING].cpu().numpy())) == len(np.unique(
                plant.env_inertia[abi.VI_LINK_MASS0].cpu().numpy())) == 4
            ctl = mai.AdaptiveInertiaController(plant, model, K, adapt, H, seed=5, keep_weights=True, **kw)
            assert ctl.use_graph == (tag == "graph") and (ctl.W, ctl.E, ctl.D, ctl.Dm) == (4, 5, 1, 2)
            assert any(t is model.env_inertia for t in ctl.tensors()) and any(t is ctl.mass_mean for t in ctl.tensors())
            ctl.run(32)
            torch.cuda.synchronize()
            assert ctl.launches["inertia_pin"] == ctl.launches["inertia_estimate"] == ctl.launches["pin"] == 6
            if tag == "graph":
                assert ctl.graph_launches["inertia_pin"] == ctl.graph_launches["inertia_estimate"] == 2
            assert np.all(ctl.passes.cpu().numpy() == 6)
            runs.append(([t.cpu().numpy().copy() for t in ctl.tensors()], plant.state.cpu().numpy().copy(),
                         model.state.cpu().numpy().copy(), ctl.mass_belief()[0], ctl.mass_prior_mean.cpu().numpy()))
            env_params.check_inertia_table(model._lib, model._vcfg, model.env_inertia.cpu().numpy())
        finally:
            model.close()
            plant.close()
    (ta, pa, ma, mean, prior), (tb, pb, mb, _, _) = runs
    for a, b in zip(ta, tb):
        assert _same(a, b)
    assert _same(pa, pb) and _same(ma, mb)
    assert mean.shape == (M, 2) and np.isfinite(mean).all() and not _same(mean, prior)


def test_mpc_py_with_masses_and_set_model_params(tmp_path):
    """``mpc.py``'s main with ``adapt={masses: ...}`` alone (the placeholder dimension is not reported) and together with
    ``params``; ``out["adapt"]`` carries the mass names, their truth and errors; ``set_model_params`` refuses a mass name."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mpc_cli", os.path.join(REPO, "mpc.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    argv = ["plants=4", "samples=32", "horizon=6", "steps=20", "out=%s" % tmp_path, "task.env.CREATE_PIPE=False",
            "task.task.vine_randomize=False", "seed=3",
            "task.env.ENV_PARAMS={LINK_MASS: {values: [0.75, 0.9, 1.15, 1.35]}}"]
    out = cli.main(argv + ["adapt={masses: {LINK_MASS: [0.7, 1.4]}, window: 4, every: 4}"])
    a = out["adapt"]
    assert a["names"] == ["LINK_MASS"] == a["mass_names"] and a["mass_mean"].shape == a["mass_truth"].shape == (4, 1)
    assert np.allclose(a["mass_truth"][:, 0], LINKS, rtol=1e-6) and np.all(a["mass_prior_mean"] == 1.0)
    assert set(a["prior_error"]) == set(a["final_error"]) == {"LINK_MASS"} and np.all(a["passes"] == 5)
    assert out["launches"]["inertia_pin"] == out["launches"]["inertia_estimate"] == out["launches"]["estimate"] == 5
    assert out["graphed"] and np.isfinite(out["plant_return"]).all()
    out = cli.main(argv + ["adapt={params: {DAMPING: [0.005, 0.1]}, masses: {LINK_MASS: [0.7, 1.4]}, window: 4, every: 4}"])
    a = out["adapt"]
    assert a["names"] == ["DAMPING", "LINK_MASS"] and a["mass_names"] == ["LINK_MASS"] and a["mean"].shape == (4, 1)
    assert set(a["prior_error"]) == set(a["final_error"]) == {"DAMPING", "LINK_MASS"}
    plant, model = _tasks(4, 8, {"DAMPING": {"values": DAMPINGS[:4]}}, {"FPAM_K": 1.0, "LINK_MASS": 1.0})
    try:
        ctl = mai.AdaptiveInertiaController(plant, model, 8, {"masses": {"LINK_MASS": [0.7, 1.4]}, "window": 2, "every": 2}, 3,
                                            graph=False)
        assert ctl.placeholder and ctl.names == [] and ctl.D == 1 and not ctl.std.any() and not ctl.prior_std.any()
        ctl.run(4)
        with pytest.raises(ValueError, match="LINK_MASS is adapted on the device"):
            ctl.set_model_params({"LINK_MASS": 1.1})
        with pytest.raises(ValueError, match="CART_MASS lies in the inertia table"):
            ctl.set_model_params({"CART_MASS": 1.1})
        ctl.set_model_params({"RAIL_P_GAIN": np.array([1.0, 2.0, 3.0, 4.0])})
        assert _same(model._env_inertia_host, model.env_inertia.cpu().numpy())
        # the placeholder's rows: the model's own bits
        assert _same(model.env_params[abi.VP_DAMPING].cpu().numpy(), model._env_params_host[abi.VP_DAMPING])
        mean, _ = ctl.mass_belief()
        want = mai.inertia_rows(np.repeat(np.minimum(np.maximum(mean, 0.7), 1.4), 8, axis=0), ctl.mdims, ctl.base_inertia, ctl.derive)
        assert _same(model.env_inertia.cpu().numpy(), want)
    finally:
        model.close()
        plant.close()


# --------------------------------------------------------------------------------------------------------------- it adapts
# |final mean - truth| / |prior - truth| per plant from scripts/mpc_adapt_inertia_oracle_check.py (float64 oracle, random
# actions), profiles/mpc_adapt_inertia/it_adapts_oracle.txt.  The device asserts 0.5 where the oracle reaches 0.25.
ORACLE = {
    "link": ("LINK_MASS", [0.0018, 0.0033, 0.0011, 0.0016]),
    "cart": ("CART_MASS", [0.5104, 0.0132, 0.0071, 0.0205]),      # plant 0 (0.6 c) is not asserted: the oracle does not reach it
    "link_damping": ("LINK_MASS", [0.0109, 0.0176, 0.0122, 0.0033]),
}
CARTS = [0.6, 0.8, 1.4, 1.8]


@pytest.mark.parametrize("case", ["link", "cart", "link_damping"])
def test_it_adapts(case):
    """Four plants with LINK_MASS 0.75 / 0.9 / 1.15 / 1.35 (or CART_MASS 0.6 / 0.8 / 1.4 / 1.8 x c over [0.5 c, 2 c]), the prior
    at 1.0 (c), range [0.7, 1.4], K = 64, W = E = 8, ten passes, section 25's constants.  Condition, asserted for the plants
    where the float64 oracle's ratio is at most 0.25: each final |mean - truth| is at most half the prior's.  The device's own
    figures are printed in every case; profiles/mpc_adapt_inertia/it_adapts.txt holds them beside the oracle's."""
    M, K, H, P = 4, 64, 8, 10
    name, oracle = ORACLE[case]
    plant, model = _tasks(M, K, {"FPAM_K": 1.0}, {"FPAM_K": 1.0, "LINK_MASS": 1.0}, USE_TARGET_REACHED_RESET=False)
    plant.close()
    model.close()
    c = float(env_params.inertia_config_row(model._lib, model._vcfg)[abi.VI_CART_MASS])
    params = {"CART_MASS": {"values": [f * c for f in CARTS]}} if case == "cart" else {"LINK_MASS": {"values": LINKS}}
    adapt = {"masses": {name: [0.5 * c, 2.0 * c] if case == "cart" else [0.7, 1.4]}, "window": 8, "every": 8}
    model_params, plant_set = {"FPAM_K": 1.0, "LINK_MASS": 1.0}, None
    if case == "link_damping":
        plant_set = {"DAMPING": DAMPINGS[:4]}
        adapt["params"] = {"DAMPING": [0.005, 0.1]}
        model_params["DAMPING"] = 0.0525
    plant, model = _tasks(M, K, params, model_params, plant_set=plant_set, seed=1, USE_TARGET_REACHED_RESET=False)
    try:
        ctl = mai.AdaptiveInertiaController(plant, model, K, adapt, H, seed=1)
        prior, truth = ctl.mass_prior_mean.cpu().numpy()[:, 0], ctl.mass_truth()[:, 0]
        assert np.all(prior == (np.float64(np.float32(c)) if case == "cart" else 1.0))
        assert np.allclose(truth, [f * c for f in CARTS] if case == "cart" else LINKS, rtol=1e-6)
        ctl.run(P * ctl.E)
        mean, std = ctl.mass_belief()
        ratio = np.abs(mean[:, 0] - truth) / np.abs(prior - truth)
        print("it adapts (%s): %s truth %s, final mean %s, final std %s, |mean - truth| / |prior - truth| %s, passes %s" % (
            case, name, truth, mean[:, 0], std[:, 0], ratio, ctl.passes.cpu().numpy()))
        if case == "link_damping":
            dm, dt, dp = ctl.belief()[0][:, 0], ctl.truth()[:, 0], ctl.prior_mean.cpu().numpy()[:, 0]
            assert np.allclose(dt, DAMPINGS[:4], rtol=1e-6)
            print("it adapts (%s): DAMPING truth %s, final mean %s, ratio %s" % (case, dt, dm, np.abs(dm - dt) / np.abs(dp - dt)))
        assert np.all(ctl.passes.cpu().numpy() == P)
        asserted = [p for p in range(M) if oracle[p] <= 0.25]
        for p in asserted:
            assert ratio[p] <= 0.5, (p, ratio)
    finally:
        model.close()
        plant.close()
