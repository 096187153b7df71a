"""``truncate_grads`` on the device: the sum-of-squares launch (``vine_grad_sqnorm``), the clip folded into the Adam launch
(``vine_adam_step_clip``), ``FlatAdam.step(clip=...)`` and the agent's graphed update with clipping on."""
import functools
import os

import pytest
import torch

from vine_robot_isaacgymenvs_amd.learning.flat_adam import FlatAdam

VINE_ERR_UNSUPPORTED = -2


# --------------------------------------------------------------------------- CPU
def _flat_and_torch(device):
    """Five steps of FlatAdam (gradients "summed over 2 ranks", grad_scale 0.5) next to torch.optim.Adam."""
    torch.manual_seed(3)
    shapes = [(64, 28), (64,), (1024, 92), (3,), (2,)]
    a = [torch.randn(s, device=device).requires_grad_() for s in shapes]
    b = [t.detach().clone().requires_grad_() for t in a]
    c = [t.detach().clone().requires_grad_() for t in a]
    one = FlatAdam(a, torch.tensor(3e-4, device=device), eps=1e-8)
    two = FlatAdam(c, torch.tensor(3e-4, device=device), eps=1e-8)
    ref = torch.optim.Adam(b, lr=3e-4, eps=1e-8)
    return shapes, (a, one), (c, two), (b, ref)


def test_flat_adam_cpu_clip_is_clip_grad_norm_then_step():
    dev = torch.device("cpu")
    shapes, (a, one), (c, two), (b, ref) = _flat_and_torch(dev)
    for it in range(5):
        grads = [torch.randn(s) for s in shapes]          # norm ~ 310: every step clips at 1.0
        for p, r, q, g in zip(a, c, b, grads):
            p.grad.copy_(g)
            r.grad.copy_(g)
            q.grad = g.clone()
        one.step(clip=1.0)
        two.clip_grad_norm_(1.0)
        two.step()
        torch.nn.utils.clip_grad_norm_(b, 1.0)
        ref.step()
    assert torch.equal(one.flat_params, two.flat_params)
    assert torch.equal(one.exp_avg, two.exp_avg) and torch.equal(one.exp_avg_sq, two.exp_avg_sq)
    assert float(one.step_t) == 5.0 and float(one.flat_grads.abs().max()) == 0.0
    for p, q in zip(a, b):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-7)


# --------------------------------------------------------------------------- kernels
def _lib():
    from vine_robot_isaacgymenvs_amd import native
    return native.load()


def _default_numel():
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.learning.network import ModelA2CContinuousLogStd
    m = ModelA2CContinuousLogStd(load_config()["train"]["params"]["network"], 2, (28,), True, True)
    return FlatAdam(m.parameters(), 3e-4).numel


class _State:
    """Buffers of one raw Adam launch over n floats."""

    def __init__(self, n, dev, amp_scale=None, seed=0):
        from vine_robot_isaacgymenvs_amd.learning import fused
        torch.manual_seed(seed)
        self.n = n
        self.p = torch.randn(n, device=dev)
        self.g = torch.zeros(n, device=dev)
        self.m, self.v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        self.lr, self.step = torch.tensor(3e-4, device=dev), torch.zeros((), device=dev)
        self.shadow = self.p.to(fused.lp_dtype())
        self.amp = None if amp_scale is None else torch.tensor([amp_scale, 0.0, 2000.0, 0.0], device=dev)
        self.found = None if amp_scale is None else torch.zeros(1, device=dev)
        lib = _lib()
        self.parts = int(lib.vine_grad_sqnorm_parts(n))
        self.partial = torch.full((self.parts + 1,), -1.0, device=dev, dtype=torch.float64)     # (+ a sentinel)
        self.clip_out = torch.full((2,), -1.0, device=dev)

    def _common(self):
        ptr = lambda t: None if t is None else t.data_ptr()
        return (self.n, self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.lr.data_ptr(),
                self.step.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1.0, self.shadow.data_ptr(), None, 0.0, 0.0, 0.0, 0.0,
                ptr(self.amp), ptr(self.found))

    def sqnorm(self):
        st = torch.cuda.current_stream().cuda_stream
        assert _lib().vine_grad_sqnorm(self.n, self.g.data_ptr(), self.partial.data_ptr(), st) == 0

    def step_clip(self, max_norm):
        st = torch.cuda.current_stream().cuda_stream
        self.sqnorm()
        rc = _lib().vine_adam_step_clip(*self._common(), self.partial.data_ptr(), self.parts, max_norm,
                                        self.clip_out.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()

    def step_amp(self):
        assert _lib().vine_adam_step_amp(*self._common(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("gain", [0.01, 30.0])
@pytest.mark.parametrize("n", [7, 3079, "default"])
def test_sqnorm_against_float64_and_reproducible(n, gain):
    """The norm the Adam launch derives from the partial sums against torch's float64 norm, relative 1e-6: the squares
    have no cancellation, every element is squared and added in float64 in a fixed tree (workgroup partials and their
    fold included), so only the final rounding to float32 (2^-24) is visible.  Two launches over the same block give the
    same bits; the launch writes exactly ``vine_grad_sqnorm_parts(n)`` partials, whose sum is the float64 sum of squares
    (1e-12: some 2^5 float64 roundings per chain, here and in the reference)."""
    dev = torch.device("cuda:0")
    n = _default_numel() if n == "default" else n
    s = _State(n, dev)
    assert 1 <= s.parts <= 256 and s.parts == min(256, ((n + 3) // 4 + 255) // 256)
    if n == 7:
        assert s.parts == 1
    torch.manual_seed(n)
    g = torch.randn(n, device=dev) * gain
    expect = float(torch.linalg.vector_norm(g.double()))
    runs = []
    for _ in range(2):
        s.g.copy_(g)
        s.partial.fill_(-1.0)
        s.step_clip(1.0)
        runs.append((s.partial.clone(), s.clip_out.clone()))
    got = float(runs[0][1][0])
    print("n=%d gain=%g parts=%d norm %.9g expect %.9g rel %.3g" % (n, gain, s.parts, got, expect, abs(got - expect) / expect))
    assert abs(got - expect) <= 1e-6 * expect
    assert float(runs[0][0][-1]) == -1.0 and bool((runs[0][0][:-1] >= 0).all())
    assert abs(float(runs[0][0][:-1].sum()) - expect ** 2) <= 1e-12 * expect ** 2
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert abs(float(runs[0][1][1]) - min(1.0, 1.0 / (got + 1e-6))) <= 1e-6      # max_norm = 1


@pytest.mark.gpu
def test_sqnorm_rejects_a_misaligned_block():
    dev = torch.device("cuda:0")
    g = torch.zeros(1028, device=dev)
    partial = torch.zeros(4, device=dev, dtype=torch.float64)
    st = torch.cuda.current_stream().cuda_stream
    assert _lib().vine_grad_sqnorm(1024, g.data_ptr() + 4, partial.data_ptr(), st) == VINE_ERR_UNSUPPORTED
    assert _lib().vine_grad_sqnorm(1024, g.data_ptr(), partial.data_ptr(), st) == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("gain", [0.01, 30.0])
def test_clip_step_matches_torch_clip_then_adam(gain, amp):
    """``FlatAdam.step(grad_scale=0.5, clip=100)`` against ``clip_grad_norm_`` + ``torch.optim.Adam.step`` for five steps,
    with and without device loss scaling (scale 1024): gain 0.01 (norm ~ 3) never clips, gain 30 (norm ~ 9300) always."""
    from vine_robot_isaacgymenvs_amd.learning import fused
    dev = torch.device("cuda:0")
    max_norm = 100.0
    shapes, (a, flat), _, (b, ref) = _flat_and_torch(dev)
    flat.enable_lp16_shadow()
    scale = 1.0
    if amp:
        flat.enable_loss_scaling(init_scale=1024.0)
        scale = 1024.0
    coefs = []
    for it in range(5):
        grads = [torch.randn(s, device=dev) * gain for s in shapes]
        for p, q, g in zip(a, b, grads):
            p.grad.copy_(2.0 * scale * g)          # as if summed over 2 ranks, loss-scaled
            q.grad = g.clone()
        norm_ref = float(torch.nn.utils.clip_grad_norm_(b, max_norm))
        flat.step(grad_scale=0.5, clip=max_norm)
        ref.step()
        torch.cuda.synchronize()
        norm, coef = (float(x) for x in flat.clip_out)
        assert abs(norm - norm_ref) <= 1e-5 * norm_ref      # (torch's is a float32 norm of 5 float32 norms)
        coefs.append(coef)
        assert float(flat.step_t) == it + 1 and float(flat.flat_grads.abs().max()) == 0.0
        assert torch.equal(flat.shadow, flat.flat_params.to(fused.lp_dtype()))
    for p, q in zip(a, b):
        assert torch.allclose(p, q, rtol=2e-5, atol=2e-7)
    if gain < 1.0:
        assert all(c == 1.0 for c in coefs), coefs
    else:
        assert all(0.0 < c < 1.0 for c in coefs), coefs
    if amp:
        assert float(flat.amp_state[0]) == 1024.0 and float(flat.amp_state[1]) == 5.0 and float(flat.found_inf) == 0.0


@pytest.mark.gpu
def test_coefficient_one_is_the_unclipped_step_bit_for_bit():
    dev = torch.device("cuda:0")
    n = 4099
    one, two = _State(n, dev, amp_scale=1024.0), _State(n, dev, amp_scale=1024.0)
    assert torch.equal(one.p, two.p)
    for it in range(3):
        g = torch.randn(n, device=dev) * 1024.0
        one.g.copy_(g)
        two.g.copy_(g)
        one.step_amp()
        two.step_clip(1e30)
        assert float(two.clip_out[1]) == 1.0
    for x, y in ((one.p, two.p), (one.m, two.m), (one.v, two.v), (one.shadow, two.shadow), (one.amp, two.amp),
                 (one.step, two.step), (one.g, two.g), (one.found, two.found)):
        assert torch.equal(x, y)
    assert float(two.step) == 3.0


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_norm_is_an_overflow(bad):
    """One inf / NaN in the block under loss scaling, the flag NOT raised by anyone: the step is skipped as for a raised
    flag, and the next finite step proceeds."""
    dev = torch.device("cuda:0")
    n = 4099
    s = _State(n, dev, amp_scale=1024.0)
    s.g.copy_(torch.randn(n, device=dev))
    s.step_clip(1.0)
    before = (s.p.clone(), s.m.clone(), s.v.clone(), float(s.step), s.shadow.clone())
    assert before[3] == 1.0 and float(s.amp[0]) == 1024.0 and float(s.amp[1]) == 1.0
    s.g.copy_(torch.randn(n, device=dev))
    s.g[n - 2] = bad                                    # (in the scalar tail's neighbourhood)
    s.step_clip(1.0)
    assert torch.equal(s.p, before[0]) and torch.equal(s.m, before[1]) and torch.equal(s.v, before[2])
    assert float(s.step) == before[3] and torch.equal(s.shadow, before[4])
    assert float(s.amp[0]) == 512.0 and float(s.amp[1]) == 0.0 and float(s.found) == 0.0
    assert float(s.g.abs().max()) == 0.0
    assert not bool(torch.isfinite(s.clip_out[0]))
    s.g.copy_(torch.randn(n, device=dev))
    s.step_clip(1.0)
    assert float(s.step) == 2.0 and not torch.equal(s.p, before[0]) and bool(torch.isfinite(s.p).all())
    assert float(s.amp[0]) == 512.0 and float(s.amp[1]) == 1.0 and bool(torch.isfinite(s.clip_out).all())
    assert float(s.g.abs().max()) == 0.0


# --------------------------------------------------------------------------- agent
@functools.lru_cache(maxsize=None)
def _agent_run(truncate, grad_norm, use_graphs, lr_schedule="adaptive", scope=None):
    """Four iterations at 512 envs / minibatch 2048 on the default (fp16 fused) update -> the optimiser's state, the
    {norm, coef} rows of every optimiser step and how the update ran.  ``scope``: VINE_UPD_GRAPH ("epoch" = one graph per
    mini-epoch, "step" = one per optimiser step with the previous step's Adam at its head: the form several ranks use
    when the collective stays outside the graphs)."""
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_config(overrides=["num_envs=512", "minibatch_size=2048"])
    cfg["task"]["seed"] = 42
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0",
                                                  graphics_device_id=0, headless=True)
    params = cfg["train"]["params"]
    params["config"].update(write_files=False, print_stats=False, use_graphs=use_graphs, mixed_precision=True,
                            truncate_grads=truncate, grad_norm=grad_norm, lr_schedule=lr_schedule)
    torch.manual_seed(0)
    agent = A2CAgent("t", params, vec_env=env)
    assert agent.fused_mixed
    agent.init_tensors()
    agent.obs = agent.env_reset()["obs"]
    lr0 = float(agent.lr)
    rows, stats = [], None
    before = os.environ.get("VINE_UPD_GRAPH")
    if scope is not None:
        os.environ["VINE_UPD_GRAPH"] = scope
    try:
        for _ in range(4):
            _, _, stats = agent.train_epoch()
            if truncate:
                rows.append(agent._clip_rows.clone())
    finally:
        if scope is not None:
            if before is None:
                del os.environ["VINE_UPD_GRAPH"]
            else:
                os.environ["VINE_UPD_GRAPH"] = before
    torch.cuda.synchronize()
    opt = agent.optimizer
    out = {"params": opt.flat_params.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(),
           "lr": float(agent.lr), "lr0": lr0, "loss_scale": opt.loss_scale, "steps": float(opt.step_t),
           "rows": torch.cat(rows).cpu() if rows else None, "status": agent.graph_status["update"],
           "has_clip_rows": getattr(agent, "_clip_rows", None) is not None,
           "stats": {k: float(v) for k, v in stats.items()}}
    env.close()
    return out


def _same_training(a, b):
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(a[k], b[k]), k
    assert a["lr"] == b["lr"] and a["loss_scale"] == b["loss_scale"] and a["steps"] == b["steps"] > 0


def _median_norm():
    rows = _agent_run(True, 1e9, True)["rows"]
    norms = rows[:, 0][torch.isfinite(rows[:, 0])]
    assert norms.numel() > 0
    return float(norms.median())


@pytest.mark.gpu
def test_agent_clipping_update_is_graphed_and_equals_eager():
    """`truncate_grads: True` keeps the one-graph-per-iteration update; with a threshold at the median step norm of an
    unclipped run (so that some steps clip and some do not) the graphed run is the eager run bit for bit, the recorded
    {norm, coef} rows included."""
    threshold = _median_norm()
    graphed, eager = _agent_run(True, threshold, True), _agent_run(True, threshold, False)
    assert graphed["status"].startswith("graph (1 per iteration"), graphed["status"]
    assert not eager["status"].startswith("graph")
    coef = graphed["rows"][:, 1][torch.isfinite(graphed["rows"][:, 0])]      # (overflowed steps aside)
    print("threshold %.6g; steps %d, coef == 1: %d, coef < 1: %d" % (threshold, coef.numel(), int((coef == 1).sum()),
                                                                    int((coef < 1).sum())))
    assert int((coef == 1).sum()) >= 1 and int((coef < 1).sum()) >= 1
    _same_training(graphed, eager)
    assert graphed["rows"].shape == eager["rows"].shape and graphed["rows"].shape[0] >= graphed["steps"]
    assert torch.equal(graphed["rows"].view(torch.int32), eager["rows"].view(torch.int32))      # (bits: NaN == NaN)
    assert 0.0 < graphed["stats"]["grad_clip_fraction"] < 1.0 and graphed["stats"]["grad_norm"] > 0.0
    for k in ("grad_norm", "grad_clip_fraction"):
        assert graphed["stats"][k] == eager["stats"][k]


@pytest.mark.gpu
@pytest.mark.parametrize("scope,status", [("epoch", "graph (1 per mini-epoch"), ("step", "graph (per optimiser step")])
def test_agent_clipping_in_the_smaller_graphs_equals_eager(scope, status):
    """The same comparison for the per-mini-epoch graph (its own {norm, coef} buffer, copied behind the replay) and the
    per-step graphs (the clipped Adam deferred into the head of the next graph and into the tail graph)."""
    threshold = _median_norm()
    graphed, eager = _agent_run(True, threshold, True, "adaptive", scope), _agent_run(True, threshold, False)
    assert graphed["status"].startswith(status), graphed["status"]
    _same_training(graphed, eager)
    assert torch.equal(graphed["rows"].view(torch.int32), eager["rows"].view(torch.int32))


@pytest.mark.gpu
def test_constant_learning_rate_update_is_graphed_and_equals_eager():
    graphed, eager = _agent_run(False, 1.0, True, "constant"), _agent_run(False, 1.0, False, "constant")
    assert graphed["status"].startswith("graph (1 per iteration"), graphed["status"]
    _same_training(graphed, eager)
    assert graphed["lr"] == graphed["lr0"]
    assert not graphed["has_clip_rows"] and "grad_norm" not in graphed["stats"]


@pytest.mark.gpu
def test_threshold_never_reached_is_truncate_grads_off():
    loose, free = _agent_run(True, 1e9, True), _agent_run(False, 1.0, True)
    assert loose["status"].startswith("graph (1 per iteration") and free["status"] == loose["status"]
    _same_training(loose, free)
    coef = loose["rows"][:, 1][torch.isfinite(loose["rows"][:, 0])]
    assert bool((coef == 1.0).all()) and loose["stats"]["grad_clip_fraction"] == 0.0
