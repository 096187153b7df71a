"""The update's gradient block against float64 autograd.

One optimiser step of the hand-written update (``A2CAgent._fused_grad_half``: in the default configuration the
four-phase launch ``vine_trunk_phases`` -- LSTM forward, LayerNorm + heads + loss, LSTM backward, MLP backward -- then the
weight-gradient, column-sum and loss-scaling kernels) on a synthetic minibatch, compared tensor by tensor with the
float64 reference of tests/update_reference.py: every parameter's gradient in the optimiser's flat block (divided by the
device loss scale), the loss statistics, the KL slot ``optimizer.aux[0]``, the dataset's ``mu`` / ``sigma`` refreshed in
place and the observation normaliser's running statistics.

Tolerance: the same minibatch through the stock composition under ``torch.autocast(float16)``, loss scaled by the same
GradScaler scale (the reference's own ``mixed_precision: True`` arithmetic), gives a baseline error against float64 per
tensor in two norms, max |d| / max |ref| and ||d|| / ||ref||.  The kernels' error may be at most ``K`` times that
baseline, or ``K`` times ``FLOOR`` (about the fp16 unit roundoff) where autocast happens to be nearly exact.  The fp32
update is held to fixed fp32-noise bounds.  Negative controls: the float64 reference recomputed from subtly wrong inputs
(dones shifted by one row, dones ignored, h0 zeroed, clip_value flipped) must break the same bound with margin on some
parameter gradient.

The synthetic minibatch keeps every sample 0.02 away from the edges between loss branches (ratio clip, value clip,
the critic's max): a 16-bit forward pass moves mu and the value by ~1e-3, and a sample that changes branch changes its
gradient by a step.  With such samples left in, a handful of them decided every tensor's error, kernels and autocast
alike, and the per-tensor ratio between the two ranged from 0.2 to 5 at random.

Measured on an MI355X, the worst tensor of each case (kernel error / max(autocast error, FLOOR); under 1: closer to
float64 than autocast; fp32: error / FP32_BOUND), max-relative | rms-relative:
    b32_below_trunk      0.002 (stat kl)              | 0.002 (stat kl)
    b64_two_workgroups   0.738 (value.weight)         | 0.664 (actor_mlp.4.weight)
    b8192_default        0.827 (weight_ih_l0)         | 0.784 (actor_mlp.0.weight)
    b8192_low_scale      0.617 (sigma)                | 0.691 (sigma)
    b32768_largest       0.523 (new mu)               | 0.483 (actor_mlp.0.weight)
    b32800_past_limit    0.883 (weight_ih_l0)         | 0.872 (actor_mlp.0.weight)
    b8200_ragged         0.556 (weight_hh_l0)         | 0.490 (actor_mlp.0.weight)
    b8192_fp32           0.012 (actor_mlp.4.weight)   | 0.009 (actor_mlp.0.weight)
hence K = 1.5.  The negative controls (b8192_default) exceed the bound on some parameter gradient by two orders of
magnitude or more, far beyond CONTROL_MARGIN; each run prints the figures.
"""
import time

import numpy as np
import pytest
import torch

from tests import update_reference as ur
from vine_robot_isaacgymenvs_amd.learning import fused

K = 1.5                 # kernel error <= K x max(autocast error, FLOOR), per tensor and norm
FLOOR = 2.0 ** -11      # float16 unit roundoff
FP32_BOUND = 1e-4       # the fp32 update: max- and rms-relative error
CONTROL_MARGIN = 4.0    # a negative control must exceed the bound by this factor on some tensor

# (id, sequences B (n = 4 B), observation width, mixed precision, clip_value, entropy_coef, loss scale, four-phase launch)
CASES = [
    ("b32_below_trunk", 32, 28, True, True, 0.0, 2.0 ** 16, False),     # n = 128 < 256 rows: the stock module path
    ("b64_two_workgroups", 64, 18, True, False, 0.01, 2.0 ** 4, True),
    ("b8192_default", 8192, 28, True, True, 0.0, 2.0 ** 16, True),
    ("b8192_low_scale", 8192, 18, True, False, 0.01, 2.0 ** 4, True),
    ("b32768_largest", 32768, 18, True, True, 0.01, 2.0 ** 16, True),     # n / 128 = 1024
    ("b32800_past_limit", 32800, 28, True, False, 0.0, 2.0 ** 4, False),  # n / 128 = 1025
    ("b8200_ragged", 8200, 18, True, True, 0.01, 2.0 ** 16, False),       # B % 32 = 8
    ("b8192_fp32", 8192, 28, False, False, 0.01, None, False),           # mixed_precision: False
]


class _Spaces:
    """All the agent reads of a task here: the observation and action spaces (the minibatch is synthetic)."""
    num_states = 0

    def __init__(self, width, actions=2):
        from vine_robot_isaacgymenvs_amd.tasks.base.spaces import Box
        self.observation_space = Box(np.full(width, -np.inf), np.full(width, np.inf))
        self.action_space = Box(-np.ones(actions), np.ones(actions))


def _agent(B, width, mixed, clip_value, entropy_coef, minibatches=1, **conf):
    """An agent whose minibatch is ``B`` sequences of 4 steps (``minibatches`` of them per mini-epoch; ``conf``: further
    entries of the training configuration)."""
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    n = 4 * B
    cfg = load_config(overrides=["num_envs=%d" % (minibatches * n // 16), "minibatch_size=%d" % n])
    params = cfg["train"]["params"]
    params["config"].update(write_files=False, print_stats=False, use_graphs=False, mixed_precision=mixed,
                            clip_value=clip_value, entropy_coef=entropy_coef, **conf)
    torch.manual_seed(0)
    agent = A2CAgent("t", params, vec_env=_Spaces(width))
    assert agent.fused_mixed == mixed and agent.use_fused and not agent.mixed_precision and agent.seq_len == 4
    assert agent.minibatch_size == n and agent.obs_shape == (width,) and agent.num_minibatches == minibatches
    return agent


def _errs(a, ref):
    """(max |a - ref| / max |ref|, ||a - ref|| / ||ref||) in float64."""
    a = a.detach().double().reshape(-1)
    ref = ref.detach().double().reshape(-1).to(a.device)
    d = a - ref
    return (float(d.abs().max() / ref.abs().max().clamp_min(1e-300)), float(d.norm() / ref.norm().clamp_min(1e-300)))


def _compared(out):
    """{name: tensor} of everything one step produces that is held to the float64 reference."""
    t = dict(("grad " + k, g) for k, g in out["grads"].items())
    t.update(("stat " + k, torch.as_tensor(v).reshape(1)) for k, v in out["stats"].items())
    t["new mu"], t["new sigma"] = out["mu"], out["sigma"]
    return t


def _bounds(ref, auto, fp32):
    """{name: (max-relative bound, rms-relative bound)}."""
    if fp32:
        return {k: (FP32_BOUND, FP32_BOUND) for k in ref}
    out = {}
    for k in ref:
        bm, br = _errs(auto[k], ref[k])
        assert np.isfinite(bm) and np.isfinite(br), ("autocast baseline not finite", k)
        out[k] = (K * max(bm, FLOOR), K * max(br, FLOOR))
    return out


def _ratios(got, ref, bounds):
    """{name: (max-relative error / its bound, rms-relative error / its bound)}."""
    r = {}
    for k in got:
        em, er = _errs(got[k], ref[k])
        r[k] = (em / bounds[k][0], er / bounds[k][1])
    return r


def _controls(agent, mb, dev):
    """The float64 reference from subtly wrong inputs: {name: gradients}."""
    args = ur.loss_args(agent)
    T = agent.seq_len
    out = {}
    for name in ("dones shifted", "dones ignored", "h0 zeroed", "clip_value flipped"):
        m2, a2 = dict(mb), dict(args)
        if name == "dones shifted":
            m2["dones"] = torch.roll(mb["dones"], 1)
        elif name == "dones ignored":
            m2["dones"] = torch.zeros_like(mb["dones"])
        elif name == "h0 zeroed":
            m2["rnn_states"] = [torch.zeros_like(mb["rnn_states"][0]), mb["rnn_states"][1]]
        else:
            a2["clip_value"] = not args["clip_value"]
        assert a2["seq_len"] == T
        out[name] = _compared(ur.reference_step(agent.model, m2, device=dev, **a2))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_update_gradient_block_against_float64(case):
    name, B, width, mixed, clip_value, entropy_coef, scale, phases = case
    t0 = time.time()
    dev = torch.device("cuda:0")
    agent = _agent(B, width, mixed, clip_value, entropy_coef)
    T = agent.seq_len
    ur.perturb_model(agent.model, seed=1)
    if agent.fused_mixed:
        agent.optimizer.refresh_shadow()            # the 16-bit operand copies of the perturbed weights
        agent.optimizer.amp_state[0] = scale        # the device GradScaler's loss scale
    else:
        assert scale is None and agent._amp is None
    mb = ur.synthetic_minibatch(agent.model, B, T, seed=2, device=dev)
    clipped, vclipped, beyond = ur.loss_branch_shares(agent.model, mb, T)
    assert 0.2 <= clipped <= 0.4 and vclipped > 0.2 and beyond > 0.02, (clipped, vclipped, beyond)
    d = mb["dones"].view(B, T)
    assert bool(d[:, 0].any()) and bool(d.all(1).any()) and bool((d == 0).all(1).any())
    assert all(float(s.abs().mean()) > 0.1 for s in mb["rnn_states"])

    # references first: the step below moves the agent's running statistics and overwrites mb's mu / sigma
    ref_out = ur.reference_step(agent.model, mb, device=dev, **ur.loss_args(agent))
    ref = _compared(ref_out)
    auto = None
    if mixed:
        auto = _compared(ur.reference_step(agent.model, mb, device=dev, dtype=torch.float32, autocast=torch.float16,
                                           loss_scale=scale, **ur.loss_args(agent)))
    bounds = _bounds(ref, auto, not mixed)
    controls = _controls(agent, mb, dev) if name == "b8192_default" else {}

    agent.flat_grads.zero_()
    agent.optimizer.aux.zero_()
    p0 = fused.PHASE_LAUNCHES[0]
    mb_step = dict(mb)
    stats, _mu, _logstd = agent._fused_grad_half(mb_step)
    torch.cuda.synchronize()
    ran = fused.PHASE_LAUNCHES[0] - p0
    assert ran == (1 if phases else 0), (name, ran)
    if agent._amp is not None:
        assert float(agent.optimizer.amp_state[0]) == scale
        assert float(agent.optimizer.found_inf) == 0.0
    unscale = scale if mixed else 1.0
    grads = {k: p.grad.detach() / unscale for k, p in agent.model.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    got_stats = {"a_loss": stats[0], "c_loss": stats[1], "b_loss": stats[2], "entropy": stats[3], "kl": stats[4]}
    got = _compared({"grads": grads, "stats": got_stats, "mu": mb["mu"], "sigma": mb["sigma"]})
    assert mb["mu"].data_ptr() == mb_step["mu"].data_ptr()          # refreshed in place: the dataset sees it
    got["aux kl"] = agent.optimizer.aux[0:1].clone()
    ref["aux kl"], bounds["aux kl"] = ref["stat kl"], bounds["stat kl"]

    ratios = _ratios(got, ref, bounds)
    worst_m = max(ratios, key=lambda k: ratios[k][0])
    worst_r = max(ratios, key=lambda k: ratios[k][1])
    f = K if mixed else 1.0         # reported: kernel error / max(autocast error, FLOOR), or / FP32_BOUND
    report = {"path": "phases" if ran else "fallback", "worst_max": (worst_m, round(ratios[worst_m][0] * f, 3)),
              "worst_rms": (worst_r, round(ratios[worst_r][1] * f, 3))}
    margins = {}
    for cname, ctl in controls.items():
        cr = _ratios({k: v for k, v in ctl.items() if k.startswith("grad ")}, ref, bounds)
        k_ = max(cr, key=lambda k: max(cr[k]))
        margins[cname] = (k_, round(max(cr[k_]), 1))
    report["controls"] = margins

    rms = agent.model.running_mean_std
    for k in ("running_mean", "running_var"):
        report[k] = _errs(getattr(rms, k), ref_out[k])[0]
    report["seconds"] = round(time.time() - t0, 1)
    print("\n[update gradients] %s %s" % (name, report), flush=True)

    bad = {k: v for k, v in ratios.items() if max(v) > 1.0}
    assert not bad, (name, {k: (round(v[0] * f, 3), round(v[1] * f, 3)) for k, v in bad.items()})
    for k in ("running_mean", "running_var"):
        assert report[k] < 1e-9, (k, report[k])
    assert float(rms.count) == float(ref_out["count"])
    for cname, (k_, m) in margins.items():
        assert m >= CONTROL_MARGIN, ("negative control within the bound", cname, k_, m)
    if name == "b8192_default":
        assert set(margins) == {"dones shifted", "dones ignored", "h0 zeroed", "clip_value flipped"}


@pytest.mark.gpu
def test_adaptive_lr_kernel_equals_the_cpu_schedule():
    """``vine_adaptive_lr`` (the device-side AdaptiveScheduler of the non-graphed update) against the CPU branch of
    ``A2CAgent.update_lr_from_kl``, bit for bit: KL below, at and above 0.5 thr and 2 thr (and one float32 step either side
    of each edge), both clamps (min_lr, max_lr), kl_scale 1 and 1/2 (the KL summed over two ranks)."""
    import types
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    thr, lo, hi = 0.008, 1e-6, 1e-2
    f32 = np.float32
    kls = [f32(0.0), f32(1e-4), f32(0.003), f32(0.008), f32(0.012), f32(0.1)]
    for edge in (f32(0.5) * f32(thr), f32(2.0) * f32(thr)):
        kls += [np.nextafter(edge, f32(0.0)), edge, np.nextafter(edge, f32(1.0))]
    lrs = [3e-4, 1.2e-6, 1e-6, 8e-3, 1e-2]
    seen = set()
    for rank_size in (1, 2):
        for lr0 in lrs:
            for kl in kls:
                out = []
                for dev in (torch.device("cpu"), torch.device("cuda:0")):
                    ag = types.SimpleNamespace(multi_gpu=False, is_cuda=dev.type == "cuda", device=dev, rank_size=rank_size,
                                               kl_threshold=thr, min_lr=lo, max_lr=hi,
                                               lr=torch.tensor(lr0, dtype=torch.float32, device=dev))
                    A2CAgent.update_lr_from_kl(ag, torch.tensor(kl * f32(rank_size), dtype=torch.float32, device=dev))
                    out.append(ag.lr.cpu())
                cpu, gpu = out
                assert cpu.view(torch.int32) == gpu.view(torch.int32), (rank_size, lr0, float(kl), float(cpu), float(gpu))
                new, old = float(cpu), float(f32(lr0))
                seen.add("down" if new < old else "up" if new > old else "kept")
                if new == float(f32(lo)) and old < 1.5 * lo:
                    seen.add("min clamp")
                if new == float(f32(hi)) and old * 1.5 > hi:
                    seen.add("max clamp")
    assert seen == {"down", "up", "kept", "min clamp", "max clamp"}, seen
