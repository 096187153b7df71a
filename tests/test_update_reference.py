"""The float64 reference of one optimiser step's gradient (tests/update_reference.py) against the agent's stock update
on the CPU (``calc_gradients``: autograd of the module composition in fp32).  The GPU tests of the hand-written update
(tests/test_update_gradients.py) trust this helper; here it has to agree with the stock path to fp32 reduction noise."""
import pytest
import torch

from tests import update_reference as ur


def _rel(a, ref):
    """(max |a - ref| / max |ref|, ||a - ref|| / ||ref||) in float64."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    d = a - ref
    return float(d.abs().max() / ref.abs().max().clamp_min(1e-300)), float(d.norm() / ref.norm().clamp_min(1e-300))


def _cpu_agent(obs_type, **conf):
    from oracle.oracle_vec_task import OracleVecTask
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.learning import a2c_continuous as a2c
    cfg = load_config(overrides=["num_envs=16", "minibatch_size=256", "rl_device=cpu", "OBSERVATION_TYPE=" + obs_type])
    params = cfg["train"]["params"]
    params["config"].update(write_files=False, print_stats=False, **conf)
    torch.manual_seed(42)
    return a2c.A2CAgent("t", params, vec_env=OracleVecTask(cfg["task"], seed=42))


@pytest.mark.parametrize("obs_type,width,clip_value,entropy_coef", [("POS_AND_FD_VEL_AND_OBJ_INFO", 28, True, 0.0),
                                                                    ("TIP_AND_CART_AND_OBJ_INFO", 18, False, 0.01)])
def test_reference_matches_the_stock_cpu_update(obs_type, width, clip_value, entropy_coef, monkeypatch):
    agent = _cpu_agent(obs_type, clip_value=clip_value, entropy_coef=entropy_coef)
    assert not agent.is_cuda and agent.obs_shape == (width,)
    ur.perturb_model(agent.model, seed=1)
    mb = ur.synthetic_minibatch(agent.model, B=64, T=agent.seq_len, seed=2)
    clipped, vclipped, beyond = ur.loss_branch_shares(agent.model, mb, agent.seq_len)
    assert 0.2 <= clipped <= 0.4 and vclipped > 0.2 and beyond > 0.02
    count0 = float(agent.model.running_mean_std.count)
    ref = ur.reference_step(agent.model, mb, **ur.loss_args(agent))
    assert float(agent.model.running_mean_std.count) == count0         # the reference worked on a copy

    captured = {}

    def capture():                     # the gradient block as the backward pass left it, before the optimiser runs
        captured["g"] = agent.flat_grads.clone()
    monkeypatch.setattr(agent, "truncate_gradients_and_step", capture)
    a_loss, c_loss, entropy, kl, b_loss, mu, sigma = agent.calc_gradients(mb)
    views = {k: captured["g"][off:off + p.numel()].view_as(p)
             for (k, p), off in zip(agent.model.named_parameters(), agent.optimizer.offsets)}
    assert set(views) == set(ref["grads"])
    for k, g in views.items():
        mx, rms = _rel(g, ref["grads"][k])
        assert mx < 2e-5 and rms < 1e-5, (k, mx, rms)
    got = {"a_loss": a_loss, "c_loss": c_loss, "entropy": entropy, "b_loss": b_loss, "kl": kl}
    for k in ur.STAT_KEYS:
        assert abs(float(got[k]) - float(ref["stats"][k])) <= 1e-5 * (1.0 + abs(float(ref["stats"][k]))), k
    assert _rel(mu, ref["mu"])[0] < 1e-5 and _rel(sigma, ref["sigma"])[0] < 1e-6
    rms = agent.model.running_mean_std
    for k in ("running_mean", "running_var", "count"):
        assert _rel(getattr(rms, k), ref[k])[0] < 1e-6, k
    assert float(rms.count) == count0 + mb["obs"].shape[0]


# --------------------------------------------------------------------------- the step half: reference_optimizer_step
def _small_net(dtype):
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.ELU(), torch.nn.Linear(7, 3)).to(dtype)


# six steps at init_scale 8, growth_interval 2, max-norm 1: (amplitude of the unscaled gradient, an inf in the block)
#   0 ran (tracker 1) | 1 ran, clipped, scale grows to 16 | 2 overflow: skipped, scale 8 | 3 ran | 4 ran, clipped, grows | 5 ran
_SEQUENCE = [(0.01, False), (3.0, False), (0.5, True), (0.02, False), (5.0, False), (0.01, False)]
_CLIP, _LR, _SCALE0, _INTERVAL = 1.0, 1e-2, 8.0, 2


def _sequence_grads(n):
    g = torch.Generator().manual_seed(7)
    out = []
    for amp, inf in _SEQUENCE:
        x = torch.randn(n, generator=g, dtype=torch.float64) * amp
        if inf:
            x[n // 2] = float("inf")
        out.append(x)
    return out


def _reference_sequence(p0, grads):
    """reference_optimizer_step over the sequence -> (final state, [step outputs])."""
    z = torch.zeros_like(p0)
    state = {"params": p0.clone(), "exp_avg": z, "exp_avg_sq": z.clone(), "step": 0, "lr": _LR,
             "amp_state": (_SCALE0, 0, _INTERVAL)}
    outs = []
    for g in grads:
        out = ur.reference_optimizer_step(state, g * state["amp_state"][0], clip=_CLIP)
        outs.append(out)
        state = {k: out[k] for k in state}
    return state, outs


def test_reference_optimizer_step_matches_gradscaler_clip_and_adam_in_float64():
    net = _small_net(torch.float64)
    params = list(net.parameters())
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])      # noqa: E731
    p0 = flat(params)
    grads = _sequence_grads(p0.numel())
    opt = torch.optim.Adam(params, lr=_LR, eps=1e-8, foreach=False)
    scaler = torch.amp.GradScaler("cpu", init_scale=_SCALE0, growth_interval=_INTERVAL)
    scaler.scale(torch.zeros(()))            # (creates the scale tensor; the gradients below are handed over scaled)
    state = {"params": p0.clone(), "exp_avg": torch.zeros_like(p0), "exp_avg_sq": torch.zeros_like(p0), "step": 0,
             "lr": _LR, "amp_state": (_SCALE0, 0, _INTERVAL)}
    seen = set()
    for s, g in enumerate(grads):
        scale = scaler.get_scale()
        assert scale == state["amp_state"][0]
        off = 0
        for p in params:
            p.grad = (g[off:off + p.numel()] * scale).view_as(p).clone()
            off += p.numel()
        before = flat(params)
        scaler.unscale_(opt)
        norm = torch.nn.utils.clip_grad_norm_(params, _CLIP)
        scaler.step(opt)
        scaler.update()
        out = ur.reference_optimizer_step(state, g * scale, clip=_CLIP)
        ran = not torch.equal(flat(params), before)
        assert ran == (not out["skipped"]), s
        assert out["amp_state"][0] == scaler.get_scale() and out["amp_state"][1] == int(scaler._growth_tracker), s
        if ran:
            assert abs(out["norm"] - float(norm)) <= 1e-12 * float(norm), s
            st = [opt.state[p] for p in params]
            assert out["step"] == int(st[0]["step"])
            for k, got in (("params", flat(params)), ("exp_avg", flat([x["exp_avg"] for x in st])),
                           ("exp_avg_sq", flat([x["exp_avg_sq"] for x in st]))):
                mx, rms = _rel(out[k], got)
                assert mx < 1e-12 and rms < 1e-12, (s, k, mx, rms)
            seen.add("clipped" if out["coef"] < 1.0 else "unclipped")
            if out["amp_state"][0] > scale:
                seen.add("grown")
        else:
            assert out["amp_state"][0] == 0.5 * scale and out["amp_state"][1] == 0 and out["step"] == state["step"]
            assert all(torch.equal(out[k], state[k]) for k in ("params", "exp_avg", "exp_avg_sq"))
            seen.add("skipped")
        state = {k: out[k] for k in state}
    assert seen == {"clipped", "unclipped", "grown", "skipped"} and state["step"] == 5
    assert float((state["params"] - p0).abs().max()) > 3 * _LR          # five steps of about lr each


def test_reference_optimizer_step_flag_schedule_and_wrong_variants():
    """A raised flag skips a finite block; the schedule acts on the learning rate after the step used the old one; each
    negative-control variant differs from the right step."""
    p0 = torch.linspace(-1.0, 1.0, 11, dtype=torch.float64)
    g = torch.linspace(0.3, -0.2, 11, dtype=torch.float64)
    state = {"params": p0, "exp_avg": 0.1 * g, "exp_avg_sq": 0.01 * g * g, "step": 3, "lr": 3e-4, "amp_state": (4.0, 1, 2)}
    out = ur.reference_optimizer_step(state, 4.0 * g, found_inf=True)
    assert out["skipped"] and out["amp_state"] == (2.0, 0, 2) and torch.equal(out["params"], p0) and out["step"] == 3
    sched = (1.0, 0.008, 1e-6, 1e-2)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))      # noqa: E731
    lr0 = f32(3e-4)
    state["lr"] = lr0
    plain = ur.reference_optimizer_step(state, 4.0 * g, clip=0.1)
    assert plain["coef"] < 1.0 and plain["amp_state"] == (8.0, 0, 2) and plain["lr"] == lr0
    for kl, want in ((0.1, f32(f32(3e-4) / 1.5)), (0.001, f32(f32(3e-4) * 1.5)), (0.008, lr0)):
        out = ur.reference_optimizer_step(state, 4.0 * g, clip=0.1, kl=kl, schedule=sched)
        assert abs(out["lr"] - want) <= 1e-7 * want and torch.equal(out["params"], plain["params"]), kl
    assert ur.adaptive_lr(1.2e-6, 0.1, 1.0, 0.008, 1e-6, 1e-2) == f32(1e-6)
    assert ur.adaptive_lr(8e-3, 0.002, 0.5, 0.008, 1e-6, 1e-2) == f32(1e-2)
    # (eps = 1e-8 under the root is 1e-4 beside sqrt(v): it shows where the gradients are of that size or smaller)
    small = dict(state, exp_avg=1e-4 * state["exp_avg"], exp_avg_sq=1e-8 * state["exp_avg_sq"])
    for w in ur.WRONG_STEPS:
        st, gs = (small, 4e-4 * g) if w == "eps inside the root" else (state, 4.0 * g)
        move = ur.reference_optimizer_step(st, gs, clip=0.1)["params"] - p0
        out = ur.reference_optimizer_step(st, gs, clip=0.1, kl=0.1, schedule=sched, wrong=w)
        d = float(((out["params"] - p0) - move).norm() / move.norm())
        assert d > 0.05, (w, d)


def test_flat_adam_cpu_path_follows_the_reference_sequence():
    """FlatAdam's CPU path (no loss scaling there: it gets the unscaled gradients of the steps that ran; the overflow step
    is the one a GradScaler in front of it skips) against the float64 sequence.  Bound: the moments are a handful of
    float32 operations (1e-6); a parameter of size ~0.5 is rounded to 2^-24 relative at each of the five steps while it
    moves by about five learning rates, 5 x 3e-8 / 0.05 = 3e-6 of the movement, hence 1e-5."""
    from vine_robot_isaacgymenvs_amd.learning.flat_adam import FlatAdam
    net = _small_net(torch.float32)
    params = list(net.parameters())
    opt = FlatAdam(params, _LR, eps=1e-8)
    p0 = torch.cat([p.detach().reshape(-1) for p in params]).double()
    n = p0.numel()
    assert opt.num_params == n
    index = torch.cat([torch.arange(off, off + p.numel()) for p, off in zip(opt.params, opt.offsets)])
    grads = _sequence_grads(n)
    ref, outs = _reference_sequence(p0, grads)
    for g, out in zip(grads, outs):
        if out["skipped"]:
            continue
        opt.flat_grads[index] = g.float()
        opt.step(clip=_CLIP)
        assert float(opt.flat_grads.abs().max()) == 0.0
    assert float(opt.step_t) == ref["step"] == 5
    for k, got in (("exp_avg", opt.exp_avg[index]), ("exp_avg_sq", opt.exp_avg_sq[index])):
        mx, rms = _rel(got, ref[k])
        assert mx < 1e-6 and rms < 1e-6, (k, mx, rms)
    mx, rms = _rel(opt.flat_params[index].double() - p0, ref["params"] - p0)
    assert mx < 1e-5 and rms < 1e-5, (mx, rms)


# --------------------------------------------------------------------------- keep_margins
def _synthetic_minibatch_before_keep_margins(model, B, T, seed, e_clip=0.2):
    """``synthetic_minibatch`` as it stood with the nudge written inline (CPU only): what its output must stay equal to."""
    import copy
    import math
    g = torch.Generator().manual_seed(seed)
    net = model.a2c_network
    n, F_, H = B * T, net.actor_mlp[0].weight.shape[1], net.rnn_units
    A = net.mu.weight.shape[0]
    obs = torch.randn(n, F_, generator=g) * 1.5 + 0.3
    h0 = torch.randn(1, B, H, generator=g) * 0.5
    c0 = torch.randn(1, B, H, generator=g) * 0.5
    kind = torch.randint(0, 10, (B,), generator=g)
    d = (torch.rand(B, T, generator=g) < 0.3)
    d[kind < 3] = False
    d[kind < 3, 0] = True
    d[kind == 3] = True
    d[(kind >= 4) & (kind < 8)] = False
    d[kind >= 8, 0] = False
    dones = d.reshape(n).to(torch.uint8)
    lookup, net.op_weight_lookup = net.op_weight_lookup, None
    try:
        m = copy.deepcopy(model)
    finally:
        net.op_weight_lookup = lookup
    m = m.double().train()
    with torch.no_grad():
        mu, value, logstd = ur._forward(m, obs.double(), h0[0].double(), c0[0].double(), dones, T)
        sigma = torch.exp(logstd).expand_as(mu)
        actions = (mu + sigma * torch.randn(n, A, generator=g).double()).float().double()
        nlp = m.neglogp(actions, mu, sigma, logstd.expand_as(mu))
    margin = 0.02
    log_ratio = ur._away(torch.randn(n, generator=g).double() * 0.2, (math.log(1 - e_clip), math.log(1 + e_clip)), margin)
    dv = value - (value + torch.randn(n, 1, generator=g).double() * 0.3)
    dv = torch.sign(dv) * ur._away(dv.abs(), (e_clip,), margin)
    old_values = value - dv
    returns = value + torch.randn(n, 1, generator=g).double()
    clipped = dv.abs() > e_clip
    mid = (value + old_values + torch.sign(dv) * e_clip) / 2
    returns = torch.where(clipped, mid + ur._away(returns - mid, (0.0,), margin), returns)
    return {"obs": obs, "dones": dones, "rnn_states": [h0, c0], "actions": actions.float(),
            "old_logp_actions": (nlp + log_ratio).float(), "advantages": torch.randn(n, generator=g),
            "old_values": old_values.float(), "returns": returns.float(),
            "mu": (mu + torch.randn(n, A, generator=g).double() * 0.1).float(),
            "sigma": (sigma * torch.exp(torch.randn(n, A, generator=g).double() * 0.1)).float(), "range": (0, n)}


def _edge_distances(model, mb, T, e_clip=0.2):
    """Per sample, in float64: distance of the log ratio from its nearer clip edge, of |value - old_values| from e_clip,
    and (value-clipped samples only, else inf) of the return from the point where the critic's max switches."""
    import math
    m = ur._copy_of(model, "cpu").double()
    with torch.no_grad():
        mu, value, logstd = ur._forward(m, mb["obs"].double(), mb["rnn_states"][0][0].double(),
                                        mb["rnn_states"][1][0].double(), mb["dones"], T)
        sigma = torch.exp(logstd).expand_as(mu)
        nlp = m.neglogp(mb["actions"].double(), mu, sigma, logstd.expand_as(mu))
        lr = mb["old_logp_actions"].double() - nlp
        d_ratio = torch.minimum((lr - math.log(1 - e_clip)).abs(), (lr - math.log(1 + e_clip)).abs())
        dv = value - mb["old_values"].double().reshape(value.shape)
        d_value = (dv.abs() - e_clip).abs()
        mid = (value + mb["old_values"].double().reshape(value.shape) + torch.sign(dv) * e_clip) / 2
        d_ret = torch.where(dv.abs() > e_clip, (mb["returns"].double().reshape(value.shape) - mid).abs(),
                            torch.full_like(mid, float("inf")))
    return d_ratio.reshape(-1), d_value.reshape(-1), d_ret.reshape(-1)


@pytest.mark.parametrize("obs_type,seed", [("POS_AND_FD_VEL_AND_OBJ_INFO", 2), ("TIP_AND_CART_AND_OBJ_INFO", 2),
                                           ("TIP_AND_CART_AND_OBJ_INFO", 0)])
def test_synthetic_minibatch_is_unchanged_by_factoring_keep_margins_out(obs_type, seed):
    agent = _cpu_agent(obs_type)
    ur.perturb_model(agent.model, seed=1)
    T = agent.seq_len
    new = ur.synthetic_minibatch(agent.model, B=64, T=T, seed=seed)
    old = _synthetic_minibatch_before_keep_margins(agent.model, B=64, T=T, seed=seed)
    assert set(new) == set(old)
    for k, v in old.items():
        if k == "rnn_states":
            assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(new[k], v))
        elif k == "range":
            assert new[k] == v
        else:
            assert new[k].dtype == v.dtype and new[k].shape == v.shape and new[k].is_contiguous(), k
            assert torch.equal(new[k].view(torch.uint8), v.view(torch.uint8)), k       # bit for bit
    assert min(float(d.min()) for d in _edge_distances(agent.model, new, T)) > 0.0199


def test_keep_margins_restores_the_margins_for_a_moved_policy():
    """After the weights moved (as an optimiser step moves them) some samples lie within the margin of an edge again;
    keep_margins, in place on float32 views, moves exactly those and no others, and honours the normaliser's eval flag."""
    agent = _cpu_agent("TIP_AND_CART_AND_OBJ_INFO")
    ur.perturb_model(agent.model, seed=1)
    T, margin = agent.seq_len, 0.02
    whole = ur.synthetic_minibatch(agent.model, B=64, T=T, seed=2)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for p in agent.model.parameters():
            p.add_(3e-3 * torch.sign(torch.randn(p.shape, generator=g)))
    agent.model.running_mean_std.eval()
    count0 = float(agent.model.running_mean_std.count)
    mb = {k: (v if k in ("rnn_states", "range") else v[:128]) for k, v in whole.items()}       # views of the first half
    mb["rnn_states"] = [s[:, :32].contiguous() for s in whole["rnn_states"]]
    m_eval = ur._copy_of(agent.model, "cpu", keep_mode=True)
    assert not m_eval.running_mean_std.training and ur._copy_of(agent.model, "cpu").running_mean_std.training
    before = {k: whole[k].clone() for k in ("old_logp_actions", "old_values", "returns")}
    model_eval = agent.model            # distances for the policy as the step will see it: statistics frozen
    frozen = ur._copy_of(model_eval, "cpu")
    frozen.running_mean_std.count.fill_(1e30)        # (a training-mode update that moves nothing)
    d0 = _edge_distances(frozen, mb, T)
    assert min(float(d.min()) for d in d0) < margin           # the moved policy put samples near an edge
    ur.keep_margins(agent.model, mb, T, 0.2, margin, keep_mode=True)
    assert float(agent.model.running_mean_std.count) == count0
    d1 = _edge_distances(frozen, mb, T)
    assert min(float(d.min()) for d in d1) > 0.99 * margin
    for k, v in before.items():
        assert torch.equal(whole[k][128:], v[128:]), k             # outside the views nothing moved
        assert not torch.equal(whole[k][:128], v[:128]), k         # inside, in place
    far = (d0[0] > margin)
    assert torch.equal(whole["old_logp_actions"][:128][far], before["old_logp_actions"][:128][far])
