"""Every optimiser step of an update against a float64 replay, teacher-forced.

``A2CAgent.train_epoch`` runs unmodified on a synthetic dataset (``play_steps_rnn`` is replaced on the instance by a
function that hands over tests/update_reference.py's ``synthetic_minibatch`` of the whole batch as an assembled dataset;
``prepare_dataset``, ``get_minibatch`` and the step loop are the product's).  Two instance attributes are hooked:
``calc_gradients`` (before the real call: ``keep_margins`` on the minibatch's views of the dataset, the float64
``reference_step`` and the fp16-autocast baseline at the device's current loss scale) and ``optimizer.step`` (the
optimiser's whole state in front of and behind the real call).  Every check of a step starts from the device's own state
in front of that step, so errors do not compound and Adam's sensitivity to the sign of a small gradient never enters.

Per step:
  gradients   the flat block / loss scale, the loss statistics, ``aux[0]``, the new ``mu`` / ``sigma`` against float64 at the
              current fp32 parameters, within test_update_gradients' per-tensor bounds (``K`` x the autocast baseline;
              ``FP32_BOUND`` for the fp32 update).
  Adam        ``exp_avg'``, ``exp_avg_sq'`` and the movement ``p' - p`` of every parameter tensor against
              ``reference_optimizer_step`` fed the device's pre-step state and gradient block.  Baseline: the same step in
              plain float32 torch on the same snapshot (unscale, clip, ``torch.optim.Adam(foreach=False)``); the kernel's
              error may be ``K_ADAM`` x max(baseline error, 2^-24) per tensor and norm.  A step that did nothing is an
              error of 1 in the movement.
  exactly     after a step that ran: shadow == flat_params in 16 bits, the emitted operands (heads, transposed weights,
              LSTM tiles as ``rebuild()`` makes them from that shadow), gradients cleared, flag lowered, step + 1, the loss
              scaling state as the reference says, ``clip_out`` == {norm, coef} to fp32 round-off.  After a skipped step:
              parameters, moments, step, shadow and every operand byte unchanged, scale halved, gradients cleared.
  schedule    the learning rate behind a step is the float32 schedule of ``update_lr_from_kl``'s CPU branch applied to the
              device's KL, bit for bit; the step itself used the old value.
  plumbing    order and range of the minibatches, ``dataset["mu"]`` / ``["sigma"]`` untouched outside the range and the new
              policy inside, the observation normaliser (float64 update in the first mini-epoch, bit-unchanged afterwards),
              ``_stat_rows``, the number of steps.

Negative controls (b64_w18_clip_growth): ``reference_optimizer_step`` recomputed with one subtle mistake (bias correction
with the un-incremented step, clip coefficient left out, unscaled by the post-update scale, learning rate taken after
the schedule, eps inside the square root) must break the Adam bound by ``CONTROL_MARGIN`` on some tensor at some step.

K_ADAM.  Measured on an MI355X, the worst (kernel error / max(float32 torch's error, 2^-24)) over all steps and tensors of
each case, max-relative | rms-relative (tensor @step; profiles/update_trajectory/ratios.txt has every quantity of every case):
                         movement p' - p               exp_avg'                     exp_avg_sq'
    b64_w18_clip_growth    1.422 |   1.570             6.081 |   7.196              184.698 | 170.664
    b256_w28_overflow      1.549 |   1.318             6.335 |   6.412              217.005 | 217.005  (value.bias @1)
    b32_below_trunk        1.526 |   1.415             5.375 |   5.281              216.269 | 216.262
    b64_w28_fp32           1.830 |   1.537             9.055 |   9.049              216.692 | 216.183
The worst is 217.0, hence K_ADAM = 1.5 x 217.0 = 326.  It is exp_avg_sq's everywhere and the same figure everywhere: the
kernel forms 1 - beta2 from the float32 beta2 (0.999 rounds to 0.99900001287: a relative 1.29e-5 = 216 x 2^-24 on the
increment of the second moment), torch.optim.Adam forms it in double.  The bias correction is taken from the same float32
beta2, so the movement does not see it (1.8 at the worst).  The negative controls exceed the bound by a factor of 300 or
more; each run prints the figures.

The gradient half over the steps of an update (kernel error / max(autocast error, FLOOR); the bound is K = 1.5):
    b64_w18_clip_growth    1.351 (grad mu.bias @1)             | 1.260 (grad value.bias @0)
    b256_w28_overflow      1.000 (grad actor_mlp.0.weight @2)  | 1.011 (grad sigma @4)
    b32_below_trunk        0.033 (aux kl @3)                   | 0.033 (aux kl @3)
    b64_w28_fp32           0.033 (aux kl @3; / FP32_BOUND)     | 0.033 (aux kl @3)
b256_w28_overflow starts at a loss scale of 2^23, at which the first backward pass overflows and 2^22 runs: one skipped
step.  More skipped steps would bring a minibatch back in the next mini-epoch with the parameters it was last seen with;
the KL between the policy and itself is then ~1e-5, a difference of 16-bit-rounded means, and its relative error says
nothing (measured from 2^26, four skipped steps: 4.4 x the autocast baseline's on ``stat kl``, everything else inside).
torch's fp16 autocast overflows from 2^19 on at this minibatch; its baseline is then taken at the scale it backs off to.
"""
import time
import types

import numpy as np
import pytest
import torch

from tests import update_reference as ur
from tests.test_update_gradients import CONTROL_MARGIN, FLOOR, FP32_BOUND, K, _agent, _bounds, _compared, _errs, _ratios
from vine_robot_isaacgymenvs_amd.learning import fused

K_ADAM = 326.0              # kernel error <= K_ADAM x max(float32 torch's error, ADAM_FLOOR), per tensor and norm
ADAM_FLOOR = 2.0 ** -24      # float32 unit roundoff
MARGIN = 0.02                # keep_margins: distance of every sample from the loss's branch edges

# id, sequences per minibatch (n = 4 B), width, mixed, clip_value, entropy_coef, minibatches, mini-epochs, configuration
CASES = [
    ("b64_w18_clip_growth", 64, 18, True, False, 0.01, 3, 2,
     dict(truncate_grads=True, grad_norm=1.0, loss_scale_init=2.0 ** 10, loss_scale_growth_interval=2)),
    ("b256_w28_overflow", 256, 28, True, True, 0.0, 2, 3, dict(loss_scale_init=2.0 ** 23)),
    ("b32_below_trunk", 32, 28, True, True, 0.0, 2, 2, dict(loss_scale_init=2.0 ** 12)),
    ("b64_w28_fp32", 64, 28, False, False, 0.01, 2, 2, dict()),
]
INF_STEP = 1                 # b32_below_trunk: the step whose gradient block gets one inf


def _snapshot(agent):
    """The optimiser's state as the device holds it now."""
    opt = agent.optimizer
    _sync(agent)
    s = {k: getattr(opt, k).clone() for k in ("flat_params", "exp_avg", "exp_avg_sq", "flat_grads")}
    s.update(step_t=float(opt.step_t), lr=opt.lr.clone().cpu(), found_inf=float(opt.found_inf), aux0=opt.aux[0:1].clone(),
             amp_state=None if opt.amp_state is None else opt.amp_state.clone().cpu(),
             shadow=None if opt.shadow is None else opt.shadow.clone(), operands=None)
    if opt.operands is not None:
        s["operands"] = {k: v.clone() for k, v in _operand_buffers(opt.operands).items()}
    return s


def _operand_buffers(ops):
    return {"wtile": ops.wtile, "w_hh_tiled": ops.w_hh_tiled, "wts0": ops.wts[0], "wts1": ops.wts[1], "wts2": ops.wts[2],
            "w_heads": ops.w_heads, "b_heads": ops.b_heads}


def _sync(agent):
    if agent.is_cuda:
        torch.cuda.synchronize()


def _rebuilt(ops):
    """What ``rebuild()`` makes of the shadow as it stands, built in the poisoned buffers themselves, which are restored."""
    bufs = _operand_buffers(ops)
    keep = {k: v.clone() for k, v in bufs.items()}
    for v in bufs.values():
        v.view(torch.uint8).fill_(0x5a)
    ops.rebuild()
    torch.cuda.synchronize()
    out = {k: v.clone() for k, v in bufs.items()}
    for k, v in bufs.items():
        v.copy_(keep[k])
    torch.cuda.synchronize()
    return out


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                      b.reshape(-1).contiguous().view(torch.uint8))


def _float32_torch_step(pre, fed, kw, opt):
    """The same step as the stock composition does it, in plain float32 torch on the snapshot: unscale, clip,
    ``torch.optim.Adam(foreach=False)`` -> (params', exp_avg', exp_avg_sq')."""
    p = torch.nn.Parameter(pre["flat_params"].clone())
    g = fed.clone()
    if kw.get("grad_scale", 1.0) != 1.0:
        g.mul_(kw["grad_scale"])
    if pre["amp_state"] is not None:
        g.mul_(pre["amp_state"][0].double().reciprocal().float().to(g.device))      # GradScaler.unscale_
    p.grad = g
    if kw.get("clip") is not None:
        torch.nn.utils.clip_grad_norm_([p], kw["clip"])
    adam = torch.optim.Adam([p], lr=float(pre["lr"]), betas=opt.betas, eps=opt.eps, foreach=False)
    adam.state[p] = {"step": torch.tensor(pre["step_t"]), "exp_avg": pre["exp_avg"].clone(),
                     "exp_avg_sq": pre["exp_avg_sq"].clone()}
    adam.step()
    return p.detach(), adam.state[p]["exp_avg"], adam.state[p]["exp_avg_sq"]


def _per_tensor(names, slices, p0, p, m, v):
    """{"move name" | "exp_avg name" | "exp_avg_sq name": tensor} of one step's results."""
    out = {}
    for k in names:
        sl = slices[k]
        out["move " + k] = p[sl].double().cpu() - p0[sl].double().cpu()
        out["exp_avg " + k] = m[sl].double().cpu()
        out["exp_avg_sq " + k] = v[sl].double().cpu()
    return out


def _cpu_schedule(agent, lr, kl):
    """``update_lr_from_kl``'s CPU branch on float32 scalars -> the new learning rate (a float32 tensor)."""
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    ag = types.SimpleNamespace(multi_gpu=False, is_cuda=False, device=torch.device("cpu"), rank_size=agent.rank_size,
                               kl_threshold=agent.kl_threshold, min_lr=agent.min_lr, max_lr=agent.max_lr,
                               lr=lr.clone().cpu().reshape(()))
    A2CAgent.update_lr_from_kl(ag, kl.detach().clone().cpu().float().reshape(()))
    return ag.lr


def _run(case):
    name, B, width, mixed, clip_value, entropy_coef, nmb, epochs, conf = case
    dev = torch.device(conf.get("device", "cuda:0"))
    agent = _agent(B, width, mixed, clip_value, entropy_coef, minibatches=nmb, mini_epochs=epochs, **conf)
    opt, T, mbs = agent.optimizer, agent.seq_len, 4 * B
    assert agent.mini_epochs_num == epochs and agent.is_adaptive_lr and agent.schedule_type == "legacy"
    ur.perturb_model(agent.model, seed=1)
    if agent.fused_mixed:
        opt.refresh_shadow()
        assert float(opt.amp_state[0]) == conf["loss_scale_init"]
    else:
        assert agent._amp is None and opt.amp_state is None
    whole = ur.synthetic_minibatch(agent.model, B * nmb, T, seed=2, device=dev)
    calls = {"play": 0}

    def play():
        calls["play"] += 1
        batch = {k: v for k, v in whole.items() if k != "range"}
        batch.update(assembled=True, played_frames=nmb * mbs)
        return batch
    agent.play_steps_rnn = play

    names = [k for k, _ in agent.model.named_parameters()]
    slices = {k: slice(off, off + p.numel()) for (k, p), off in zip(agent.model.named_parameters(), opt.offsets)}
    assert [p.data_ptr() for _, p in agent.model.named_parameters()] == [p.data_ptr() for p in opt.params]
    args = ur.loss_args(agent)
    rms = agent.model.running_mean_std
    steps, bad = [], []
    real_calc, real_step = agent.calc_gradients, opt.step

    def finish_previous():
        """What is only visible behind ``calc_gradients``: the write-back into the dataset, the statistics row, the schedule."""
        if not steps or "lr_next" in steps[-1]:
            return
        st = steps[-1]
        _sync(agent)
        st["ds_mu_after"], st["ds_sigma_after"] = agent.dataset["mu"].clone(), agent.dataset["sigma"].clone()
        st["row"] = agent._stat_rows[st["s"]].clone()
        st["lr_next"] = opt.lr.clone().cpu()

    def calc_gradients(mb):
        finish_previous()
        s = len(steps)
        st = {"s": s, "range": mb["range"], "kw": None, "lr_in": opt.lr.clone().cpu()}
        steps.append(st)
        ur.keep_margins(agent.model, mb, T, agent.e_clip, MARGIN, keep_mode=True)
        st["ds_mu"], st["ds_sigma"] = agent.dataset["mu"].clone(), agent.dataset["sigma"].clone()
        st["rms"] = (rms.running_mean.clone(), rms.running_var.clone(), rms.count.clone(), rms.training)
        scale = None if opt.amp_state is None else float(opt.amp_state[0])
        st["scale"] = scale
        st["ref"] = ur.reference_step(agent.model, mb, device=dev, keep_mode=True, **args)
        st["auto"] = None
        if mixed:
            # at the device's scale; where autocast's own backward pass overflows there (the kernels' need not), at the
            # largest power of two below it at which it does not: the scale its GradScaler would back off to
            auto_scale = scale
            while True:
                st["auto"] = ur.reference_step(agent.model, mb, device=dev, dtype=torch.float32, autocast=torch.float16,
                                               loss_scale=auto_scale, keep_mode=True, **args)
                if auto_scale <= 1.0 or all(bool(torch.isfinite(g).all()) for g in st["auto"]["grads"].values()):
                    break
                auto_scale *= 0.5
            st["auto_scale"] = auto_scale
        launches = fused.PHASE_LAUNCHES[0]
        out = real_calc(mb)
        _sync(agent)
        st["launches"] = fused.PHASE_LAUNCHES[0] - launches
        st["returned"] = [t.detach().clone() for t in out]
        st["rms_after"] = (rms.running_mean.clone(), rms.running_var.clone(), rms.count.clone())
        return out

    def step(**kw):
        st = steps[-1]
        assert st["kw"] is None, "two optimiser steps in one calc_gradients"
        st["kw"] = dict(kw)
        st["pre"] = _snapshot(agent)
        start, end = st["range"]
        st["mu_kernel"], st["sigma_kernel"] = agent.dataset["mu"][start:end].clone(), agent.dataset["sigma"][start:end].clone()
        if name == "b32_below_trunk" and st["s"] == INF_STEP:
            assert opt.check_grads and st["pre"]["found_inf"] == 0.0
            opt.flat_grads[slices["a2c_network.rnn.rnn.weight_hh_l0"].start + 77] = float("inf")
        st["fed"] = opt.flat_grads.clone()
        real_step(**kw)
        st["post"] = _snapshot(agent)
        out = opt.clip_out if kw.get("clip_out") is None else kw["clip_out"]
        if kw.get("clip") is not None and out is not None:      # (the CPU path records no {norm, coef})
            st["clip_out"] = out.clone().cpu()
        if opt.operands is not None:
            st["rebuilt"] = _rebuilt(opt.operands)
    agent.calc_gradients = calc_gradients
    opt.step = step

    agent.train_epoch()
    finish_previous()
    assert calls["play"] == 1
    if len(steps) != epochs * nmb or any(st["kw"] is None for st in steps):
        bad.append(("number of optimiser steps", len(steps), [st["kw"] is None for st in steps]))
        return agent, steps, bad, {}

    table = {}                      # quantity -> (worst max ratio, worst rms ratio, step of the worst) in units of the baseline
    report = {"steps": [], "lr": []}
    controls = {w: (None, 0.0) for w in ur.WRONG_STEPS} if name == "b64_w18_clip_growth" else {}

    def note(kind, ratios, factor, s):
        for k, (rm, rr) in ratios.items():
            key = kind + " " + k
            old = table.get(key, (0.0, 0.0, s))
            table[key] = (max(old[0], rm * factor), max(old[1], rr * factor), s if max(rm, rr) * factor > max(old[:2]) else old[2])

    for st in steps:
        s, pre, post, kw, ref_out = st["s"], st["pre"], st["post"], st["kw"], st["ref"]
        mini_ep, i = divmod(s, nmb)
        start, end = st["range"]
        if st["range"] != (i * mbs, (i + 1) * mbs):
            bad.append(("range", s, st["range"]))
        if st["launches"] != (1 if mixed and mbs >= 256 else 0):      # the route: trunk launch | stock modules
            bad.append(("trunk launches", s, st["launches"]))
        scale = st["scale"] if mixed else 1.0

        # ---- gradients
        finite = bool(torch.isfinite(pre["flat_grads"]).all())
        ref = _compared(ref_out)
        ref["aux kl"] = ref["stat kl"]
        got_stats = dict(zip(("a_loss", "c_loss", "entropy", "kl", "b_loss"), st["returned"][:5]))
        # on the device the loss kernels refresh the dataset's mu / sigma in place and park the KL next to the gradients
        # before the optimiser steps; the CPU composition hands all three back
        got = _compared({"grads": {k: pre["flat_grads"][slices[k]] / scale for k in names}, "stats": got_stats,
                         "mu": st["mu_kernel"] if agent.is_cuda else st["returned"][5],
                         "sigma": st["sigma_kernel"] if agent.is_cuda else st["returned"][6]})
        got["aux kl"] = pre["aux0"] if agent.is_cuda else got_stats["kl"].reshape(1)
        if not finite:                      # an overflowed backward pass: the forward half is still held to the reference
            ref = {k: v for k, v in ref.items() if not k.startswith("grad ")}
            got = {k: v for k, v in got.items() if not k.startswith("grad ")}
        auto = None
        if mixed:
            auto = _compared(st["auto"])
            auto["aux kl"] = auto["stat kl"]
        gb = _bounds(ref, auto, not mixed)
        gr = _ratios(got, ref, gb)
        f = K if mixed else 1.0
        note("grad-half", gr, f, s)
        bad += [("gradient", s, k, round(v[0] * f, 3), round(v[1] * f, 3)) for k, v in gr.items() if not max(v) <= 1.0]
        # the dataset behind the step: the new policy inside the range, untouched outside
        inside = _ratios({"new mu": st["ds_mu_after"][start:end], "new sigma": st["ds_sigma_after"][start:end]}, ref, gb)
        bad += [("dataset inside the range", s, k, v) for k, v in inside.items() if not max(v) <= 1.0]
        for k in ("mu", "sigma"):
            a, b = st["ds_%s_after" % k], st["ds_" + k]
            if not (torch.equal(a[:start], b[:start]) and torch.equal(a[end:], b[end:])):
                bad.append(("dataset outside the range moved", s, k))
            if mini_ep == 0 and torch.equal(a[start:end], b[start:end]):      # (later, skipped steps may leave the policy as it was)
                bad.append(("dataset inside the range did not move", s, k))
        row = dict(zip(("a_loss", "c_loss", "b_loss", "entropy", "kl"), st["row"][:5]))
        rr = _ratios({"stat " + k: v.reshape(1) for k, v in row.items()}, ref, gb)
        bad += [("_stat_rows", s, k, v) for k, v in rr.items() if not max(v) <= 1.0]
        # the observation normaliser
        mean0, var0, count0, training = st["rms"]
        if training != (mini_ep == 0):
            bad.append(("normaliser's training flag", s, training))
        if mini_ep == 0:
            e = [_errs(st["rms_after"][0], ref_out["running_mean"])[0], _errs(st["rms_after"][1], ref_out["running_var"])[0]]
            # (the device's kernels sum the batch moments in float64; the CPU composition takes them in float32, and
            # tests/test_update_reference.py holds it to 1e-6)
            if not (max(e) < (1e-9 if agent.is_cuda else 1e-6) and float(st["rms_after"][2]) == float(ref_out["count"]) == float(count0) + mbs):
                bad.append(("normaliser", s, e, float(st["rms_after"][2])))
        elif not all(_bytes_equal(a, b) for a, b in zip(st["rms_after"], (mean0, var0, count0))):
            bad.append(("normaliser moved after the first mini-epoch", s))

        # ---- the Adam step
        state = {"params": pre["flat_params"], "exp_avg": pre["exp_avg"], "exp_avg_sq": pre["exp_avg_sq"],
                 "step": pre["step_t"], "lr": float(pre["lr"]),
                 "amp_state": None if pre["amp_state"] is None else tuple(float(x) for x in pre["amp_state"][:3])}
        sched = kw.get("lr_schedule")
        ref_kw = dict(found_inf=pre["found_inf"] != 0.0 and pre["amp_state"] is not None, grad_scale=kw.get("grad_scale", 1.0),
                      clip=kw.get("clip"), betas=opt.betas, eps=opt.eps)
        if sched is not None:
            ref_kw.update(kl=float(sched[0]), schedule=tuple(sched[1:]))
        R = ur.reference_optimizer_step(state, st["fed"], **ref_kw)
        status = "skipped" if R["skipped"] else "ran"
        if pre["amp_state"] is not None:
            want_amp = torch.tensor(R["amp_state"], dtype=torch.float32)
            if not torch.equal(post["amp_state"][:3], want_amp):
                bad.append(("amp_state", s, post["amp_state"].tolist(), R["amp_state"]))
            if not R["skipped"] and R["amp_state"][0] > state["amp_state"][0]:
                status += " grew"
        if pre["lr"].view(torch.int32).item() != st["lr_in"].view(torch.int32).item():
            bad.append(("the step did not use the old learning rate", s, float(st["lr_in"]), float(pre["lr"])))
        if float(post["lr"]) != R["lr"]:
            bad.append(("learning rate behind the step", s, float(post["lr"]), R["lr"]))
        if bool(post["flat_grads"].any()) or post["found_inf"] != 0.0:
            bad.append(("gradients not cleared or flag left up", s))
        if R["skipped"]:
            for k in ("flat_params", "exp_avg", "exp_avg_sq", "shadow"):
                if pre[k] is not None and not _bytes_equal(pre[k], post[k]):
                    bad.append(("skipped step moved", s, k))
            if post["step_t"] != pre["step_t"]:
                bad.append(("skipped step counted", s))
            if pre["operands"] is not None:
                bad += [("skipped step moved operand", s, k) for k in pre["operands"] if not _bytes_equal(pre["operands"][k], post["operands"][k])]
        else:
            if post["step_t"] != pre["step_t"] + 1.0:
                bad.append(("step_t", s, pre["step_t"], post["step_t"]))
            p32, m32, v32 = _float32_torch_step(pre, st["fed"], kw, opt)
            a_ref = _per_tensor(names, slices, pre["flat_params"], R["params"], R["exp_avg"], R["exp_avg_sq"])
            a_got = _per_tensor(names, slices, pre["flat_params"], post["flat_params"], post["exp_avg"], post["exp_avg_sq"])
            a_base = _per_tensor(names, slices, pre["flat_params"], p32, m32, v32)
            ab = {}
            for k in a_ref:
                bm, br = _errs(a_base[k], a_ref[k])
                ab[k] = (K_ADAM * max(bm, ADAM_FLOOR), K_ADAM * max(br, ADAM_FLOOR))
            ar = _ratios(a_got, a_ref, ab)
            for kind in ("move", "exp_avg", "exp_avg_sq"):
                note("adam " + kind, {k[len(kind) + 1:]: v for k, v in ar.items() if k.startswith(kind + " ")}, K_ADAM, s)
            bad += [("adam", s, k, round(v[0] * K_ADAM, 3), round(v[1] * K_ADAM, 3)) for k, v in ar.items() if not max(v) <= 1.0]
            pad = torch.ones(opt.numel, dtype=torch.bool)
            for sl in slices.values():
                pad[sl] = False
            if bool(post["flat_params"].cpu()[pad].any()):
                bad.append(("padding moved", s))
            for w in controls:
                if w == "bias correction with the old step" and pre["step_t"] == 0.0:
                    continue                    # (1 - beta^0 = 0: not a subtle mistake at the very first step)
                wk = dict(ref_kw)
                if sched is None:               # the schedule runs behind the step: its arguments, for the control only
                    wk.update(kl=float(pre["aux0"]), schedule=(1.0 / agent.rank_size, agent.kl_threshold, agent.min_lr, agent.max_lr))
                W = ur.reference_optimizer_step(state, st["fed"], wrong=w, **wk)
                cr = _ratios(_per_tensor(names, slices, pre["flat_params"], W["params"], W["exp_avg"], W["exp_avg_sq"]), a_ref, ab)
                k_ = max(cr, key=lambda k: max(cr[k]))
                if max(cr[k_]) > controls[w][1]:
                    controls[w] = ("%s @%d" % (k_, s), round(max(cr[k_]), 1))
            # exactly
            if pre["shadow"] is not None and not torch.equal(post["shadow"], post["flat_params"].to(post["shadow"].dtype)):
                bad.append(("shadow", s))
            if post["operands"] is not None:
                net, ops, o = agent.model.a2c_network, opt.operands, post["operands"]
                sh = lambda p_: post["shadow"][slices[p_]]      # noqa: E731
                fp = lambda p_: post["flat_params"][slices[p_]]      # noqa: E731
                A_ = net.mu.weight.shape[0]
                want = {"w_heads": torch.cat([fp("a2c_network.mu.weight").view(A_, -1), fp("a2c_network.value.weight").view(1, -1)]),
                        "b_heads": torch.cat([fp("a2c_network.mu.bias"), fp("a2c_network.value.bias")]),
                        "wts0": sh("a2c_network.rnn.rnn.weight_ih_l0").view(1024, -1)[:, :ops.U].t(),
                        "wts1": sh("a2c_network.actor_mlp.2.weight").view(128, 256).t(),
                        "wts2": sh("a2c_network.actor_mlp.4.weight").view(64, 128).t(),
                        "wtile": st["rebuilt"]["wtile"], "w_hh_tiled": st["rebuilt"]["w_hh_tiled"]}
                bad += [("operand", s, k) for k, v in want.items() if not _bytes_equal(o[k], v)]
                bad += [("operand != rebuild()", s, k) for k in o if not _bytes_equal(o[k], st["rebuilt"][k])]
                if all(_bytes_equal(o[k], pre["operands"][k]) for k in o):
                    bad.append(("operands did not move", s))
        if "clip_out" in st:
            norm, coef = float(st["clip_out"][0]), float(st["clip_out"][1])
            ok = (abs(norm - R["norm"]) <= 1e-6 * R["norm"] and abs(coef - R["coef"]) <= 1e-6) if np.isfinite(R["norm"]) else not np.isfinite(norm)
            if not ok:
                bad.append(("clip_out", s, (norm, coef), (R["norm"], R["coef"])))
        if kw.get("clip") is not None and not R["skipped"]:
            status += " clipped %.3f" % R["coef"] if R["coef"] < 1.0 else " unclipped"
        if mixed and st["auto_scale"] != st["scale"]:
            status += " (autocast baseline at 2^%d)" % round(np.log2(st["auto_scale"]))
        report["steps"].append(status)
        report["lr"].append(float(pre["lr"]))

        # ---- the schedule behind the step (the eager update runs it after calc_gradients returned)
        if sched is None:
            want_lr = _cpu_schedule(agent, post["lr"], st["returned"][3])
            if want_lr.view(torch.int32).item() != st["lr_next"].view(torch.int32).item():
                bad.append(("schedule", s, float(st["lr_next"]), float(want_lr), float(st["returned"][3])))
        if s + 1 < len(steps) and steps[s + 1]["pre"]["lr"].view(torch.int32).item() != st["lr_next"].view(torch.int32).item():
            bad.append(("learning rate changed between the steps", s))
    report["lr"].append(float(steps[-1]["lr_next"]))
    report["controls"] = controls
    return agent, steps, bad, {"report": report, "table": table}


def _worst(table, prefix):
    rows = {k: v for k, v in table.items() if k.startswith(prefix)}
    km, kr = max(rows, key=lambda k: rows[k][0]), max(rows, key=lambda k: rows[k][1])
    return ("%s @%d" % (km[len(prefix) + 1:], rows[km][2]), round(rows[km][0], 3)), ("%s @%d" % (kr[len(prefix) + 1:], rows[kr][2]), round(rows[kr][1], 3))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_optimiser_step_against_a_float64_replay(case):
    if fused.lp_dtype() != torch.float16 and case[3]:
        pytest.skip("bf16 build")
    name = case[0]
    t0 = time.time()
    agent, steps, bad, out = _run(case)
    assert out, (name, bad)
    report, table = out["report"], out["table"]
    report["worst_gradient"] = _worst(table, "grad-half")          # kernel error / max(autocast error, FLOOR), or / FP32_BOUND
    report["worst_adam"] = _worst(table, "adam")                   # kernel error / max(float32 torch's error, ADAM_FLOOR)
    report["seconds"] = round(time.time() - t0, 1)
    print("\n[update trajectory] %s %s" % (name, report), flush=True)
    for k in sorted(table):
        print("[update trajectory table] %-20s %-60s %10.3f %10.3f  @%d" % ((name, k) + table[k]), flush=True)
    for b in bad:
        print("[update trajectory] %s FAILED %s" % (name, b), flush=True)
    assert not bad, (name, bad)
    status = report["steps"]
    lrs = report["lr"]
    assert any(a != b for a, b in zip(lrs, lrs[1:])), ("no learning-rate change", lrs)
    if name == "b64_w18_clip_growth":
        assert any("clipped" in x and "unclipped" not in x for x in status) and any("grew" in x for x in status), status
        assert not any("skipped" in x for x in status), status
        assert set(report["controls"]) == set(ur.WRONG_STEPS)
        for w, (where, m) in report["controls"].items():
            assert m >= CONTROL_MARGIN, ("negative control within the bound", w, where, m)
    elif name == "b256_w28_overflow":
        assert status[0].startswith("skipped") and any(x.startswith("ran") for x in status), status
    elif name == "b32_below_trunk":
        assert [x.startswith("skipped") for x in status] == [s == INF_STEP for s in range(len(status))], status
    else:
        assert all(x.startswith("ran") for x in status), status


CPU_CASE = ("cpu_b32_w18_stock", 32, 18, False, True, 0.01, 2, 2, dict(device="cpu", truncate_grads=True, grad_norm=1.0))


def test_every_optimiser_step_of_the_cpu_update_against_a_float64_replay():
    """The same harness over the CPU update (autograd of the module composition, ``FlatAdam``'s CPU path, the schedule's
    CPU branch): here the loop's write-back into ``dataset["mu"]`` / ``["sigma"]`` is the only writer of the new policy."""
    t0 = time.time()
    agent, steps, bad, out = _run(CPU_CASE)
    assert out, bad
    report, table = out["report"], out["table"]
    report["worst_gradient"], report["worst_adam"] = _worst(table, "grad-half"), _worst(table, "adam")
    report["seconds"] = round(time.time() - t0, 1)
    print("\n[update trajectory] %s %s" % (CPU_CASE[0], report), flush=True)
    assert not bad, bad
    lrs = report["lr"]
    assert any(a != b for a, b in zip(lrs, lrs[1:])), ("no learning-rate change", lrs)
    assert any("clipped" in x and "unclipped" not in x for x in report["steps"]), report["steps"]
