"""The optimiser step in five launches: the Adam launch writes the forward pass's parameter-derived operands
(``vine_adam_step_emit``, ``FlatAdam.enable_operand_set``) and the MLP forward runs as phase 0 of ``vine_trunk_phases``.

Everything here is a bit-for-bit comparison against the route it replaces: the operands against what ``vine_copy_batched``
builds from the 16-bit shadow, the five-phase launch against ``vine_mlp3_elu_mfma`` followed by the four-phase launch,
training with ``fused.MLP_PHASE`` on against off."""
import ctypes as C
import re
import os

import numpy as np
import pytest
import torch

from vine_robot_isaacgymenvs_amd import abi
from vine_robot_isaacgymenvs_amd.learning import fused

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fp16_build():
    if fused.lp_dtype() != torch.float16:
        pytest.skip("bf16 build")


# --------------------------------------------------------------------------- 1. emitted operands == copied operands
def _default_parameters(F_in, dev):
    """The default network's parameter shapes, in the module's order (408 k parameters at F_in = 28)."""
    g = torch.Generator(device="cpu").manual_seed(3)
    shapes = [("W1", (256, F_in)), ("b1", (256,)), ("W2", (128, 256)), ("b2", (128,)), ("W3", (64, 128)), ("b3", (64,)),
              ("w_ih", (1024, 64 + F_in)), ("w_hh", (1024, 256)), ("b_ih", (1024,)), ("b_hh", (1024,)), ("ln_g", (256,)),
              ("ln_b", (256,)), ("v_w", (1, 256)), ("v_b", (1,)), ("mu_w", (2, 256)), ("mu_b", (2,)), ("sigma", (2,))]
    return {k: torch.nn.Parameter((torch.randn(s, generator=g) * 0.1).to(dev)) for k, s in shapes}


@pytest.mark.gpu
@pytest.mark.parametrize("F_in", [28, 18])
def test_operands_written_by_adam_equal_the_copied_ones(F_in):
    """Four Adam steps through vine_adam_step_emit -- ordinary, clipped, skipped (found_inf), the one after the skip: after
    each, every derived buffer holds what vine_copy_batched builds from the shadow; over the skipped step not a byte
    moves.  w_ih has 92 (F_in = 28: four columns are one 8-byte store) or 82 valid columns (rows straddle a thread's four
    elements)."""
    _fp16_build()
    from vine_robot_isaacgymenvs_amd.learning.flat_adam import FlatAdam
    dev = torch.device("cuda:0")
    P = _default_parameters(F_in, dev)
    opt = FlatAdam(list(P.values()), 1e-2)
    opt.enable_lp16_shadow()
    opt.enable_loss_scaling(init_scale=4.0)
    ops = opt.enable_operand_set([P["W1"], P["W2"], P["W3"]], P["w_ih"], P["w_hh"], P["mu_w"], P["mu_b"], P["v_w"], P["v_b"])
    assert ops is not None and opt.operands is ops and ops.emit_jobs[0] == 10
    assert opt.num_params == (408261 if F_in == 28 else 395461)      # the whole block of the default network
    bufs = {"wtile": ops.wtile, "w_hh_tiled": ops.w_hh_tiled, "wts0": ops.wts[0], "wts1": ops.wts[1], "wts2": ops.wts[2],
            "w_heads": ops.w_heads, "b_heads": ops.b_heads}
    g = torch.Generator(device="cpu").manual_seed(5)

    def snapshot():
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in bufs.items()}

    def copied():
        """What vine_copy_batched builds from the shadow as it stands (into the poisoned buffers themselves)."""
        keep = snapshot()
        for v in bufs.values():
            v.view(torch.uint8).fill_(0x5a)
        ops.rebuild()
        out = snapshot()
        for k, v in bufs.items():
            v.copy_(keep[k])
        return out

    for name, kw, inf in (("ordinary", {}, False), ("clipped", {"clip": 0.5}, False), ("skipped", {}, True),
                          ("after the skip", {"clip": 0.5}, False)):
        before, shadow0, scale0 = snapshot(), opt.shadow.clone(), opt.loss_scale
        opt.flat_grads.copy_((torch.randn(opt.numel, generator=g) * 4.0).to(dev))
        if inf:
            opt.found_inf.fill_(1.0)
        opt.step(**kw)
        after = snapshot()
        if inf:
            assert torch.equal(opt.shadow, shadow0) and opt.loss_scale == 0.5 * scale0, name
            assert all(torch.equal(after[k].view(torch.uint8), before[k].view(torch.uint8)) for k in bufs), name
        else:
            assert not torch.equal(opt.shadow, shadow0), name
            assert all(not torch.equal(after[k], before[k]) for k in bufs), name
            if "clip" in kw:
                assert float(opt.clip_out[1]) < 1.0, name            # the clip really bit
        ref = copied()
        for k in bufs:
            assert torch.equal(after[k].view(torch.uint8), ref[k].view(torch.uint8)), (name, k)
        assert torch.equal(opt.shadow, opt.flat_params.to(opt.shadow.dtype)), name
    assert float(opt.step_t) == 3.0


# --------------------------------------------------------------------------- 2. five phases == MLP launch + four phases
def _trunk_case(B, F_in, dev):
    """Random inputs of one vine_trunk_phases call at B sequences x T = 4, and a factory of zeroed output sets."""
    T, H, U, NH, A_ = 4, 256, 64, 3, 2
    n = B * T
    lp = fused.lp_dtype()
    g = torch.Generator(device="cpu").manual_seed(B + F_in)

    def rnd(*shape, scale=1.0, dtype=torch.float32):
        return (torch.randn(shape, generator=g) * scale).to(dev).to(dtype)
    done = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
    done.view(B, T)[0] = 1                      # a sequence that is done at every step
    done.view(B, T)[1] = 0
    inp = {
        "raw": rnd(n, F_in), "mean": rnd(F_in, scale=0.3).double(), "var": (torch.rand(F_in, generator=g) + 0.5).to(dev).double(),
        "W1": rnd(256, F_in, scale=0.1, dtype=lp), "b1": rnd(256, scale=0.1), "W2": rnd(128, 256, scale=0.06, dtype=lp),
        "b2": rnd(128, scale=0.1), "W3": rnd(64, 128, scale=0.09, dtype=lp), "b3": rnd(64, scale=0.1),
        "wtile": rnd(4 * H * (96 + H), scale=0.05, dtype=lp), "w_hh_tiled": rnd(4 * H * H, scale=0.05, dtype=lp),
        "b_ih": rnd(4 * H, scale=0.1), "b_hh": rnd(4 * H, scale=0.1), "c0": rnd(B, H, scale=0.5), "h0": rnd(B, H, scale=0.5),
        "done": done.to(dev), "ln_g": 1.0 + rnd(H, scale=0.1), "ln_b": rnd(H, scale=0.1), "w_heads": rnd(NH, H, scale=0.1),
        "b_heads": rnd(NH, scale=0.1), "logstd": rnd(A_, scale=0.1), "actions": rnd(n, A_), "old_neglogp": 2.0 + rnd(n, scale=0.3),
        "adv": rnd(n), "old_values": rnd(n), "returns": rnd(n), "old_mu": rnd(n, A_, scale=0.3),
        "old_sigma": 1.0 + 0.1 * torch.rand((n, A_), generator=g).to(dev), "wt0": rnd(U, 4 * H, scale=0.05, dtype=lp),
        "wt1": rnd(128, 64, scale=0.09, dtype=lp), "wt2": rnd(256, 128, scale=0.06, dtype=lp),
    }

    def outputs():
        z = lambda *s, dtype=lp: torch.zeros(s, device=dev, dtype=dtype)      # noqa: E731
        f32 = torch.float32
        return {"xfull": z(n, 96), "act1": z(n, 256), "act2": z(n, 128), "h_out": z(B * (T + 1), H), "c_all": z(T + 1, B, H),
                "gates": z(T, B, 4 * H), "c_last": z(B, H, dtype=f32), "heads": z(n, NH, dtype=f32), "d_out": z(n, H),
                "ln_partial": z(n // 128, (2 + NH) * H, dtype=f32), "loss_partial": z(abi.PPO_LOSS_SCRATCH_FLOATS, dtype=f32),
                "stats": z(8, dtype=f32), "grad_logstd": z(A_, dtype=f32), "grad_mu_bias": z(A_, dtype=f32),
                "grad_value_bias": z(1, dtype=f32), "kl_out": z(1, dtype=f32), "logstd_grad_accum": z(A_, dtype=f32),
                "dG": z(n, 4 * H), "bias_partial": z(B // 32, 4 * H, dtype=f32), "gz1": z(n, 256), "gz2": z(n, 128), "gz3": z(n, 64),
                "part1": z(n // 128, 256, dtype=f32), "part2": z(n // 128, 128, dtype=f32), "part3": z(n // 128, 64, dtype=f32)}
    return inp, outputs


def _trunk_args(B, F_in, i, o, bias, bias2, phase0):
    ta = abi.TrunkArgs()
    p = lambda t: t.data_ptr()      # noqa: E731
    ta.B, ta.T = B, 4
    ta.x, ta.ldx, ta.w_tiled, ta.bias = p(o["xfull"]), 96, p(i["wtile"]), p(bias)
    ta.c0, ta.h0, ta.done = p(i["c0"]), p(i["h0"]), p(i["done"])
    ta.h_out, ta.c_all, ta.gates, ta.c_last = p(o["h_out"]), p(o["c_all"]), p(o["gates"]), p(o["c_last"])
    ta.ln_gamma, ta.ln_beta, ta.ln_eps = p(i["ln_g"]), p(i["ln_b"]), 1e-5
    ta.w_heads, ta.b_heads, ta.logstd = p(i["w_heads"]), p(i["b_heads"]), p(i["logstd"])
    ta.actions, ta.old_neglogp, ta.advantages, ta.old_values = p(i["actions"]), p(i["old_neglogp"]), p(i["adv"]), p(i["old_values"])
    ta.returns, ta.old_mu, ta.old_sigma = p(i["returns"]), p(i["old_mu"]), p(i["old_sigma"])
    ta.e_clip, ta.clip_value, ta.critic_coef, ta.entropy_coef, ta.bounds_coef, ta.soft_bound = 0.2, 1, 2.0, 0.01, 1e-4, 1.1
    ta.alpha = 1.0
    ta.heads, ta.d_out, ta.ln_partial, ta.loss_partial = p(o["heads"]), p(o["d_out"]), p(o["ln_partial"]), p(o["loss_partial"])
    ta.stats, ta.grad_logstd = p(o["stats"]), p(o["grad_logstd"])
    ta.grad_mu_bias, ta.grad_value_bias = p(o["grad_mu_bias"]), p(o["grad_value_bias"])
    ta.kl_out, ta.logstd_grad_accum = p(o["kl_out"]), p(o["logstd_grad_accum"])
    ta.w_hh_tiled, ta.dgates, ta.bias_partial = p(i["w_hh_tiled"]), p(o["dG"]), p(o["bias_partial"])
    ta.wt0, ta.ldw0, ta.wt1, ta.ldw1, ta.wt2, ta.ldw2 = p(i["wt0"]), 1024, p(i["wt1"]), 64, p(i["wt2"]), 128
    ta.a3, ta.a3_stride, ta.a2, ta.a1 = p(o["xfull"]), 96, p(o["act2"]), p(o["act1"])
    ta.gz3, ta.gz2, ta.gz1 = p(o["gz3"]), p(o["gz2"]), p(o["gz1"])
    ta.part3, ta.part2, ta.part1 = p(o["part3"]), p(o["part2"]), p(o["part1"])
    if bias2 is not None:
        ta.bias2 = p(bias2)
    if phase0:
        ta.mlp_raw, ta.mlp_F_in, ta.mlp_mean, ta.mlp_var, ta.mlp_eps, ta.mlp_clip = p(i["raw"]), F_in, p(i["mean"]), p(i["var"]), 1e-5, 5.0
        ta.mlp_w1, ta.mlp_ldw1, ta.mlp_b1 = p(i["W1"]), F_in, p(i["b1"])
        ta.mlp_w2, ta.mlp_ldw2, ta.mlp_b2 = p(i["W2"]), 256, p(i["b2"])
        ta.mlp_w3, ta.mlp_ldw3, ta.mlp_b3 = p(i["W3"]), 128, p(i["b3"])
    return ta


@pytest.mark.gpu
@pytest.mark.parametrize("B,F_in", [(32, 28), (96, 18), (32 * 257, 28)], ids=["one_workgroup", "three_workgroups", "257_workgroups"])
def test_five_phases_equal_the_mlp_launch_plus_four_phases(B, F_in):
    """vine_trunk_phases with its phase-0 fields against vine_mlp3_elu_mfma followed by the four-phase launch, same inputs:
    every output buffer bit for bit.  n = 128 (one workgroup; the stand-alone MLP runs its 4-wave form here), 384, and one
    workgroup more than the chip has CUs.  The five-phase side also takes the LSTM bias as two pointers (b_ih, b_hh),
    the other side their fp32 sum."""
    _fp16_build()
    dev = torch.device("cuda:0")
    lib = fused._lib()
    st = torch.cuda.current_stream().cuda_stream
    i, outputs = _trunk_case(B, F_in, dev)
    n = 4 * B
    five, four = outputs(), outputs()
    assert lib.vine_trunk_phases(C.byref(_trunk_args(B, F_in, i, five, i["b_ih"], i["b_hh"], True)), st) == 0
    w1p = torch.zeros((256, 32), device=dev, dtype=fused.lp_dtype())
    w1p[:, :F_in] = i["W1"]
    bias = i["b_ih"] + i["b_hh"]
    x = four["xfull"]
    assert lib.vine_mlp3_elu_mfma(n, x.data_ptr() + 2 * 64, 96, i["raw"].data_ptr(), F_in, i["mean"].data_ptr(),
                                  i["var"].data_ptr(), 1e-5, 5.0, w1p.data_ptr(), i["b1"].data_ptr(), 256, i["W2"].data_ptr(), 256,
                                  i["b2"].data_ptr(), 128, i["W3"].data_ptr(), 128, i["b3"].data_ptr(), 64, 1.0,
                                  four["act1"].data_ptr(), four["act2"].data_ptr(), x.data_ptr(), 96, st) == 0
    assert lib.vine_trunk_phases(C.byref(_trunk_args(B, F_in, i, four, bias, None, False)), st) == 0
    torch.cuda.synchronize()
    for k in five:
        assert torch.equal(five[k], four[k]), k
    for k in ("xfull", "act1", "act2", "h_out", "gates", "heads", "d_out", "dG", "gz1", "gz2", "gz3", "part1", "loss_partial"):
        assert bool(torch.isfinite(five[k].float()).all()) and float(five[k].float().abs().max()) > 0.0, k
    # a zeroed tail is the four-phase launch: x, a1, a2 stay inputs
    again = outputs()
    for k in ("xfull", "act1", "act2"):
        again[k].copy_(four[k])
    assert lib.vine_trunk_phases(C.byref(_trunk_args(B, F_in, i, again, bias, None, False)), st) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(again[k], four[k]) for k in four)


# --------------------------------------------------------------------------- 3. training is bit-identical across the routes
def _train(monkeypatch, phase, num_envs, minibatch, iterations=4, after_init=None):
    from vine_robot_isaacgymenvs_amd import load_config, native
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    monkeypatch.setattr(fused, "MLP_PHASE", phase)
    lib = native.load()
    calls = {"prep": 0}
    real = lib.vine_mlp3_elu_mfma_prep

    def counting(*a):
        calls["prep"] += 1
        return real(*a)
    monkeypatch.setattr(lib, "vine_mlp3_elu_mfma_prep", counting)
    cfg = load_config(overrides=["num_envs=%d" % num_envs, "minibatch_size=%d" % minibatch])
    cfg["task"]["seed"] = 42
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0",
                                                  graphics_device_id=0, headless=True)
    params = cfg["train"]["params"]
    params["config"].update(write_files=False, print_stats=False, use_graphs=True, mixed_precision=True)
    torch.manual_seed(0)
    agent = A2CAgent("t", params, vec_env=env)
    assert agent.fused_mixed and (agent.optimizer.operands is not None) == phase
    agent.init_tensors()
    agent.obs = agent.env_reset()["obs"]
    if after_init is not None:
        after_init(agent)
    launches0, rides0 = fused.PHASE_LAUNCHES[0], fused.RIDES[0]
    for _ in range(iterations):          # (the later iterations replay the captured update)
        agent.train_epoch()
    torch.cuda.synchronize()
    assert iterations < 4 or agent.graph_status["update"].startswith("graph")
    opt = agent.optimizer
    out = {"flat_params": opt.flat_params.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(),
           "step_t": opt.step_t.clone(), "amp_state": opt.amp_state.clone(), "stats": agent._stat_rows.clone()}
    counts = {"prep": calls["prep"], "launches": fused.PHASE_LAUNCHES[0] - launches0, "rides": fused.RIDES[0] - rides0}
    monkeypatch.setattr(lib, "vine_mlp3_elu_mfma_prep", real)
    env.close()
    return out, counts


@pytest.mark.gpu
@pytest.mark.parametrize("num_envs,minibatch", [(64, 1024), (2048, 16384)])
def test_training_is_bit_identical_with_the_mlp_forward_as_phase_0(num_envs, minibatch, monkeypatch):
    """Two eager and two graph-replayed iterations with MLP_PHASE on and off: parameters, both moments, step counter,
    loss-scaling state and the loss statistics agree bit for bit; on the new route every trunk launch carried the MLP (no
    vine_mlp3_elu_mfma_prep call at all) and the forward passes count as rides."""
    _fp16_build()
    on, con = _train(monkeypatch, True, num_envs, minibatch)
    off, coff = _train(monkeypatch, False, num_envs, minibatch)
    assert con["launches"] > 0 and con["launches"] == coff["launches"]
    assert con["prep"] == 0 and con["rides"] == con["launches"]
    assert coff["prep"] == coff["launches"]
    for k in on:
        assert bool(torch.isfinite(on[k]).all()) and torch.equal(on[k], off[k]), k
    assert float(on["step_t"]) > 0


# --------------------------------------------------------------------------- 4. no stale operands
def _other_weights(agent):
    """A checkpoint with different weights: the model's state dict, every floating-point entry moved."""
    g = torch.Generator(device="cpu").manual_seed(11)
    sd = {}
    for k, v in agent.model.state_dict().items():
        sd[k] = v + (0.02 * torch.randn(v.shape, generator=g)).to(v.device, v.dtype) if v.is_floating_point() and v.dim() >= 2 else v.clone()
    return sd


@pytest.mark.gpu
def test_no_stale_operands_after_a_checkpoint_load(monkeypatch):
    """load_state_dict of other weights + refresh_shadow(): the optimiser steps that follow agree bit for bit between the
    routes (the operand set was rebuilt, not left at the old weights)."""
    _fp16_build()

    def load(agent):
        agent.model.load_state_dict(_other_weights(agent))
        agent.optimizer.refresh_shadow()
    on, con = _train(monkeypatch, True, 64, 1024, iterations=1, after_init=load)
    off, _ = _train(monkeypatch, False, 64, 1024, iterations=1, after_init=load)
    plain, _ = _train(monkeypatch, True, 64, 1024, iterations=1)
    assert con["prep"] == 0 and con["launches"] > 0
    for k in on:
        assert torch.equal(on[k], off[k]), k
    assert not torch.equal(on["flat_params"], plain["flat_params"])      # the loaded weights really differ


@pytest.mark.gpu
def test_no_stale_operands_after_the_parameter_broadcast(monkeypatch):
    """The one-rank multi-GPU path (multi_gpu = True, world size 1): broadcast_parameters() after the weights were replaced
    refreshes the shadow and with it the operand set."""
    _fp16_build()
    import torch.distributed as dist

    def broadcast(agent):
        with torch.no_grad():
            for k, v in _other_weights(agent).items():
                agent.model.state_dict()[k].copy_(v)
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        monkeypatch.setattr(agent, "multi_gpu", True)
        agent.broadcast_parameters()          # (its refresh_shadow is what is under test)
        monkeypatch.setattr(agent, "multi_gpu", False)
    try:
        on, con = _train(monkeypatch, True, 64, 1024, iterations=1, after_init=broadcast)
        off, _ = _train(monkeypatch, False, 64, 1024, iterations=1, after_init=broadcast)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    assert con["prep"] == 0 and con["launches"] > 0
    for k in on:
        assert torch.equal(on[k], off[k]), k


# --------------------------------------------------------------------------- 5. the ABI mirror (no GPU)
def test_trunk_args_tail_and_emit_prototype_match_the_header():
    """What tests/test_abi.py does not see by itself: the ORDER and types of the fields appended to VineTrunkArgs, that a
    zeroed tail is what a default-constructed mirror holds, and the argument count of vine_adam_step_emit."""
    text = open(os.path.join(REPO, "include", "vine_ppo.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct VineTrunkArgs \{(.*?)\} VineTrunkArgs;", text, re.S).group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        ctype = C.c_void_p if m.group(3) else {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}[m.group(2)]
        fields += [(name.strip(), ctype) for name in m.group(4).split(",")]
    assert fields == [(k, t) for k, t in abi.TrunkArgs._fields_]
    names = [k for k, _ in fields]
    tail = names[names.index("part1") + 1:]
    assert tail[0] == "bias2" and tail[1] == "mlp_raw" and "mlp_w1" in tail and len(tail) == 16
    ta = abi.TrunkArgs()
    assert all(not getattr(ta, k) for k in tail)
    proto = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"int vine_adam_step_emit\((.*?)\);", proto, re.S).group(1).split(",")
    restype, argtypes = abi.PPO_PROTOTYPES["vine_adam_step_emit"]
    assert restype is C.c_int and len(argtypes) == len(args) == 34
    for a, t in zip(args, argtypes):
        a = a.strip()
        want = (C.c_void_p if "*" in a else C.c_float if a.startswith("float") else C.c_int64 if a.startswith("int64_t")
                else C.c_int32)
        assert t is want, a
