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
