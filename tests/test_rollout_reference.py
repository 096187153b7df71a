"""The float64 replay of the rollout record (tests/rollout_reference.py) against the agent's stock rollout on the CPU
(``_rollout_body``: the module composition in fp32, the oracle as the env).  The GPU test of the hand-written rollout
(tests/test_rollout_record.py) trusts this helper; here it has to agree with the stock path to fp32 noise, and every
negative control has to leave that noise far behind."""
import numpy as np
import pytest
import torch

from tests import rollout_reference as rr
from tests import update_reference as ur
from tests.test_update_reference import _rel

NOISE = 2e-5            # fp32 module composition against float64, max- and rms-relative
TENSORS = ("mus", "values", "neglogpacs", "snap_h", "snap_c", "h_end", "c_end", "last_values")


def _cpu_agent(obs_type, n):
    from oracle.oracle_vec_task import OracleVecTask
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.learning import a2c_continuous as a2c
    cfg = load_config(overrides=["num_envs=%d" % n, "minibatch_size=%d" % (4 * n), "rl_device=cpu", "OBSERVATION_TYPE=" + obs_type,
                                 "task.env.maxEpisodeLength=6", "task.env.CREATE_PIPE=False"])
    params = cfg["train"]["params"]
    params["config"].update(write_files=False, print_stats=False)
    torch.manual_seed(42)
    agent = a2c.A2CAgent("t", params, vec_env=OracleVecTask(cfg["task"], seed=42))
    agent.init_tensors()
    agent.obs = agent.env_reset()["obs"]
    ur.perturb_model(agent.model, seed=1)
    vms = agent.model.value_mean_std
    vms.running_mean.fill_(0.37); vms.running_var.fill_(2.3)
    agent.set_eval()
    return agent


@pytest.mark.parametrize("obs_type,width", [("POS_AND_FD_VEL_AND_OBJ_INFO", 28), ("TIP_AND_CART_AND_OBJ_INFO", 18)])
def test_replay_matches_the_stock_cpu_rollout(obs_type, width, monkeypatch):
    N = 24
    agent = _cpu_agent(obs_type, N)
    assert not agent.is_cuda and agent.obs_shape == (width,) and not agent._can_fuse_rollout()
    T, L = agent.horizon_length, agent.seq_len
    env = agent.vec_env
    stepped = []
    step = env.step

    def watched(actions):                       # the raw reward and the flags of every step
        out = step(actions)
        stepped.append((out[1].numpy().astype(np.float64), out[2].numpy().copy(), out[3]["time_outs"].numpy().copy()))
        return out
    monkeypatch.setattr(env, "step", watched)
    recs = []
    with torch.no_grad():
        for r in range(3):
            start = [s[0].clone() for s in agent.rnn_states]
            batch = agent.play_steps_rnn()
            recs.append(rr.record(agent, [], batch, start))
    m64 = rr.model_copy(agent.model, torch.float64, "cpu")

    def replay_all(control=None):
        h = torch.zeros(N, agent.model.a2c_network.rnn_units, dtype=torch.float64)
        c, outs = torch.zeros_like(h), []
        for rec in recs:
            outs.append(rr.replay(m64, rec, h, c, L, control))
            h, c = outs[-1]["h_end"], outs[-1]["c_end"]
        return {k: torch.stack([o[k] for o in outs]) for k in TENSORS}
    got = {"mus": "mus", "values": "values", "neglogpacs": "neglogpacs", "snap_h": "mb_h", "snap_c": "mb_c", "h_end": "h_end",
           "c_end": "c_end", "last_values": "last_values"}
    got = {k: torch.stack([rec[v] for rec in recs]) for k, v in got.items()}
    ref = replay_all()
    for k in TENSORS:
        mx, rms = _rel(got[k], ref[k])
        assert mx < NOISE and rms < NOISE, (k, mx, rms)
    for control in rr.CONTROLS:
        worst = max(max(_rel(got[k], v)) for k, v in replay_all(control).items())
        assert worst > 100 * NOISE, (control, worst)
    assert rr.noise_statistics(torch.cat([(rec["actions"] - rec["mus"]) / rec["sigmas"] for rec in recs]))["repeats"] == 0
    twice = torch.cat([recs[0]["actions"], recs[0]["actions"]])
    assert rr.noise_statistics(twice)["repeats"] >= recs[0]["actions"][..., 0].numel()

    # bookkeeping, shaped rewards, GAE
    books = rr.Books(N, agent.games_to_track)
    dones_seen = 0
    for r, rec in enumerate(recs):
        for n in range(T):
            rew, done, tmo = stepped[r * T + n]
            books.step(rew, done)
            dones_seen += int(done.sum())
            shaped = (rew + agent.reward_shift) * agent.reward_scale + agent.gamma * rec["values"][n, :, 0].double().numpy() * tmo
            assert np.abs(rec["rewards"][n, :, 0].numpy() - shaped).max() < 1e-6 * (1.0 + np.abs(shaped).max())
            nxt = rec["dones"][n + 1] if n + 1 < T else rec["dones_end"]
            assert np.array_equal(nxt.numpy(), (done != 0).astype(np.uint8))
        assert np.abs(rec["cur_r"][:, 0].numpy() - books.cur_r).max() <= 1e-6 * books.scale
        assert np.array_equal(rec["cur_l"].numpy(), books.cur_l)
        want, have = books.meter()[:4], rec["meter"].double().numpy()
        assert have[1] == want[1] and have[3] == want[3]
        assert abs(have[0] - want[0]) <= 2e-5 * books.scale and abs(have[2] - want[2]) <= 2e-5 * T
        advs, rets = rr.gae(rec["rewards"], rec["values"], rec["dones"], rec["last_values"], rec["dones_end"],
                            float(agent.gamma), float(agent.tau))
        assert not rec["assembled"]
        err = float((rec["batch_returns"].double() - rets.transpose(0, 1).reshape(-1, 1)).abs().max())
        assert err <= 1e-5, err
    assert dones_seen >= 2 * N


def test_value_normaliser_update_is_the_modules():
    from vine_robot_isaacgymenvs_amd.learning.running_mean_std import RunningMeanStd
    g = torch.Generator().manual_seed(0)
    x = torch.randn(777, 1, generator=g, dtype=torch.float64) * 3.0 + 1.5
    rms = RunningMeanStd((1,))
    rms.running_mean.fill_(0.37); rms.running_var.fill_(2.3); rms.count.fill_(40.0)
    rms.update(x)
    m, v, c = rr.rms_update(0.37, 2.3, 40.0, x)
    assert abs(m - float(rms.running_mean)) < 1e-12 and abs(v - float(rms.running_var)) < 1e-12 and c == float(rms.count)
