"""vine_step_eval (include/vine_ppo.h): the evaluation mode of the four-lanes-per-env step kernel -- the policy head's mean in
front of the step, per-episode task statistics behind it.  The ABI mirror on the CPU; on the GPU the kernel against a twin
env stepped through vine_step with its actions, and its accounting against a float64 restatement."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from vine_robot_isaacgymenvs_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_abi_constants_and_mirror():
    text = open(os.path.join(REPO, "include", "vine_ppo.h")).read()
    defines = dict(re.findall(r"#define VINE_(EVAL_[A-Z_]+) (\d+)", text))
    assert len(defines) == 2 + abi.EVAL_EPISODE_FIELDS + abi.EVAL_NUM_TOTALS
    for name, val in defines.items():
        assert getattr(abi, name) == int(val), name
    assert abi.EVAL_EPISODE_FIELDS == 4 and abi.EVAL_NUM_TOTALS == 12
    for name in ("vine_step_eval", "vine_step_eval_rows", "vine_step_eval_args_size"):
        assert name in abi.PPO_PROTOTYPES, name
    # VineEvalArgs <-> abi.EvalArgs: the same fields in the same order
    body = re.search(r"typedef struct VineEvalArgs \{(.*?)\} VineEvalArgs;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"^.*[\s\*]", "", d.strip()) for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in abi.EvalArgs._fields_]
    assert C.sizeof(abi.EvalArgs) == 15 * 8


def test_eval_args_size_matches_the_library():
    from vine_robot_isaacgymenvs_amd import native
    native.build()
    assert native.load().vine_step_eval_args_size() == C.sizeof(abi.EvalArgs)


# --------------------------------------------------------------------------- GPU
N_TWIN, H, A, STEPS, MAX_LEN, SUCCESS_DIST, SOFT_LIMIT = 160, 256, 2, 14, 8, 0.25, 0.3
SHELF = ["task.env.CREATE_SHELF=True", "task.env.USE_NONZERO_CONTACT_FORCE_RESET=True",
         # the shelf's target ranges of tests/helpers.py (f6_cfg)
         "task.env.MIN_TARGET_Y=-0.12", "task.env.MAX_TARGET_Y=-0.02", "task.env.MIN_TARGET_Z=0.56", "task.env.MAX_TARGET_Z=0.66",
         "task.env.MIN_TARGET_DEPTH_IN_OBSTACLE=0.0", "task.env.MAX_TARGET_DEPTH_IN_OBSTACLE=0.1"]


def _make_env(n, overrides, seed=42):
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_config(overrides=["num_envs=%d" % n, "task.env.CREATE_PIPE=False", "task.env.maxEpisodeLength=%d" % MAX_LEN,
                                 "task.env.SUCCESS_DIST=%g" % SUCCESS_DIST, "task.env.MIN_TARGET_Y=-0.4",
                                 "task.env.MAX_TARGET_Y=0.0", "task.env.USE_TIP_LIMIT_HIT_RESET=True"] + overrides)
    cfg["task"]["seed"] = seed
    return isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0",
                                                  graphics_device_id=0, headless=True)


def _head(dev, lib, st):
    """The head tensors of test_rollout_step_in_one_launch_matches_the_three_launches and their prepared products."""
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    p = dict(gamma=1.0 + 0.1 * rnd(H), beta=0.1 * rnd(H))
    p.update(w_mu=0.1 * rnd(A, H), b_mu=0.1 * rnd(A), w_v=0.1 * rnd(1, H), b_v=0.1 * rnd(1))
    p.update(logstd=torch.tensor([-0.3, 0.2], device=dev), hw=torch.empty(3 * H, device=dev), hc=torch.empty(3, device=dev),
             vmean=torch.tensor([0.37], device=dev, dtype=torch.float64), vvar=torch.tensor([2.3], device=dev, dtype=torch.float64),
             counter=torch.tensor([3], device=dev, dtype=torch.int64))
    assert lib.vine_rollout_head_prep(p["gamma"].data_ptr(), p["beta"].data_ptr(), p["w_mu"].data_ptr(), p["b_mu"].data_ptr(),
                                      p["w_v"].data_ptr(), p["b_v"].data_ptr(), p["hw"].data_ptr(), p["hc"].data_ptr(), st) == 0
    return p, rnd


def _eval_state(env, n, dev):
    rows = env.eval_step_rows()
    s = dict(mu=torch.empty(n, A, device=dev), action=torch.empty(n, A, device=dev),
             dones=torch.empty(n, device=dev, dtype=torch.uint8), h=torch.ones(1, n, H, device=dev),
             c=torch.ones(1, n, H, device=dev), hop=torch.ones(n, 352, device=dev), obs=torch.empty(n, env.num_obs, device=dev),
             episode=torch.zeros(abi.EVAL_EPISODE_FIELDS, n, device=dev),
             totals=torch.zeros(rows, abi.EVAL_NUM_TOTALS, device=dev, dtype=torch.float64))
    s["episode"][abi.EVAL_EP_MIN_DIST] = math.inf
    return s


def _eval_args(s, p, y, deterministic, seed=12345):
    a = abi.EvalArgs()
    a.y, a.hw, a.hc, a.logstd = y.data_ptr(), p["hw"].data_ptr(), p["hc"].data_ptr(), p["logstd"].data_ptr()
    a.ln_eps, a.deterministic, a.seed = 1e-5, deterministic, seed
    a.mu_out, a.action_out, a.dones_out = s["mu"].data_ptr(), s["action"].data_ptr(), s["dones"].data_ptr()
    a.h_state, a.c_state, a.h_op, a.h_op_stride = s["h"].data_ptr(), s["c"].data_ptr(), s["hop"].data_ptr() + 4 * 96, 352
    a.episode, a.totals = s["episode"].data_ptr(), s["totals"].data_ptr()
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("overrides", [[], ["task.env.CREATE_PIPE=True"],
                                       ["OBSERVATION_TYPE=TIP_AND_CART_AND_OBJ_INFO", "vine_randomize=False"], SHELF],
                         ids=["free", "pipe", "tipobs", "shelf"])
def test_eval_step_matches_a_twin_and_a_float64_restatement(overrides):
    """Env B runs vine_step_eval (deterministic); its twin A, with introspection armed, is stepped through vine_step with B's
    action_out.  Flags and counters agree exactly, observations and rewards are expected bit-identical (held to the rollout
    twin test's 1e-4; the largest difference is printed), mu agrees with vine_policy_head_rms to that test's 2e-6, the
    LSTM-state rows of finished envs -- and only those -- are cleared.  The accounting (the per-env ``episode`` block and the
    per-workgroup ``totals``) is restated in float64 numpy from A's rew_buf / reset_buf / timeout_buf and state fields: counts,
    lengths and first_reach exactly, sums to rtol 1e-5 (an fp32 sum of <= 64 terms, a running fp32 sum of <= 8 rewards),
    min_dist to 1e-6.  160 envs = 2.5 workgroups in a grid of 4: a partly filled and an idle workgroup."""
    from vine_robot_isaacgymenvs_amd.learning import fused
    lib = fused._lib()
    dev = torch.device("cuda:0")
    N = N_TWIN
    st = torch.cuda.current_stream().cuda_stream
    shelf = overrides is SHELF
    ea, eb = _make_env(N, overrides), _make_env(N, overrides)
    ea.set_introspection(True)
    assert eb.eval_step_rows() == 4 and lib.vine_step_eval_rows(eb._handle) == 4
    p, rnd = _head(dev, lib, st)
    sb = _eval_state(eb, N, dev)
    obs_a = torch.empty(N, ea.num_obs, device=dev)
    scratch = dict(mu=torch.empty(N, A, device=dev), sigma=torch.empty(N, A, device=dev), value=torch.empty(N, 1, device=dev),
                   action=torch.empty(N, A, device=dev), nlp=torch.empty(N, device=dev))
    # float64 restatement
    ep = np.zeros((4, N))
    ep[abi.EVAL_EP_MIN_DIST] = np.inf
    tot = np.zeros((4, abi.EVAL_NUM_TOTALS))
    lengths, margins, worst = set(), [np.inf, np.inf, np.inf], [0.0, 0.0]
    f = abi
    for step in range(STEPS):
        y = rnd(N, H)
        for k in ("h", "c", "hop"):
            sb[k].fill_(1.0)
        # ---- B: one launch;  A: vine_step with B's action
        eb.step_eval_into(_eval_args(sb, p, y, 1), sb["obs"])
        ea.step_into(sb["action"], obs_a)
        assert lib.vine_policy_head_rms(N, A, H, y.data_ptr(), p["w_mu"].data_ptr(), p["b_mu"].data_ptr(), p["w_v"].data_ptr(),
                                        p["b_v"].data_ptr(), p["logstd"].data_ptr(), p["vmean"].data_ptr(), p["vvar"].data_ptr(),
                                        1e-5, 12345, p["counter"].data_ptr(), scratch["mu"].data_ptr(), scratch["sigma"].data_ptr(),
                                        scratch["value"].data_ptr(), scratch["action"].data_ptr(), scratch["nlp"].data_ptr(),
                                        p["gamma"].data_ptr(), p["beta"].data_ptr(), 1e-5, st) == 0
        torch.cuda.synchronize()
        torch.testing.assert_close(sb["mu"], scratch["mu"], rtol=2e-6, atol=2e-6, msg="step %d mu" % step)
        assert torch.equal(sb["action"], sb["mu"])                      # deterministic: the action is the mean
        assert torch.equal(eb.reset_buf, ea.reset_buf) and torch.equal(eb.timeout_buf, ea.timeout_buf), step
        assert torch.equal(eb.progress_buf, ea.progress_buf), step
        done_t = ea.reset_buf != 0
        assert torch.equal(sb["dones"], done_t.to(torch.uint8)), step
        worst[0] = max(worst[0], float((sb["obs"] - obs_a).abs().max()))
        worst[1] = max(worst[1], float((eb.rew_buf - ea.rew_buf).abs().max()))
        torch.testing.assert_close(sb["obs"], obs_a, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(eb.rew_buf, ea.rew_buf, rtol=1e-4, atol=1e-4)
        # rows of finished envs cleared, nothing else touched
        keep = (~done_t).float().view(N, 1)
        assert torch.equal(sb["h"][0], keep.expand(N, H)) and torch.equal(sb["c"][0], keep.expand(N, H)), step
        assert torch.equal(sb["hop"][:, 96:], keep.expand(N, H)) and float(sb["hop"][:, :96].min()) == 1.0, step
        # ---- the restatement, from A
        sa = ea.state.double().cpu().numpy()
        rew, done, to = ea.rew_buf.double().cpu().numpy().reshape(N), done_t.cpu().numpy(), ea.timeout_buf.cpu().numpy() != 0
        dy, dz = sa[f.VF_TIP_Y] - sa[f.VF_TARGET_Y], sa[f.VF_TIP_Z] - sa[f.VF_TARGET_Z]
        dist = np.sqrt(dy * dy + dz * dz)
        reached = dist < np.float32(SUCCESS_DIST)
        rail = np.abs(sa[f.VF_CART_Y]) > np.float32(SOFT_LIMIT)
        tip_limit = sa[f.VF_TIP_Y] < sa[f.VF_TARGET_Y]
        contact = (sa[f.VF_CONTACT_MEAN] > 0) if shelf else np.zeros(N, bool)
        margins = [min(margins[0], np.abs(dist - np.float32(SUCCESS_DIST)).min()),
                   min(margins[1], np.abs(np.abs(sa[f.VF_CART_Y]) - np.float32(SOFT_LIMIT)).min()), min(margins[2], np.abs(dy).min())]
        ep[f.EVAL_EP_RETURN] += rew
        ep[f.EVAL_EP_LENGTH] += 1
        ep[f.EVAL_EP_MIN_DIST] = np.minimum(ep[f.EVAL_EP_MIN_DIST], dist)
        first = (ep[f.EVAL_EP_FIRST_REACH] == 0) & reached
        ep[f.EVAL_EP_FIRST_REACH][first] = ep[f.EVAL_EP_LENGTH][first]
        for b in range(4):
            m = done.copy()
            m[:b * 64] = False
            m[(b + 1) * 64:] = False
            ever = ep[f.EVAL_EP_FIRST_REACH] != 0
            tot[b] += [m.sum(), ep[f.EVAL_EP_RETURN][m].sum(), ep[f.EVAL_EP_LENGTH][m].sum(), (m & ever).sum(), (m & reached).sum(),
                       ep[f.EVAL_EP_FIRST_REACH][m].sum(), dist[m].sum(), ep[f.EVAL_EP_MIN_DIST][m].sum(), (m & to).sum(),
                       (m & rail).sum(), (m & tip_limit).sum(), (m & contact).sum()]
        lengths |= set(ep[f.EVAL_EP_LENGTH][done].astype(int).tolist())
        ep[:, done] = 0.0
        ep[f.EVAL_EP_MIN_DIST][done] = np.inf
        got = sb["episode"].double().cpu().numpy()
        for k in (f.EVAL_EP_LENGTH, f.EVAL_EP_FIRST_REACH):
            assert np.array_equal(got[k], ep[k]), (step, k)
        np.testing.assert_allclose(got[f.EVAL_EP_RETURN], ep[f.EVAL_EP_RETURN], rtol=1e-5, atol=0, err_msg="step %d" % step)
        live = np.isfinite(ep[f.EVAL_EP_MIN_DIST])
        assert np.array_equal(np.isfinite(got[f.EVAL_EP_MIN_DIST]), live)
        np.testing.assert_allclose(got[f.EVAL_EP_MIN_DIST][live], ep[f.EVAL_EP_MIN_DIST][live], rtol=0, atol=1e-6)
    got = sb["totals"].cpu().numpy()
    print("max |obs diff| %.3e  max |rew diff| %.3e  margins %s  totals %s lengths %s"
          % (worst[0], worst[1], margins, tot.sum(0).tolist(), sorted(lengths)))
    counts = [f.EVAL_EPISODES, f.EVAL_LENGTH_SUM, f.EVAL_REACHED_EVER, f.EVAL_REACHED_AT_END, f.EVAL_FIRST_REACH_SUM,
              f.EVAL_END_TIMEOUT, f.EVAL_END_RAIL_LIMIT, f.EVAL_END_TIP_LIMIT, f.EVAL_END_CONTACT]
    assert np.array_equal(got[:, counts], tot[:, counts])
    sums = [f.EVAL_RETURN_SUM, f.EVAL_FINAL_DIST_SUM, f.EVAL_MIN_DIST_SUM]
    np.testing.assert_allclose(got[:, sums], tot[:, sums], rtol=1e-5, atol=0)
    assert not got[3].any() and tot[2, f.EVAL_EPISODES] > 0        # the idle workgroup's row; the partly filled one's
    # the run exercised what it is meant to check, and no float64 test sat on a float32 threshold
    t = tot.sum(0)
    for k in (f.EVAL_END_TIMEOUT, f.EVAL_REACHED_AT_END, f.EVAL_END_RAIL_LIMIT, f.EVAL_END_TIP_LIMIT):
        assert t[k] >= 1, k
    assert 1 in lengths and MAX_LEN in lengths
    if shelf:
        assert t[f.EVAL_END_CONTACT] >= 1
    else:
        assert t[f.EVAL_END_CONTACT] == 0
    assert min(margins) >= 1e-5, margins
    # the entry refuses what it does not cover
    bad = abi.EvalArgs()
    assert lib.vine_step_eval(eb._handle, C.addressof(bad), sb["obs"].data_ptr(), eb.rew_buf.data_ptr(), eb.reset_buf.data_ptr(),
                              eb.progress_buf.data_ptr(), eb.timeout_buf.data_ptr(), st) == abi.ERR_INVALID_ARG == -1
    ea.close(); eb.close()


@pytest.mark.gpu
def test_eval_step_refuses_a_handle_on_the_one_lane_kernel(monkeypatch):
    from vine_robot_isaacgymenvs_amd.learning import fused
    lib = fused._lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    monkeypatch.setenv("VINE_STEP_KERNEL", "lane")          # read by vine_create
    env = _make_env(64, [])
    monkeypatch.delenv("VINE_STEP_KERNEL")
    assert env.step_kernel_name == "vine_step_kernel"
    assert lib.vine_step_eval_rows(env._handle) == 0 and env.eval_step_rows() == 0
    p, rnd = _head(dev, lib, st)
    s = _eval_state(env, 64, dev)
    s["totals"] = torch.zeros(1, abi.EVAL_NUM_TOTALS, device=dev, dtype=torch.float64)
    a = _eval_args(s, p, rnd(64, H), 1)
    assert lib.vine_step_eval(env._handle, C.addressof(a), s["obs"].data_ptr(), env.rew_buf.data_ptr(), env.reset_buf.data_ptr(),
                              env.progress_buf.data_ptr(), env.timeout_buf.data_ptr(), st) == abi.ERR_UNSUPPORTED == -2
    with pytest.raises(NotImplementedError):
        env.step_eval_into(a, s["obs"])
    torch.cuda.synchronize()
    assert int(env.progress_buf.max()) == 0 and not s["totals"].any()
    env.close()


@pytest.mark.gpu
def test_eval_step_samples_unit_normal_noise_keyed_by_the_step_count():
    """deterministic = 0: eps = (action_out - mu_out) / exp(logstd) over 8 steps x 1024 envs x 2 (16384 samples) has
    |mean| < 0.04 and |std - 1| < 0.04 (about 5 standard errors); twins with the same seed draw the same actions; consecutive
    steps draw different noise."""
    from vine_robot_isaacgymenvs_amd.learning import fused
    lib = fused._lib()
    dev = torch.device("cuda:0")
    N = 1024
    st = torch.cuda.current_stream().cuda_stream
    e1, e2 = _make_env(N, []), _make_env(N, [])
    p, rnd = _head(dev, lib, st)
    s1, s2 = _eval_state(e1, N, dev), _eval_state(e2, N, dev)
    eps = []
    for step in range(8):
        y = rnd(N, H)
        e1.step_eval_into(_eval_args(s1, p, y, 0), s1["obs"])
        e2.step_eval_into(_eval_args(s2, p, y, 0), s2["obs"])
        torch.cuda.synchronize()
        assert torch.equal(s1["action"], s2["action"]) and torch.equal(s1["mu"], s2["mu"]) and torch.equal(s1["obs"], s2["obs"])
        eps.append(((s1["action"] - s1["mu"]) / torch.exp(p["logstd"])).cpu())
        if step:
            assert float((eps[-1] - eps[-2]).abs().max()) > 1.0
    eps = torch.stack(eps).double()
    print("eps mean %.4f std %.4f" % (float(eps.mean()), float(eps.std())))
    assert abs(float(eps.mean())) < 0.04 and abs(float(eps.std()) - 1.0) < 0.04
    # another seed: other noise
    e2.step_eval_into(_eval_args(s2, p, y, 0, seed=999), s2["obs"])
    e1.step_eval_into(_eval_args(s1, p, y, 0), s1["obs"])
    torch.cuda.synchronize()
    assert not torch.equal(s1["action"], s2["action"])
    e1.close(); e2.close()
