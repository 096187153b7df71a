"""ENV_PARAMS on the GPU: vine_step_kernel's per-env instantiation (include/vine_env_params.h) against the same kernel without a
table, against uniform handles, against the oracle; the routing; a captured graph; the task class and the entry points.

The shapes: 70 envs = two waves, the second partial; delays cycling 0..8 inside one wave; 12-step episodes, so that resets and
time-outs occur inside every 40-step run.  "Bit-identical" below is literal: float tensors are compared as 32-bit words."""
import ctypes as C
import glob
import types

import numpy as np
import pytest
import torch

from oracle import vine_oracle as vo
from tests.env_params_sets import NUM_SETS, set_cfg, table_of
from tests.helpers import base_cfg, f6_cfg, random_state
from tests.test_hip_parity import QPOS, compare_step
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params

pytestmark = pytest.mark.gpu

N, T, MAX_LEN = 70, 40, 12


@pytest.fixture(scope="module")
def Lane():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    from tests.hip_env import HipEnv as H

    def bind(self, table):
        if table is None:
            self.table_t = None
            native.check(self.lib.vine_bind_env_params(self.h, None), self.lib)
        else:
            env_params.check_table(self.lib, self.cfg, table)
            self.table_t = torch.as_tensor(np.ascontiguousarray(table, np.float32)).to(self.dev).contiguous()
            assert self.table_t.shape == (abi.VP_COUNT, self.n)
            torch.cuda.synchronize(self.dev)
            native.check(self.lib.vine_bind_env_params(self.h, self.table_t.data_ptr()), self.lib)
        assert self.lib.vine_env_params_bound(self.h) == int(table is not None)

    def kernel_name(self):
        return self.lib.vine_step_kernel_name(self.h).decode()

    return type("HipEnvLane", (H,), {"kernel": "lane", "bind": bind, "kernel_name": kernel_name})


def own_table(env):
    return np.repeat(env_params.config_row(env.lib, env.cfg)[:, None], env.n, axis=1)


def actions_for(n, steps, seed=3):
    return torch.as_tensor(np.random.default_rng(seed).uniform(-1.3, 1.3, (steps, n, 2)).astype(np.float32))


def rollout(env, actions):
    """Step ``env`` through ``actions[T, n, 2]``; every output and the whole state block after every step, on the host."""
    rec = {k: [] for k in ("obs", "rew", "reset", "progress", "timeouts", "state")}
    for a in actions:
        env.step_t(a.to(env.dev).contiguous(), sync=False)
        for k, t in (("obs", env.obs_t), ("rew", env.rew_t), ("reset", env.reset_t), ("progress", env.progress_t),
                     ("timeouts", env.timeouts_t), ("state", env.state_t)):
            rec[k].append(t.clone())
    torch.cuda.synchronize(env.dev)
    return {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bit_equal(a, b, envs=None, what=""):
    """Every recorded array of two rollouts, bit for bit (``envs``: only these env indices)."""
    for k in a:
        x, y = bits(a[k]), bits(b[k])
        if envs is not None:
            axis = 2 if k == "state" else 1
            x, y = np.take(x, envs, axis=axis), np.take(y, envs, axis=axis)
        assert np.array_equal(x, y), "%s: %s differs in %d words" % (what, k, np.count_nonzero(x != y))


def saw_resets_and_timeouts(rec):
    return rec["reset"].sum() > 0 and rec["timeouts"].sum() > 0 and (rec["progress"][1:] == 0).any()


def case_cfg(case):
    if case in ("free-obs0", "free-obs1"):
        return base_cfg(N, int(case[-1]), False, max_episode_length=MAX_LEN, seed=21)
    if case in ("shelf", "pipe"):
        cfg = f6_cfg(N, 1, 0, "shelf_contact_reset" if case == "shelf" else "pipe")
        cfg.max_episode_length, cfg.seed = MAX_LEN, 22
        return cfg
    cfg = base_cfg(N, 0, True, max_episode_length=MAX_LEN, seed=23, action_delay=int(case[-1]))
    cfg.obs_noise_std, cfg.action_noise_std, cfg.dyn_scale_min, cfg.dyn_scale_max = 0.01, 0.02, 0.9, 1.1
    return cfg


_BASELINES = {}


def baseline(Lane, case):
    """The unbound one-lane handle's 40-step run of a case, computed once."""
    if case not in _BASELINES:
        env = Lane(case_cfg(case))
        assert env.kernel_name() == "vine_step_kernel"
        _BASELINES[case] = rollout(env, actions_for(N, T))
        env.close()
        assert saw_resets_and_timeouts(_BASELINES[case]), case
    return _BASELINES[case]


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", ["free-obs0", "free-obs1", "shelf", "pipe", "rand-delay0", "rand-delay1", "rand-delay3"])
def test_own_row_table_changes_nothing(Lane, case):
    """A table filled with the configuration's own row against the unbound one-lane kernel: same seed, same actions, 40
    steps; observations, rewards, flags, counters and the whole state block after every step, bit for bit."""
    ref = baseline(Lane, case)
    env = Lane(case_cfg(case))
    env.bind(own_table(env))
    assert env.kernel_name() == "vine_step_kernel"
    got = rollout(env, actions_for(N, T))
    env.close()
    assert_bit_equal(got, ref, what=case)


# ---------------------------------------------------------------------------------------------------------------- 2
def het_cfg():
    cfg = base_cfg(N, 0, True, max_episode_length=MAX_LEN, seed=31)
    cfg.obs_noise_std, cfg.action_noise_std, cfg.dyn_scale_min, cfg.dyn_scale_max = 0.01, 0.02, 0.9, 1.1
    return cfg


@pytest.fixture(scope="module")
def het_run(Lane):
    """The 70-env handle whose env e carries parameter set e % 9, 40 steps."""
    env = Lane(het_cfg())
    table = table_of(env.lib, env.cfg, N)
    env.bind(table)
    rec = rollout(env, actions_for(N, T, seed=4))
    env.close()
    assert saw_resets_and_timeouts(rec)
    return rec, table


def test_nine_plants_in_one_batch_equal_nine_uniform_handles(Lane, het_run):
    """Env e of the heterogeneous handle against env e of the unbound handle created with set e % 9 in its VineConfig (same
    seed, same actions): bit for bit, every step.  The delay is the set index, so one wave holds delays 0..8."""
    het, table = het_run
    assert sorted(set(table[abi.VP_ACTION_DELAY, :64].tolist())) == list(range(NUM_SETS))
    for g in range(NUM_SETS):
        env = Lane(set_cfg(het_cfg(), g))
        assert np.array_equal(own_table(env)[:, 0], table[:, g])
        uni = rollout(env, actions_for(N, T, seed=4))
        env.close()
        assert_bit_equal(het, uni, envs=np.arange(g, N, NUM_SETS), what="set %d" % g)
    # and the sets do differ: env 0 (set 0) and env 1 (set 1) part ways
    assert not np.array_equal(het["state"][-1][abi.VF_Q0:abi.VF_Q0 + 6, 0], het["state"][-1][abi.VF_Q0:abi.VF_Q0 + 6, 1])


# ---------------------------------------------------------------------------------------------------------------- 3
def _composite(oracles):
    """Env e of oracle e % 9, as one oracle-like object for compare_step."""
    pick = lambda get, axis: np.stack([np.take(get(oracles[e % NUM_SETS]), e, axis=axis) for e in range(N)], axis=axis)   # noqa: E731
    return types.SimpleNamespace(reset_buf=pick(lambda o: o.reset_buf, 0), progress=pick(lambda o: o.progress, 0),
                                 timeouts=pick(lambda o: o.timeouts, 0), obs=pick(lambda o: o.obs, 0), rew=pick(lambda o: o.rew, 0),
                                 state=pick(lambda o: np.asarray(o.state, np.float64), 1))


@pytest.mark.parametrize("precision,tol", [("f32", (2e-5, 2e-3, 2e-3)), ("f64", (1e-4, 1e-2, 1e-2))])
def test_heterogeneous_step_matches_nine_oracles(Lane, precision, tol):
    """One step from a random mid-episode state with resets and time-outs seeded as test_hip_parity's seed_both does,
    randomisation on, against nine OracleEnvs (one per parameter set) at single_step_case's tolerances for the one-lane
    kernel."""
    cfg = het_cfg()
    rng = np.random.default_rng(9)
    hip = Lane(cfg)
    hip.bind(table_of(hip.lib, cfg, N))
    oracles = [vo.OracleEnv(set_cfg(cfg, g), precision) for g in range(NUM_SETS)]
    st = random_state(rng, N, cfg)
    for s in range(1, abi.MAX_DELAY):            # every slot of the FIFO rings holds something: delays up to 8 read them
        st[abi.VF_FIFO0 + 2 * s] = rng.uniform(-1, 1, N)
        st[abi.VF_FIFO0 + 2 * s + 1] = rng.uniform(-0.1, 3.0, N)
    reset = (rng.uniform(size=N) < 0.15).astype(np.int64)
    progress = rng.integers(0, cfg.max_episode_length - 1, N)
    progress[: N // 16] = cfg.max_episode_length - 2
    hip.set_state(st)
    hip.set_flags(reset, progress)
    hip.step_count = 7
    for o in oracles:
        o.state[:] = st.astype(o.real)
        o.reset_buf[:], o.progress[:], o.step_count = reset, progress, 7
    actions = rng.uniform(-1.3, 1.3, (N, 2))
    out = hip.step(actions)
    for o in oracles:
        o.step(actions)
    orc = _composite(oracles)
    compare_step(out, orc, hip, *tol)
    assert hip.step_count == 8 and orc.reset_buf.sum() > 0 and orc.timeouts.sum() > 0
    hip.close()
    for o in oracles:
        o.close()


def test_heterogeneous_trajectory_tracks_nine_oracles(Lane):
    """40 steps against the float32 oracles at test_trajectory_tracks_oracle's tolerances (its randomisation settings)."""
    cfg = base_cfg(N, randomize=True, max_episode_length=MAX_LEN, seed=33)
    hip = Lane(cfg)
    hip.bind(table_of(hip.lib, cfg, N))
    oracles = [vo.OracleEnv(set_cfg(cfg, g), "f32") for g in range(NUM_SETS)]
    rng = np.random.default_rng(5)
    worst_q, mismatched = 0.0, np.zeros(N, bool)
    for t in range(T):
        a = rng.uniform(-1, 1, (N, 2))
        obs, rew, rst, to = hip.step(a)
        for o in oracles:
            o.step(a)
        orc = _composite(oracles)
        mismatched |= (rst != orc.reset_buf)
        ok = ~mismatched
        worst_q = max(worst_q, np.abs(hip.state[QPOS][:, ok] - orc.state[QPOS][:, ok]).max())
        np.testing.assert_allclose(obs[ok], orc.obs[ok], rtol=0, atol=2e-2)
        np.testing.assert_allclose(rew[ok], orc.rew[ok], rtol=1e-4, atol=5e-3)
        np.testing.assert_array_equal(hip.progress[ok], orc.progress[ok])
    print("mismatched %d of %d, worst |dq| %.3g" % (mismatched.sum(), N, worst_q))
    assert mismatched.mean() < 0.02
    assert worst_q < 5e-3
    hip.close()
    for o in oracles:
        o.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_one_column_reaches_one_env(Lane):
    """Env 5's damping alone is changed: env 5 leaves test 1's run, every other env stays on it bit for bit (a transposed or
    mis-strided table would move others)."""
    ref = baseline(Lane, "free-obs0")
    env = Lane(case_cfg("free-obs0"))
    table = own_table(env)
    table[abi.VP_DAMPING, 5] = 0.05
    env.bind(table)
    got = rollout(env, actions_for(N, T))
    env.close()
    others = np.array([e for e in range(N) if e != 5])
    assert_bit_equal(got, ref, envs=others, what="envs other than 5")
    assert not np.array_equal(bits(got["state"][:, abi.VF_Q0:abi.VF_Q0 + 6, 5]), bits(ref["state"][:, abi.VF_Q0:abi.VF_Q0 + 6, 5]))
    assert not np.array_equal(bits(got["obs"][:, 5]), bits(ref["obs"][:, 5]))


# ---------------------------------------------------------------------------------------------------------------- 5
def test_binding_routes_to_the_one_lane_kernel_and_unbinding_leaves_no_trace(Lane):
    """512 envs on the four-lane kernel: binding switches the kernel, the fused rollout and evaluation steps answer
    VINE_ERR_UNSUPPORTED and report no rows; after unbinding, 8 further steps equal those of a handle that was never bound
    and starts from the same state and step count, bit for bit (randomisation on: the step count keys every draw, and it is
    re-based on the other kernel's grid at each switch)."""
    n = 512
    Quad = type("HipEnvQuad", (Lane,), {"kernel": "quad"})
    cfg = base_cfg(n, 0, True, max_episode_length=MAX_LEN, seed=41)
    cfg.obs_noise_std, cfg.action_noise_std, cfg.dyn_scale_min, cfg.dyn_scale_max = 0.01, 0.02, 0.9, 1.1
    lib = native.load()
    acts = actions_for(n, 16, seed=6)
    a = Quad(cfg)
    assert a.kernel_name() == "vine_step_quad_kernel" and lib.vine_step_rollout_blocks(a.h) == 8 and lib.vine_step_eval_rows(a.h) == 8
    rollout(a, acts[:4])
    a.bind(own_table(a))
    assert a.kernel_name() == "vine_step_kernel"
    assert lib.vine_step_rollout_blocks(a.h) == 0 and lib.vine_step_eval_rows(a.h) == 0
    assert a.step_count == 4
    # arguments that pass the entry points' own checks (never dereferenced: the answer comes before any launch)
    buf = torch.zeros(4096, device=a.dev)
    ra, ea = abi.RolloutArgs(), abi.EvalArgs()
    for args in (ra, ea):
        for name, ctype in args._fields_:
            if ctype is C.c_void_p:
                setattr(args, name, buf.data_ptr())
        args.h_op_stride = 256
    out = (a.obs_t.data_ptr(), a.rew_t.data_ptr(), a.reset_t.data_ptr(), a.progress_t.data_ptr(), a.timeouts_t.data_ptr(), None)
    assert lib.vine_step_rollout(a.h, C.addressof(ra), *out) == abi.ERR_UNSUPPORTED
    assert lib.vine_step_eval(a.h, C.addressof(ea), *out) == abi.ERR_UNSUPPORTED
    rollout(a, acts[4:8])
    assert a.step_count == 8
    torch.cuda.synchronize()
    b = Quad(cfg)                                  # never bound: takes over a's state, flags and step count
    b.state_t.copy_(a.state_t)
    b.reset_t.copy_(a.reset_t)
    b.progress_t.copy_(a.progress_t)
    b.step_count = 8
    a.bind(None)
    assert a.kernel_name() == b.kernel_name() == "vine_step_quad_kernel" and lib.vine_step_rollout_blocks(a.h) == 8
    assert a.step_count == 8
    ra_, rb_ = rollout(a, acts[8:]), rollout(b, acts[8:])
    assert a.step_count == b.step_count == 16
    a.close(); b.close()
    assert_bit_equal(ra_, rb_, what="after unbinding")
    assert saw_resets_and_timeouts(rb_)


# ------------------------------------------------------------------------------------------------- the task class: 6, 7
SPEC = {"DAMPING": [0.01, 0.05], "ACTION_DELAY": {"values": [0, 2]}}


def _make_env(n, spec, extra=(), seed=42):
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_config(overrides=["num_envs=%d" % n, "task.env.CREATE_PIPE=False", "task.env.maxEpisodeLength=%d" % MAX_LEN] + list(extra))
    cfg["task"]["seed"] = seed
    cfg["task"]["env"]["ENV_PARAMS"] = spec
    return isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0",
                                                  graphics_device_id=0, headless=True)


def test_captured_steps_read_the_table_at_replay():
    """Four steps with a bound table captured in a graph, replayed twice with one column rewritten by set_env_params in
    between, against the same eight steps issued eagerly: bit for bit."""
    n = N
    acts = actions_for(n, 8, seed=7).cuda()
    new_damping = torch.linspace(0.05, 0.01, n)

    def between(env):
        env.set_env_params({"DAMPING": new_damping})
        assert torch.equal(env.env_params[abi.VP_DAMPING].cpu(), new_damping)

    eager = _make_env(n, SPEC)
    obs_e = torch.zeros(8, n, eager.num_obs, device="cuda")
    for k in range(8):
        if k == 4:
            between(eager)
        eager.step_into(acts[k], obs_e[k])
    torch.cuda.synchronize()

    graphed = _make_env(n, SPEC)
    a_in = torch.zeros(4, n, 2, device="cuda")
    obs_g = torch.zeros(4, n, graphed.num_obs, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for k in range(4):
            graphed.step_into(a_in[k], obs_g[k])
    got = []
    for half in range(2):
        if half == 1:
            between(graphed)
        a_in.copy_(acts[4 * half:4 * half + 4])
        g.replay()
        torch.cuda.synchronize()
        got.append(obs_g.clone())
    got = torch.cat(got)
    assert graphed.step_count == eager.step_count == 8
    assert torch.equal(got.view(torch.int32), obs_e.view(torch.int32))
    for name in ("state", "rew_buf", "reset_buf", "progress_buf", "timeout_buf"):
        x, y = getattr(graphed, name), getattr(eager, name)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), name
    # the rewrite mattered: without it the second half is another trajectory
    plain = _make_env(n, SPEC)
    obs_p = torch.zeros(8, n, plain.num_obs, device="cuda")
    for k in range(8):
        plain.step_into(acts[k], obs_p[k])
    torch.cuda.synchronize()
    assert torch.equal(obs_p[:4], obs_e[:4]) and not torch.equal(obs_p[4:], obs_e[4:])
    with pytest.raises(ValueError, match="SMOOTHING_ALPHA_INFLATE"):
        eager.set_env_params({"SMOOTHING_ALPHA_INFLATE": 1.5})
    with pytest.raises(ValueError, match="unknown"):
        eager.set_env_params({"MASS": 1.0})
    for e in (eager, graphed, plain):
        e.close()
    unbound = _make_env(n, {})
    assert unbound.env_params is None
    with pytest.raises(RuntimeError, match="no per-env parameter table"):
        unbound.set_env_params({"DAMPING": 0.03})
    unbound.close()


def test_task_class_builds_checks_and_binds_the_table(caplog):
    import logging
    with caplog.at_level(logging.INFO):
        env = _make_env(512, SPEC)
    try:
        expect = env_params.build_table(SPEC, env._vcfg, int(env._vcfg.seed), 512, 0, lib=env._lib)
        assert env.env_params.shape == (abi.VP_COUNT, 512) and env.env_params.dtype == torch.float32
        assert np.array_equal(env.env_params.cpu().numpy(), expect)
        assert tuple(env.env_param_names) == abi.ENV_PARAM_ROW_NAMES
        assert set(expect[abi.VP_ACTION_DELAY].tolist()) == {0.0, 2.0} and len(np.unique(expect[abi.VP_DAMPING])) > 400
        # the routing the trainer and the player decide by: no fused rollout step, the player's stock path
        assert env.step_kernel_name == "vine_step_kernel" and env.rollout_step_blocks() == 0 and env.eval_step_rows() == 0
        assert env._lib.vine_env_params_bound(env._handle) == 1
        assert any("ENV_PARAMS" in r.message and "vine_step_quad_kernel -> vine_step_kernel" in r.message for r in caplog.records)
    finally:
        env.close()
    with pytest.raises(ValueError, match="ACTION_DELAY"):
        _make_env(64, {"ACTION_DELAY": [0, 9]})
    with pytest.raises(ValueError, match="DAMPNG"):
        _make_env(64, {"DAMPNG": 0.02})


def test_train_and_play_entries_with_env_params(tmp_path, monkeypatch, capsys):
    """Two training iterations (horizon 8) through train.py's entry with ENV_PARAMS, EPISODE_LOG and RECORD_TRAJECTORIES on,
    then test=True on the checkpoint: finite scalars, the table in the .npz, the recorded env's column in the MAT file, a
    reached-rate per ACTION_DELAY value whose episode counts add up to the report's."""
    import scipy.io
    from vine_robot_isaacgymenvs_amd.learning.player import PpoPlayerContinuous
    from vine_robot_isaacgymenvs_amd.train import main
    from vine_robot_isaacgymenvs_amd.utils import episodes
    monkeypatch.chdir(tmp_path)
    common = ["task=Vine5LinkMovingBase", "num_envs=512", "headless=True", "experiment=plants", "task.env.CREATE_PIPE=False",
              "task.env.maxEpisodeLength=%d" % MAX_LEN,
              "task.env.ENV_PARAMS={DAMPING: [0.01, 0.05], ACTION_DELAY: {values: [0, 2]}}", "task.env.EPISODE_LOG=True",
              "task.env.EPISODE_LOG_CAPACITY=32768", "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "train")]
    main(common + ["minibatch_size=2048", "max_iterations=2", "train.params.config.horizon_length=8",
                   "train.params.config.save_frequency=1", "train.params.config.save_best_after=0",
                   "+train.params.config.print_stats=False", "task.env.RECORD_TRAJECTORIES=True",
                   "task.env.RECORD_TRAJECTORIES_EVERY=8", "task.env.RECORD_TRAJECTORIES_STEPS=8",
                   "task.env.RECORD_TRAJECTORIES_DIR=" + str(tmp_path / "train")])
    torch.cuda.synchronize()
    run = tmp_path / "runs" / "plants"
    from vine_robot_isaacgymenvs_amd.utils import tfevents
    (events,) = glob.glob(str(run / "summaries" / "events.out.tfevents.*"))
    scalars = tfevents.read_scalars(events)
    tags = {t for t, _, _, _ in scalars}
    assert {"losses/a_loss", "losses/c_loss", "info/kl", "episodes/episodes", "episodes/reached_ever_rate"} <= tags, sorted(tags)
    assert all(np.isfinite(v) for _, v, _, _ in scalars), [(t, v) for t, v, _, _ in scalars if not np.isfinite(v)]
    (npz,) = glob.glob(str(tmp_path / "train" / "*_episodes.npz"))
    table, names = episodes.load_env_params(npz)
    rows = episodes.load(npz)[0]
    assert table.shape == (abi.VP_COUNT, 512) and tuple(names) == abi.ENV_PARAM_ROW_NAMES and len(rows["env"]) >= 512
    assert set(table[abi.VP_ACTION_DELAY].tolist()) == {0.0, 2.0}
    mats = sorted(glob.glob(str(tmp_path / "train" / "*_trajectory_*_env*.mat")))
    assert mats, "RECORD_TRAJECTORIES wrote nothing"
    mat = scipy.io.loadmat(mats[0])
    e = int(mat["env"][0, 0])
    assert mat["env_params"].shape == (abi.VP_COUNT, 1)
    assert np.array_equal(mat["env_params"][:, 0], table[:, e].astype(np.float64))
    ckpts = sorted(glob.glob(str(run / "nn" / "*.pth")))
    assert ckpts, "no checkpoint written"
    seen = {}
    finish = PpoPlayerContinuous._finish

    def finish_and_keep(self, *a):
        seen["player"] = self
        return finish(self, *a)
    monkeypatch.setattr(PpoPlayerContinuous, "_finish", finish_and_keep)
    capsys.readouterr()
    common[-1] = "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "play")
    reward, steps = main(common + ["test=True", "checkpoint=" + ckpts[-1], "+train.params.config.player={max_steps: 40}"])
    out = capsys.readouterr().out
    player = seen["player"]
    assert np.isfinite(reward) and steps > 0 and player.device_path is False          # eval_step_rows() == 0: the stock path
    assert "reached_ever_rate by param_ACTION_DELAY:" in out and "reached_ever_rate by param_DAMPING:" in out
    delays, rate, count = player.report["by_param"]["param_ACTION_DELAY"]
    assert delays.tolist() == [0.0, 2.0] and np.isfinite(rate).all() and ((0 <= rate) & (rate <= 1)).all()
    assert int(count.sum()) == player.report["episodes"] and count.min() > 0
    edges, drate, dcount = player.report["by_param"]["param_DAMPING"]
    assert len(edges) == len(drate) + 1 and int(dcount.sum()) == player.report["episodes"]
