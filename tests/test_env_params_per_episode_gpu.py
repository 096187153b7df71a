"""ENV_PARAMS_PER_EPISODE on the GPU: the redraw node (include/vine_env_redraw.h) alone against utils/env_params.py
draw_columns, behind every step against the host doing the same between steps, under env_id_offset, in a replayed graph,
and through the task class, the episode log and train.py's entry points.

The shapes are those of tests/test_env_params_gpu.py: 70 envs = two waves, the second partial; 12-step episodes, 40 steps.
"Bit for bit" is literal: float tensors are compared as 32-bit words."""
import ctypes as C
import glob

import numpy as np
import pytest
import torch

from tests.helpers import base_cfg, f6_cfg
from tests.test_env_params_gpu import MAX_LEN, N, T, _make_env, actions_for, assert_bit_equal, saw_resets_and_timeouts
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params

pytestmark = pytest.mark.gpu

# every one of the 28 parameter rows, the three mass names, and the delay over all nine values
SPEC = {"DAMPING": [0.01, 0.05], "SMOOTHING_ALPHA_INFLATE": [0.6, 0.95], "SMOOTHING_ALPHA_DEFLATE": {"values": [0.6, 0.75, 0.9]},
        "RAIL_VELOCITY_SCALE": [0.7, 1.3], "RAIL_P_GAIN": [7.0, 13.0], "RAIL_D_GAIN": [0.0, 0.4], "RAIL_ACCELERATION": [5.6, 10.4],
        "ACTION_DELAY": [0, 8], "FPAM_K": [0.8, 1.2], "FPAM_C": [0.8, 1.2], "FPAM_b": {"values": [0.9, 1.1]}, "FPAM_B": [0.8, 1.2],
        "CART_MASS": [0.35, 0.7], "LINK_MASS": [0.8, 1.3], "TIP_LINK_MASS": {"values": [1.0, 1.5, 2.0]}}
RING = slice(abi.VF_FIFO0, abi.VF_FIFO0 + 2 * abi.MAX_DELAY)
SENTINEL = np.float32(-777.25)


def words(t):
    t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return t.view(np.uint32) if t.dtype == np.float32 else t


@pytest.fixture(scope="module")
def Lane():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    from tests.hip_env import HipEnv as H

    def bind_spec(self, spec, offset=None):
        """Both tables of the spec at episode 0, uploaded and bound; the redraw's spec, value array and episode counters."""
        off = int(self.cfg.env_id_offset)
        self.spec = spec
        self.table_t = torch.as_tensor(env_params.build_table(spec, self.cfg, int(self.cfg.seed), self.n, off, lib=self.lib)).to(self.dev)
        inertia = env_params.build_inertia_table(spec, self.cfg, int(self.cfg.seed), self.n, off, lib=self.lib)
        self.inertia_t = None if inertia is None else torch.as_tensor(inertia).to(self.dev)
        torch.cuda.synchronize(self.dev)
        native.check(self.lib.vine_bind_env_params(self.h, self.table_t.data_ptr()), self.lib)
        if inertia is not None:
            native.check(self.lib.vine_bind_env_inertia(self.h, self.inertia_t.data_ptr()), self.lib)
        _, values = env_params.redraw_names(spec)
        self.values_t = torch.as_tensor(values, dtype=torch.float64).to(self.dev) if len(values) else None
        self.rspec = env_params.redraw_spec(self.lib, self.cfg, spec, self.values_t.data_ptr() if len(values) else None)
        self.episode_t = torch.zeros(self.n, dtype=torch.int32, device=self.dev)
        self.episode_host = np.zeros(self.n, dtype=np.int64)
        torch.cuda.synchronize(self.dev)

    def redraw(self):
        """The node, behind whatever is on the stream."""
        return self.lib.vine_env_redraw_scheduled(
            self.h, self.rspec, self.reset_t.data_ptr(), self.table_t.data_ptr(),
            self.inertia_t.data_ptr() if self.inertia_t is not None else None, self.episode_t.data_ptr(),
            torch.cuda.current_stream(self.dev).cuda_stream)

    def columns(self, envs, episodes):
        return env_params.build_columns(self.spec, self.cfg, np.asarray(envs, np.int64) + int(self.cfg.env_id_offset), episodes,
                                        lib=self.lib)

    def host_redraw(self):
        """What the node does, done from the host: read the flags back, write draw_columns' columns, zero the changed rings."""
        flagged = np.flatnonzero(self.reset_t.cpu().numpy() != 0)
        if not len(flagged):
            return
        self.episode_host[flagged] += 1
        params, inertia = columns(self, flagged, self.episode_host[flagged])
        idx = torch.as_tensor(flagged, device=self.dev)
        changed = flagged[self.table_t[abi.VP_ACTION_DELAY].cpu().numpy()[flagged] != params[abi.VP_ACTION_DELAY]]
        self.table_t[:, idx] = torch.as_tensor(params).to(self.dev)
        self.inertia_t[:, idx] = torch.as_tensor(inertia).to(self.dev)
        if len(changed):
            ring = self.state_t[RING]
            ring[:, torch.as_tensor(changed, device=self.dev)] = 0.0

    return type("HipEnvRedraw", (H,), {"kernel": "lane", "bind_spec": bind_spec, "redraw": redraw, "columns": columns,
                                       "host_redraw": host_redraw})


def plain_cfg(seed=21, offset=0):
    cfg = base_cfg(N, 0, False, max_episode_length=MAX_LEN, seed=seed)
    cfg.env_id_offset = offset
    return cfg


# ------------------------------------------------------------------------------------------------------- the node alone
def test_node_alone_writes_flagged_columns_and_nothing_else(Lane):
    env = Lane(plain_cfg())
    env.bind_spec(SPEC)
    narrow = {"DAMPING": [0.01, 0.05], "ACTION_DELAY": [0, 8], "FPAM_C": {"values": [0.9, 1.1]}}      # rows 0, 7, 13..17 only
    flags = np.zeros(N, dtype=np.int64)
    flags[[0, 1, 5, 62, 63, 64, 65, N - 1]] = 1                   # first, last, and the lanes across the wave boundary
    flags[30:40:3] = 1
    flagged, clear = np.flatnonzero(flags), np.flatnonzero(flags == 0)
    rng = np.random.default_rng(0)
    state0 = rng.uniform(-1.0, 1.0, (abi.VF_COUNT, N)).astype(np.float32)
    state0[RING][state0[RING] == 0.0] = 0.5
    env.state_t.copy_(torch.as_tensor(state0))
    env.reset_t.copy_(torch.as_tensor(flags))
    p0, i0 = env.table_t.cpu().numpy(), env.inertia_t.cpu().numpy()
    for launch in (1, 2):                                         # the second launch on the same flags draws episode 2
        before_p = env.table_t.cpu().numpy()
        assert env.redraw() == abi.OK
        torch.cuda.synchronize()
        p, i, st = env.table_t.cpu().numpy(), env.inertia_t.cpu().numpy(), env.state_t.cpu().numpy()
        want_p, want_i = env.columns(flagged, launch)
        assert np.array_equal(words(p[:, flagged]), words(want_p)), "parameter rows, launch %d" % launch
        assert np.array_equal(words(i[:, flagged]), words(want_i)), "inertia rows (primary and derived), launch %d" % launch
        env_params.check_table(env.lib, env.cfg, p)
        env_params.check_inertia_table(env.lib, env.cfg, i)       # the derived rows are what the host derives, bit for bit
        assert np.array_equal(words(p[:, clear]), words(p0[:, clear])) and np.array_equal(words(i[:, clear]), words(i0[:, clear]))
        episodes = env.episode_t.cpu().numpy()
        assert np.array_equal(episodes, flags * launch)
        moved = before_p[abi.VP_ACTION_DELAY] != p[abi.VP_ACTION_DELAY]
        assert moved[flagged].any() and not moved[clear].any()
        state0[RING][:, moved] = 0.0                              # the ring is zeroed exactly where the delay changed,
        assert np.array_equal(words(st), words(state0)), "the state block, launch %d" % launch      # nothing else is written
    assert not np.array_equal(p[:, flagged], p0[:, flagged])
    env.close()

    # rows the spec does not name are never written: a sentinel survives in them
    env = Lane(plain_cfg())
    env.bind_spec(narrow)
    assert env.inertia_t is None
    named = sorted(r for name in narrow for r in range(abi.ENV_PARAM_ROWS[name][0], sum(abi.ENV_PARAM_ROWS[name])))
    unnamed = [r for r in range(abi.VP_COUNT) if r not in named]
    env.table_t[unnamed] = float(SENTINEL)
    env.reset_t.copy_(torch.as_tensor(flags))
    assert env.redraw() == abi.OK
    torch.cuda.synchronize()
    p = env.table_t.cpu().numpy()
    assert (p[unnamed] == SENTINEL).all()
    want_p, want_i = env.columns(flagged, 1)
    assert want_i is None and np.array_equal(words(p[named][:, flagged]), words(want_p[named]))
    env.close()


def test_refusals_on_a_handle(Lane):
    env = Lane(plain_cfg())
    lib = env.lib
    env.bind_spec(SPEC)
    stream = torch.cuda.current_stream().cuda_stream
    args = [env.h, env.rspec, env.reset_t.data_ptr(), env.table_t.data_ptr(), env.inertia_t.data_ptr(), env.episode_t.data_ptr(), stream]
    for k in (0, 1, 2, 3, 5):
        bad = list(args)
        bad[k] = None
        assert lib.vine_env_redraw_scheduled(*bad) == abi.ERR_INVALID_ARG and b"null argument" in lib.vine_last_error()
    bad = list(args)
    bad[4] = None
    assert lib.vine_env_redraw_scheduled(*bad) == abi.ERR_INVALID_ARG and b"needs an inertia table" in lib.vine_last_error()
    other = env.table_t.clone()
    bad = list(args)
    bad[3] = other.data_ptr()
    assert lib.vine_env_redraw_scheduled(*bad) == abi.ERR_INVALID_ARG and b"not the table bound" in lib.vine_last_error()
    unchecked = abi.VineEnvRedrawSpec.from_buffer_copy(env.rspec)
    unchecked.checked = 0
    bad = list(args)
    bad[1] = unchecked
    assert lib.vine_env_redraw_scheduled(*bad) == abi.ERR_INVALID_ARG and b"not filled by" in lib.vine_last_error()
    native.check(lib.vine_bind_env_inertia(env.h, None), lib)
    assert lib.vine_env_redraw_scheduled(*args) == abi.ERR_INVALID_ARG and b"needs an inertia table" in lib.vine_last_error()
    native.check(lib.vine_bind_env_params(env.h, None), lib)
    assert lib.vine_env_redraw_scheduled(*args) == abi.ERR_INVALID_ARG and b"needs a parameter table" in lib.vine_last_error()
    env.close()


# ---------------------------------------------------------------------------------------- against the host doing it
def equivalence_cfg(case):
    if case == "free":
        return plain_cfg()
    if case == "pipe":
        cfg = f6_cfg(N, 1, 0, "pipe")
        cfg.max_episode_length, cfg.seed = MAX_LEN, 22
        return cfg
    cfg = base_cfg(N, 0, True, max_episode_length=MAX_LEN, seed=23)
    cfg.obs_noise_std, cfg.action_noise_std, cfg.dyn_scale_min, cfg.dyn_scale_max = 0.01, 0.02, 0.9, 1.1
    if case == "offset":
        cfg.env_id_offset = 1000
    return cfg


def run_with(env, actions, after_step):
    rec = {k: [] for k in ("obs", "rew", "reset", "progress", "timeouts", "state", "params", "inertia")}
    for a in actions:
        env.step_t(a.to(env.dev).contiguous(), sync=False)
        after_step()
        for k, t in (("obs", env.obs_t), ("rew", env.rew_t), ("reset", env.reset_t), ("progress", env.progress_t),
                     ("timeouts", env.timeouts_t), ("state", env.state_t), ("params", env.table_t), ("inertia", env.inertia_t)):
            rec[k].append(t.clone())
    torch.cuda.synchronize(env.dev)
    return {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}


@pytest.mark.parametrize("case", ["free", "pipe", "randomize-noise", "offset"])
def test_node_behind_every_step_equals_the_host_rewriting_between_steps(Lane, case):
    """Handle A: the node behind every step.  Handle B: after every step the host reads reset_buf back and writes
    draw_columns' columns and the ring zeroing itself.  State block, obs, rew, reset, progress, timeouts (and both tables)
    after each of the 40 steps, bit for bit.  `offset`: env_id_offset 1000 on both, so the node's global id is checked
    against the host draw of ids 1000..1069."""
    acts = actions_for(N, T)
    a = Lane(equivalence_cfg(case))
    a.bind_spec(SPEC)

    def node():
        assert a.redraw() == abi.OK
    ra = run_with(a, acts, node)
    episodes_a = a.episode_t.cpu().numpy()
    a.close()
    b = Lane(equivalence_cfg(case))
    b.bind_spec(SPEC)
    rb = run_with(b, acts, b.host_redraw)
    assert saw_resets_and_timeouts(rb), case
    assert_bit_equal({k: ra[k] for k in ra if k not in ("params", "inertia")}, {k: rb[k] for k in rb if k not in ("params", "inertia")},
                     what=case)
    assert np.array_equal(words(ra["params"]), words(rb["params"])) and np.array_equal(words(ra["inertia"]), words(rb["inertia"]))
    assert np.array_equal(episodes_a, b.episode_host) and episodes_a.max() >= 2
    if case == "offset":
        p, _ = env_params.build_columns(SPEC, b.cfg, np.arange(1000, 1000 + N), b.episode_host, lib=b.lib)
        assert np.array_equal(words(ra["params"][-1]), words(p))
    b.close()


# ------------------------------------------------------------------------------------------------------------- replay
def test_captured_step_and_node_pairs_replay_like_eager_launches(Lane):
    """Four (step + node) pairs captured once and replayed ten times against the same 40 pairs launched eagerly."""
    acts = actions_for(N, T).cuda()
    eager = Lane(equivalence_cfg("randomize-noise"))
    eager.bind_spec(SPEC)
    for k in range(T):
        eager.step_t(acts[k].contiguous(), sync=False)
        assert eager.redraw() == abi.OK
    torch.cuda.synchronize()
    g_env = Lane(equivalence_cfg("randomize-noise"))
    g_env.bind_spec(SPEC)
    a_in = torch.zeros(4, N, 2, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for k in range(4):
            g_env.step_t(a_in[k], sync=False)
            assert g_env.redraw() == abi.OK
    for r in range(10):
        a_in.copy_(acts[4 * r:4 * r + 4])
        graph.replay()
    torch.cuda.synchronize()
    assert g_env.step_count == eager.step_count == T
    for name in ("state_t", "obs_t", "rew_t", "reset_t", "progress_t", "timeouts_t", "table_t", "inertia_t", "episode_t"):
        assert np.array_equal(words(getattr(g_env, name)), words(getattr(eager, name))), name
    assert int(eager.episode_t.max()) >= 2
    eager.close()
    g_env.close()


# ----------------------------------------------------------------------------------------------------- the task class
def test_task_class_redraws_exactly_the_envs_that_reset(tmp_path):
    """After 40 steps env.env_params differs from the initial table exactly in the envs that reset; every episode-log row's
    param_* equals draw_columns(env, episode); set_env_params raises."""
    from vine_robot_isaacgymenvs_amd.utils import episodes
    extra = ["task.env.ENV_PARAMS_PER_EPISODE=True", "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_DIR=" + str(tmp_path)]
    env = _make_env(N, SPEC, extra)
    try:
        assert env.env_redraw is not None and env.observers[-1] is env.env_redraw
        first_p, first_i = env.env_params.clone(), env.env_inertia.clone()
        want_p = env_params.build_table(SPEC, env._vcfg, int(env._vcfg.seed), N, 0, lib=env._lib)
        assert np.array_equal(words(first_p), words(want_p))
        acts = actions_for(N, T, seed=7).cuda()
        obs = torch.zeros(N, env.num_obs, device="cuda")
        resets = np.zeros(N, dtype=np.int64)
        for k in range(T):
            env.step_into(acts[k], obs)
            resets += env.reset_buf.cpu().numpy()
        did, did_not = np.flatnonzero(resets > 0), np.flatnonzero(resets == 0)
        assert len(did) > 0
        now_p, now_i = env.env_params.cpu().numpy(), env.env_inertia.cpu().numpy()
        assert np.array_equal(words(now_p[:, did_not]), words(first_p.cpu().numpy()[:, did_not]))
        assert np.array_equal(words(now_i[:, did_not]), words(first_i.cpu().numpy()[:, did_not]))
        assert (now_p[abi.VP_DAMPING, did] != first_p.cpu().numpy()[abi.VP_DAMPING, did]).all()
        assert np.array_equal(env.env_redraw.episodes_now(), resets)
        p, i = env.env_redraw.columns(np.arange(N), resets)
        assert np.array_equal(words(now_p), words(p)) and np.array_equal(words(now_i), words(i))
        assert np.array_equal(env.env_params_of(range(N)), now_p.astype(np.float64))
        with pytest.raises(RuntimeError, match="the spec owns the tables"):
            env.set_env_params({"DAMPING": 0.03})
        env.episode_log.harvest()
        rows = env.episode_log.rows_with_params()
        assert len(rows["env"]) == resets.sum() and rows["episode"].max() >= 1
        for e in did:                                             # each env's rows are its episodes 0, 1, ... in end-step order
            assert rows["episode"][rows["env"] == e].tolist() == list(range(resets[e]))
        cp, ci = env.env_redraw.columns(rows["env"], rows["episode"])
        assert np.array_equal(rows["param_DAMPING"], cp[abi.VP_DAMPING]) and np.array_equal(rows["param_FPAM_K"], cp[abi.VP_FPAM_K0])
        assert np.array_equal(rows["param_ACTION_DELAY"], cp[abi.VP_ACTION_DELAY])
        assert np.array_equal(rows["param_CART_MASS"], ci[abi.VI_CART_MASS]) and np.array_equal(rows["param_LINK_MASS"], ci[abi.VI_LINK_MASS0])
        path = env.episode_log.path
    finally:
        env.close()
    episode, columns = episodes.load_env_redraw(path)            # the offline reader rebuilds the same columns, no device
    stored = episodes.load(path)[0]
    assert np.array_equal(episode, rows["episode"])
    op, oi = columns(stored["env"], episode)
    assert np.array_equal(words(op), words(cp)) and np.array_equal(words(oi), words(ci))


def test_train_and_play_entries_per_episode(tmp_path, monkeypatch, capsys):
    """Two training iterations (horizon 8) and test=True through train.py's entry point with the switch on: finite scalars,
    the episode column and the spec in the .npz, env_episode in the recorded env's MAT files, by_param in the player's report."""
    import scipy.io
    from vine_robot_isaacgymenvs_amd.learning.player import PpoPlayerContinuous
    from vine_robot_isaacgymenvs_amd.train import main
    from vine_robot_isaacgymenvs_amd.utils import episodes, tfevents
    monkeypatch.chdir(tmp_path)
    common = ["task=Vine5LinkMovingBase", "num_envs=512", "headless=True", "experiment=plants", "task.env.CREATE_PIPE=False",
              "task.env.maxEpisodeLength=%d" % MAX_LEN, "task.env.ENV_PARAMS_PER_EPISODE=True",
              "task.env.ENV_PARAMS={DAMPING: [0.01, 0.05], ACTION_DELAY: {values: [0, 2]}, LINK_MASS: [0.8, 1.3]}",
              "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_CAPACITY=32768", "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "train")]
    main(common + ["minibatch_size=2048", "max_iterations=2", "train.params.config.horizon_length=8",
                   "train.params.config.save_frequency=1", "train.params.config.save_best_after=0",
                   "+train.params.config.print_stats=False", "task.env.RECORD_TRAJECTORIES=True",
                   "task.env.RECORD_TRAJECTORIES_EVERY=8", "task.env.RECORD_TRAJECTORIES_STEPS=8",
                   "task.env.RECORD_TRAJECTORIES_DIR=" + str(tmp_path / "train")])
    torch.cuda.synchronize()
    run = tmp_path / "runs" / "plants"
    (events,) = glob.glob(str(run / "summaries" / "events.out.tfevents.*"))
    scalars = tfevents.read_scalars(events)
    assert all(np.isfinite(v) for _, v, _, _ in scalars)
    (npz,) = glob.glob(str(tmp_path / "train" / "*_episodes.npz"))
    episode, columns = episodes.load_env_redraw(npz)
    mats = sorted(glob.glob(str(tmp_path / "train" / "*_trajectory_*_env*.mat")))
    assert mats, "RECORD_TRAJECTORIES wrote nothing"
    for m in mats:                                            # a recorded env's plant at harvest is that of its env_episode
        mat = scipy.io.loadmat(m)
        mp, mi = columns([int(mat["env"][0, 0])], [int(mat["env_episode"][0, 0])])
        assert np.array_equal(mat["env_params"][:, 0], mp[:, 0].astype(np.float64))
        assert np.array_equal(mat["env_inertia"][:, 0], mi[:abi.VI_PRIMARY_COUNT, 0].astype(np.float64))
    assert max(int(scipy.io.loadmat(m)["env_episode"][0, 0]) for m in mats) >= 1
    rows = episodes.load(npz)[0]
    assert len(episode) == len(rows["env"]) >= 512 and episode.max() >= 1
    p, i = columns(rows["env"], episode)
    assert set(p[abi.VP_ACTION_DELAY].tolist()) == {0.0, 2.0} and i.shape == (abi.VI_COUNT, len(episode))
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
    assert np.isfinite(reward) and steps > 0
    assert "reached_ever_rate by param_ACTION_DELAY:" in out and "reached_ever_rate by param_DAMPING:" in out
    delays, rate, count = player.report["by_param"]["param_ACTION_DELAY"]
    assert delays.tolist() == [0.0, 2.0] and int(count.sum()) == player.report["episodes"] and count.min() > 0
    assert "param_LINK_MASS" in player.report["by_param"]
