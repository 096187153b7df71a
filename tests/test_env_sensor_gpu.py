"""ENV_SENSOR on the GPU: the launch of include/vine_env_sensor.h alone, behind real steps, under env_id_offset and in a
shard, in a replayed graph, through the task class (every step entry, reset_idx, the episode log) and through train.py's
entries -- each against utils/env_sensor.py sensor_replay.

The shapes are those of tests/test_env_params_gpu.py: 70 envs = two waves, the second partial, in one workgroup that is not
full; 12-step episodes, 40 steps.  "Bit for bit" is literal: float tensors are compared as 32-bit words, noise included."""
import glob

import numpy as np
import pytest
import torch

from tests.helpers import base_cfg, f6_cfg
from tests.test_env_params_gpu import MAX_LEN, N, T, actions_for, assert_bit_equal, saw_resets_and_timeouts
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_sensor

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
PAD = 64                                 # guard elements on both sides of every buffer
SPEC = {"DELAY": [0, 8], "HOLD": {"values": [0.0, 0.3, 0.9]}, "NOISE_STD": {"values": [0.0, 0.01]}, "COLUMNS": list(range(1, 27)),
        "PER_EPISODE": True}
STATE = ("ring", "table", "fresh", "episode_index")


def words(t):
    t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return t.view(np.uint32) if t.dtype == np.float32 else t


def config(num_obs=28, **keys):
    return env_sensor.sensor_config({"ENV_SENSOR": keys}, num_obs)


def guarded(shape, dtype, dev, fill=0):
    """A tensor of ``shape`` in the middle of a larger allocation whose PAD elements on both sides hold a sentinel."""
    numel = int(np.prod(shape))
    sentinel = 0xA5 if dtype == torch.uint8 else -77725 if dtype == torch.int32 else SENTINEL
    whole = torch.full((PAD + numel + PAD,), sentinel, dtype=dtype, device=dev)
    view = whole[PAD:PAD + numel].view(*shape)
    view.fill_(fill)
    return whole, view, sentinel


def hand_table(n):
    """Delays 0..8 all in one wave (env e gets e % 9), holds in {0, 0.3, 0.9}, stds in {0, 0.01}."""
    e = np.arange(n)
    return np.stack([(e % 9).astype(np.float32), np.asarray([0.0, 0.3, 0.9], dtype=np.float32)[(e // 9) % 3],
                     np.asarray([0.0, 0.01], dtype=np.float32)[(e // 3) % 2]])


@pytest.fixture(scope="module")
def Sensed():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    from tests.hip_env import HipEnv as H

    def bind_sensor(self, spec, table=None):
        """The observer's state (guarded) and the checked spec; ``table``: float32 [3, n] instead of episode 0's draw."""
        self.sensor_cfg = spec
        self.gids = np.arange(self.n, dtype=np.int64) + int(self.cfg.env_id_offset)
        _, values = env_sensor.sensor_names(spec)
        self.values_t = torch.as_tensor(values, dtype=torch.float64).to(self.dev) if len(values) else None
        self.sspec = env_sensor.sensor_spec(self.lib, self.cfg, spec, self.values_t.data_ptr() if len(values) else None)
        self.guards = {}
        for name, shape, dtype, fill in (("ring", (abi.SENSOR_SLOTS, self.n, self.num_obs), torch.float32, 0),
                                         ("table", (3, self.n), torch.float32, 0), ("fresh", (self.n,), torch.uint8, 1),
                                         ("episode_index", (self.n,), torch.int32, 0), ("sobs", (self.n, self.num_obs), torch.float32, 0)):
            whole, view, sentinel = guarded(shape, dtype, self.dev, fill)
            self.guards[name] = (whole, sentinel)
            setattr(self, name, view)
        first = env_sensor.draw_sensor(spec, int(self.cfg.seed), self.gids, 0).astype(np.float32) if table is None else table
        self.table.copy_(torch.as_tensor(np.ascontiguousarray(first)))
        self.table0 = np.ascontiguousarray(first)
        torch.cuda.synchronize(self.dev)

    def sensor(self, obs=None):
        """The launch, behind whatever is on the stream, on ``obs`` (default: the step's own buffer)."""
        obs = self.obs_t if obs is None else obs
        return self.lib.vine_env_sensor_scheduled(
            self.h, self.sspec, obs.data_ptr(), self.reset_t.data_ptr(), self.progress_t.data_ptr(), self.table.data_ptr(),
            self.ring.data_ptr(), self.fresh.data_ptr(), self.episode_index.data_ptr(), torch.cuda.current_stream(self.dev).cuda_stream)

    def guards_intact(self):
        for name, (whole, sentinel) in self.guards.items():
            w = whole.cpu().numpy()
            assert (w[:PAD] == sentinel).all() and (w[-PAD:] == sentinel).all(), name
        return True

    def replay(self, steps, raw, progress, resets, external=None, table=None):
        return env_sensor.sensor_replay(self.sensor_cfg, int(self.cfg.seed), self.gids, steps, raw, progress, resets, external,
                                        float(self.cfg.clip_observations), table=self.table0 if table is None else table)

    def state_equals(self, want, what=""):
        for name in STATE:
            assert np.array_equal(words(getattr(self, name)), words(want[name].astype(getattr(self, name).cpu().numpy().dtype))), (what, name)
        return True

    return type("HipEnvSensed", (H,), {"kernel": "lane", "bind_sensor": bind_sensor, "sensor": sensor, "guards_intact": guards_intact, "replay": replay,
                                       "state_equals": state_equals})


def case_cfg(case, n=N, offset=0):
    if case == "pipe":
        cfg = f6_cfg(n, 1, 0, "pipe")
        cfg.max_episode_length, cfg.seed = MAX_LEN, 22
    elif case == "free":
        cfg = base_cfg(n, 0, False, max_episode_length=MAX_LEN, seed=21)
    elif case == "tipobs":                                   # 18 columns: rows move as 8-byte vectors
        cfg = base_cfg(n, abi.OBS_TYPE_BY_NAME["TIP_AND_CART_AND_OBJ_INFO"], False, max_episode_length=MAX_LEN, seed=24)
    else:                                                    # vine_randomize with the reference's own Gaussian noise on
        cfg = base_cfg(n, 0, True, max_episode_length=MAX_LEN, seed=23)
        cfg.obs_noise_std, cfg.action_noise_std, cfg.dyn_scale_min, cfg.dyn_scale_max = 0.01, 0.02, 0.9, 1.1
    cfg.env_id_offset = offset
    return cfg


def pattern(t, n, num_obs):
    e, j = np.meshgrid(np.arange(n), np.arange(num_obs), indexing="ij")
    return ((t + 1) / 64.0 + e / 4096.0 + j / 262144.0).astype(np.float32)


def hand_flags(steps, n):
    """progress and reset by hand: env e runs episodes of 5 + e % 7 steps; the step before a progress of 0 raised its flag."""
    t, e = np.meshgrid(np.arange(steps + 1), np.arange(n), indexing="ij")
    progress = (t + e) % (5 + e % 7)
    return progress[:steps].astype(np.int64), (progress[1:] == 0).astype(np.int64)


# ------------------------------------------------------------------------------------------------------ the launch alone
@pytest.mark.parametrize("case", ["free", "tipobs"])
def test_launch_alone_equals_the_replay_after_every_launch(Sensed, case):
    """48 launches on a pattern of (step, env, column), progress and reset set by hand, the step count set to the index the
    launch rides behind; delays 0..8 in one wave, the mask without the first and the last column: delivered buffer and all
    observer state against the replay after every launch, the guards around every buffer untouched."""
    env = Sensed(case_cfg(case))
    assert env.num_obs == (28 if case == "free" else 18)
    spec = config(env.num_obs, DELAY=[0, 8], HOLD=[0.0, 0.9], NOISE_STD=[0.0, 0.01], COLUMNS=list(range(1, env.num_obs - 1)))
    table = hand_table(N)
    assert sorted(set(table[0, :64].tolist())) == list(range(9))
    env.bind_sensor(spec, table)
    steps = 48
    progress, resets = hand_flags(steps, N)
    raw = np.stack([pattern(t, N, env.num_obs) for t in range(steps)])
    index = np.arange(steps) + 3
    want = env.replay(index, raw, progress, resets)
    held = 0
    for t in range(steps):
        env.step_count = int(index[t]) + 1                       # the launch rides behind the step with this index
        env.sobs.copy_(torch.as_tensor(raw[t]))
        env.set_flags(resets[t], progress[t])
        assert env.sensor(env.sobs) == abi.OK
        torch.cuda.synchronize()
        assert np.array_equal(words(env.sobs), words(want[t]["obs"])), "delivered, launch %d" % t
        assert env.state_equals(want[t], "launch %d" % t) and env.guards_intact()
        held += int(want[t]["held"].sum())
    assert held > 100 and not np.array_equal(words(want[-1]["obs"]), words(raw[-1]))
    assert np.array_equal(words(env.sobs[:, [0, env.num_obs - 1]]), words(raw[-1][:, [0, env.num_obs - 1]]))
    assert np.array_equal(words(env.table), words(table)) and int(env.episode_index.abs().max()) == 0      # held: never rewritten
    env.close()


def test_all_zero_settings_leave_every_bit(Sensed):
    env = Sensed(case_cfg("free"))
    env.bind_sensor(config(DELAY=0, PER_EPISODE=True))
    assert float(env.table.abs().max()) == 0.0
    progress, resets = hand_flags(12, N)
    rng = np.random.default_rng(5)
    for t in range(12):
        raw = rng.standard_normal((N, 28)).astype(np.float32)
        raw[t % N, 3], raw[(t + 1) % N, 27] = np.float32(-0.0), np.float32(1e-42)      # a signed zero, a denormal
        env.step_count = t + 1
        env.sobs.copy_(torch.as_tensor(raw))
        env.set_flags(resets[t], progress[t])
        assert env.sensor(env.sobs) == abi.OK
        torch.cuda.synchronize()
        assert np.array_equal(words(env.sobs), words(raw)) and env.guards_intact()
        assert np.array_equal(words(env.ring[t % 9]), words(raw))                        # ... and the frame was still pushed
    assert float(env.table.abs().max()) == 0.0 and np.array_equal(env.episode_index.cpu().numpy(), resets.sum(axis=0))
    env.close()


def test_per_episode_rewrites_flagged_envs_only(Sensed):
    env = Sensed(case_cfg("free", offset=1000))
    env.bind_sensor(config(**SPEC))
    steps = 30
    progress, resets = hand_flags(steps, N)
    quiet = [5, 63, 64, N - 1]                                   # never flagged: their (hand-made) entries must survive
    resets[:, quiet] = 0
    table = env.table0.copy()
    table[:, quiet] = np.asarray([[3.0], [0.125], [0.0456]], dtype=np.float32)
    env.table.copy_(torch.as_tensor(table))
    raw = np.stack([pattern(t, N, 28) for t in range(steps)])
    want = env.replay(np.arange(steps), raw, progress, resets, table=table)
    for t in range(steps):
        env.step_count = t + 1
        env.sobs.copy_(torch.as_tensor(raw[t]))
        env.set_flags(resets[t], progress[t])
        assert env.sensor(env.sobs) == abi.OK
        torch.cuda.synchronize()
        assert env.state_equals(want[t], "launch %d" % t) and np.array_equal(words(env.sobs), words(want[t]["obs"]))
        assert np.array_equal(words(env.table[:, quiet]), words(table[:, quiet])) and env.guards_intact()
    episodes = env.episode_index.cpu().numpy()
    assert np.array_equal(episodes, resets.sum(axis=0)) and episodes.max() >= 3 and (episodes[quiet] == 0).all()
    assert np.array_equal(words(env.table), words(np.where(episodes > 0, env_sensor.draw_sensor(env.sensor_cfg, int(env.cfg.seed),
                                                                                               env.gids, episodes).astype(np.float32), table)))
    env.close()


def test_refusals_on_a_handle(Sensed):
    env = Sensed(case_cfg("free"))
    env.bind_sensor(config(**SPEC))
    lib, stream = env.lib, torch.cuda.current_stream().cuda_stream
    args = [env.h, env.sspec, env.sobs.data_ptr(), env.reset_t.data_ptr(), env.progress_t.data_ptr(), env.table.data_ptr(),
            env.ring.data_ptr(), env.fresh.data_ptr(), env.episode_index.data_ptr(), stream]
    for k in range(9):
        bad = list(args)
        bad[k] = None
        assert lib.vine_env_sensor_scheduled(*bad) == abi.ERR_INVALID_ARG and b"null argument" in lib.vine_last_error()
    unchecked = abi.VineEnvSensorSpec.from_buffer_copy(env.sspec)
    unchecked.checked = 0
    bad = list(args)
    bad[1] = unchecked
    assert lib.vine_env_sensor_scheduled(*bad) == abi.ERR_INVALID_ARG and b"not filled by" in lib.vine_last_error()
    bad = list(args)
    bad[2] = env.sobs.data_ptr() + 4
    assert lib.vine_env_sensor_scheduled(*bad) == abi.ERR_INVALID_ARG and b"aligned" in lib.vine_last_error()
    assert env.guards_intact()
    env.close()


# -------------------------------------------------------------------------------------------------- behind real steps
def run_pair(Sensed, case, offset=0, n=N, acts=None):
    """Handle A with the launch behind every step, handle B without it, the same actions: per step everything both wrote."""
    acts = actions_for(N, T) if acts is None else acts
    a, b = Sensed(case_cfg(case, n, offset)), Sensed(case_cfg(case, n, offset))
    a.bind_sensor(config(**SPEC))
    keys = ("obs", "rew", "reset", "progress", "timeouts", "state")
    ra, rb = {k: [] for k in keys}, {k: [] for k in keys}
    for act in acts:
        for env, rec in ((a, ra), (b, rb)):
            env.step_t(act.to(env.dev).contiguous(), sync=False)
            if env is a:
                assert a.sensor() == abi.OK
            for k, t in zip(keys, (env.obs_t, env.rew_t, env.reset_t, env.progress_t, env.timeouts_t, env.state_t)):
                rec[k].append(t.clone())
    torch.cuda.synchronize()
    ra, rb = ({k: torch.stack(v).cpu().numpy() for k, v in r.items()} for r in (ra, rb))
    return a, b, ra, rb


@pytest.mark.parametrize("case,offset", [("free", 0), ("pipe", 0), ("randomize-noise", 0), ("randomize-noise", 1000)])
def test_behind_real_steps_only_the_observation_changes_and_it_is_the_replays(Sensed, case, offset):
    a, b, ra, rb = run_pair(Sensed, case, offset)
    assert saw_resets_and_timeouts(rb), case
    rest = [k for k in ra if k != "obs"]
    assert_bit_equal({k: ra[k] for k in rest}, {k: rb[k] for k in rest}, what=case)      # state, rewards, flags, progress
    want = a.replay(np.arange(T), rb["obs"], rb["progress"], rb["reset"])
    for t in range(T):
        assert np.array_equal(words(ra["obs"][t]), words(want[t]["obs"])), (case, t)
    assert a.state_equals(want[-1], case) and a.guards_intact()
    assert want[-1]["episode_index"].max() >= 2 and not np.array_equal(words(ra["obs"]), words(rb["obs"]))
    assert np.array_equal(words(ra["obs"][:, :, [0, 27]]), words(rb["obs"][:, :, [0, 27]]))
    for t in range(1, T):                                            # no frame of an earlier episode in a later one
        first = rb["progress"][t] == 0
        quiet = want[t - 1]["table"][2] == 0                             # (the values in force while step t was sensed)
        assert np.array_equal(words(ra["obs"][t][first & quiet]), words(rb["obs"][t][first & quiet]))
    a.close()
    b.close()
    if case == "free":                                               # a 35-env shard at offset 35 is the whole batch's upper half
        acts = actions_for(N, T)
        s, sb, rs, _ = run_pair(Sensed, case, 35, 35, acts[:, 35:])
        assert np.array_equal(words(rs["obs"]), words(ra["obs"][:, 35:])) and np.array_equal(words(rs["state"]), words(ra["state"][:, :, 35:]))
        assert np.array_equal(words(s.table), words(want[-1]["table"][:, 35:]))
        assert np.array_equal(s.episode_index.cpu().numpy(), want[-1]["episode_index"][35:])
        s.close()
        sb.close()


def test_captured_groups_of_four_steps_replay_like_eager_launches(Sensed):
    """Four (step + launch) pairs captured once, each writing its own observation slot, replayed ten times, against the same
    forty pairs launched eagerly into the same four slots."""
    acts = actions_for(N, T).cuda()
    envs = []
    for graphed in (False, True):
        env = Sensed(case_cfg("randomize-noise"))
        env.bind_sensor(config(**SPEC))
        env.slots = torch.zeros(4, N, 28, device="cuda")
        a_in = torch.zeros(4, N, 2, device="cuda")
        torch.cuda.synchronize()

        def group():
            for k in range(4):
                native.check(env.lib.vine_step(env.h, a_in[k].data_ptr(), env.slots[k].data_ptr(), env.rew_t.data_ptr(),
                                               env.reset_t.data_ptr(), env.progress_t.data_ptr(), env.timeouts_t.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), env.lib)
                assert env.sensor(env.slots[k]) == abi.OK
        if graphed:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                group()
        for r in range(10):
            a_in.copy_(acts[4 * r:4 * r + 4])
            graph.replay() if graphed else group()
        torch.cuda.synchronize()
        envs.append(env)
    eager, g_env = envs
    assert g_env.step_count == eager.step_count == T
    for name in ("slots", "state_t", "rew_t", "reset_t", "progress_t", "timeouts_t") + STATE:
        assert np.array_equal(words(getattr(g_env, name)), words(getattr(eager, name))), name
    assert int(eager.episode_index.max()) >= 2 and eager.guards_intact() and g_env.guards_intact()
    eager.close()
    g_env.close()


# ----------------------------------------------------------------------------------------------------- the task class
class Tap:
    """A step observer in front of the sensor that keeps a copy of what the step wrote, and of its flags."""
    wants_obs = True
    paused, copy_done = 0, None

    def __init__(self, env):
        self.env, self.known, self.raw, self.progress, self.reset, self.steps = env, list(env._obs_ring), [], [], [], []

    def enqueue(self, stream, actions=None, obs=None):
        (tensor,) = [t for t in self.known if t.data_ptr() == obs]
        self.raw.append(tensor.clone())
        self.progress.append(self.env.progress_buf.clone())
        self.reset.append(self.env.reset_buf.clone())

    def before(self, n):
        pass

    advance = set_steps = before

    def live_tensors(self):
        return []

    def drain(self):
        pass

    close = drain

    def arrays(self):
        return tuple(torch.stack(v).cpu().numpy() for v in (self.raw, self.progress, self.reset))


def make_task(n, extra, env_params=None, seed=42):
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_config(overrides=["num_envs=%d" % n, "task.env.CREATE_PIPE=False", "task.env.maxEpisodeLength=%d" % MAX_LEN] + list(extra))
    cfg["task"]["seed"] = seed
    cfg["task"]["env"]["ENV_SENSOR"] = dict(SPEC)
    if env_params:
        cfg["task"]["env"]["ENV_PARAMS"] = env_params
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                  headless=True)
    tap = Tap(env)
    env._observers.insert(env._observers.index(env.env_sensor), tap)
    return env, tap


def task_replay(env, tap, first_step=0, external=None):
    raw, progress, resets = tap.arrays()
    s = env.env_sensor
    return env_sensor.sensor_replay(s.spec, s.seed, np.arange(env.num_envs) + s.env_id_offset, first_step + np.arange(len(raw)), raw,
                                    progress, resets, external, float(env._vcfg.clip_observations))


def test_every_step_entry_of_the_task_class_delivers_the_replays_observation(tmp_path):
    """step, step_into, the fused rollout step and the evaluation step, ten of each in one run on the four-lane kernel, with a
    reset_idx from outside in the middle; every delivered observation, the observer's final state and every episode-log row's
    param_SENSOR_* against the replay of what a tap in front of the sensor saw."""
    from tests.test_eval_step import H, _eval_args, _eval_state, _head
    n = 256
    env, tap = make_task(n, ["task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_DIR=" + str(tmp_path)])
    try:
        lib, dev, st = env._lib, torch.device("cuda:0"), torch.cuda.current_stream().cuda_stream
        assert env.step_kernel_name == "vine_step_quad_kernel" and env.rollout_step_blocks() > 0 and env.eval_step_rows() > 0
        assert env.observers[-1] is env.env_sensor and env.episode_log.sensor is env.env_sensor
        p, rnd = _head(dev, lib, st)
        acts = actions_for(n, 20, seed=11).cuda()
        delivered, external = [], []
        out = torch.zeros(10, n, env.num_obs, device=dev)
        tap.known += list(out)
        for k in range(10):
            obs, _, _, _ = env.step(acts[k])
            delivered.append(obs["obs"].clone())
            external.append([])
        for k in range(10):
            external.append([])
            if k == 4:                                           # from outside, between two steps
                env.reset_idx(torch.tensor([3, 64, n - 1], device=dev))
                external[-1] = [3, 64, n - 1]
            delivered.append(env.step_into(acts[10 + k], out[k]).clone())
        sb = dict(mu=torch.empty(n, 2, device=dev), sigma=torch.empty(n, 2, device=dev), value=torch.empty(n, 1, device=dev),
                  action=torch.empty(n, 2, device=dev), nlp=torch.empty(n, device=dev), shaped=torch.empty(n, 1, device=dev),
                  dones=torch.empty(n, device=dev, dtype=torch.uint8), cur_r=torch.zeros(n, 1, device=dev), cur_l=torch.zeros(n, device=dev),
                  h=torch.ones(1, n, H, device=dev), c=torch.ones(1, n, H, device=dev), hop=torch.ones(n, 352, device=dev),
                  scratch=torch.zeros(abi.ROLLOUT_POST_SCRATCH_FLOATS, device=dev))
        for k in range(10):
            y = rnd(n, H)
            ra = abi.RolloutArgs()
            ra.y, ra.hw, ra.hc, ra.logstd = y.data_ptr(), p["hw"].data_ptr(), p["hc"].data_ptr(), p["logstd"].data_ptr()
            ra.value_mean, ra.value_var, ra.ln_eps, ra.value_eps = p["vmean"].data_ptr(), p["vvar"].data_ptr(), 1e-5, 1e-5
            ra.seed, ra.counter = 12345, p["counter"].data_ptr()
            ra.mu_out, ra.sigma_out, ra.value_out = sb["mu"].data_ptr(), sb["sigma"].data_ptr(), sb["value"].data_ptr()
            ra.action_out, ra.neglogp_out = sb["action"].data_ptr(), sb["nlp"].data_ptr()
            ra.reward_shift, ra.reward_scale, ra.gamma_bootstrap = 0.0, 0.01, 0.99
            ra.shaped_out, ra.dones_out = sb["shaped"].data_ptr(), sb["dones"].data_ptr()
            ra.cur_rewards, ra.cur_lengths = sb["cur_r"].data_ptr(), sb["cur_l"].data_ptr()
            ra.h_state, ra.c_state, ra.h_op, ra.h_op_stride = sb["h"].data_ptr(), sb["c"].data_ptr(), sb["hop"].data_ptr() + 4 * 96, 352
            ra.partial = sb["scratch"].data_ptr()
            delivered.append(env.step_rollout_into(ra, out[k]).clone())
            external.append([])
            torch.cuda.synchronize()
            p["counter"] += 1
        se = _eval_state(env, n, dev)
        for k in range(10):
            y = rnd(n, H)
            delivered.append(env.step_eval_into(_eval_args(se, p, y, 1), out[k]).clone())
            external.append([])
            torch.cuda.synchronize()
        want = task_replay(env, tap, external=external)
        assert len(want) == 40 == int(env.step_count)
        for t in range(40):
            assert np.array_equal(words(delivered[t]), words(want[t]["obs"])), "step %d" % t
        assert want[14]["first"][[3, 64, n - 1]].all() and not want[14]["first"].all()      # the frame behind reset_idx is fresh
        s = env.env_sensor
        for name in STATE:
            assert np.array_equal(words(getattr(s, name)), words(want[-1][name].astype(getattr(s, name).cpu().numpy().dtype))), name
        assert np.array_equal(s.episodes_now(), want[-1]["episode_index"]) and s.episodes_now().max() >= 2
        assert [t.data_ptr() for t in env.live_tensors()[-4:]] == [t.data_ptr() for t in (s.ring, s.table, s.fresh, s.episode_index)]
        env.episode_log.harvest()
        rows = env.episode_log.rows_with_params()
        assert len(rows["env"]) > n and rows["episode"].max() >= 1
        expect = env_sensor.draw_sensor(s.spec, s.seed, rows["env"], rows["episode"]).astype(np.float32)
        for slot, name in enumerate(env_sensor.DRAW_NAMES):
            assert np.array_equal(words(rows["param_" + name]), words(expect[slot])), name
        # ... which is what the replay's table held while the step that ended the row's episode was sensed
        first = env_sensor.draw_sensor(s.spec, s.seed, np.arange(n), 0).astype(np.float32)
        tables = np.stack([first] + [w["table"] for w in want[:-1]])
        for slot, name in enumerate(env_sensor.DRAW_NAMES):
            assert np.array_equal(words(rows["param_" + name]), words(tables[rows["end_step"], slot, rows["env"]])), name
        path = env.episode_log.path
    finally:
        env.close()
    from vine_robot_isaacgymenvs_amd.utils import episodes
    back = episodes.load_rows_with_params(path)
    for name in env_sensor.DRAW_NAMES:
        assert np.array_equal(words(back["param_" + name]), words(rows["param_" + name]))


def test_with_the_redraw_on_the_two_ordinals_are_equal(tmp_path):
    plants = {"DAMPING": [0.01, 0.05], "ACTION_DELAY": [0, 3]}
    env, tap = make_task(N, ["task.env.ENV_PARAMS_PER_EPISODE=True", "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_DIR=" + str(tmp_path)],
                         plants)
    try:
        assert env.observers[-1] is env.env_redraw and env.observers[-2] is env.env_sensor and env.step_kernel_name == "vine_step_kernel"
        acts = actions_for(N, T, seed=7).cuda()
        obs = torch.zeros(N, env.num_obs, device="cuda")
        tap.known.append(obs)
        delivered = []
        for k in range(T):
            delivered.append(env.step_into(acts[k], obs).clone())
        want = task_replay(env, tap)
        for t in range(T):
            assert np.array_equal(words(delivered[t]), words(want[t]["obs"])), t
        ordinals = env.env_redraw.episodes_now()
        assert np.array_equal(env.env_sensor.episodes_now(), ordinals) and ordinals.max() >= 2
        env.episode_log.harvest()
        rows = env.episode_log.rows_with_params()
        s = env.env_sensor
        expect = env_sensor.draw_sensor(s.spec, s.seed, rows["env"], rows["episode"]).astype(np.float32)
        assert np.array_equal(words(rows["param_SENSOR_DELAY"]), words(expect[0])) and "param_DAMPING" in rows and "param_ACTION_DELAY" in rows
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------ train.py's entry
def test_train_and_play_entries_with_the_sensor_on(tmp_path, monkeypatch, capsys):
    """Two training iterations (horizon 8) with the sensor on: finite scalars, the fused rollout (3 launches per step) and the
    four-lane kernel in force.  Then test=True with DELAY {values: [0, 2, 4]} and the episode log: the printed report has a
    param_SENSOR_DELAY block with three values."""
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    from vine_robot_isaacgymenvs_amd.learning.player import PpoPlayerContinuous
    from vine_robot_isaacgymenvs_amd.train import main
    from vine_robot_isaacgymenvs_amd.utils import tfevents
    monkeypatch.chdir(tmp_path)
    common = ["task=Vine5LinkMovingBase", "num_envs=512", "headless=True", "experiment=sensed", "task.env.CREATE_PIPE=False",
              "task.env.maxEpisodeLength=%d" % MAX_LEN, "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_CAPACITY=32768"]
    seen = {}
    play = A2CAgent.play_steps_rnn

    def play_and_keep(self):
        out = play(self)
        env = getattr(self.vec_env, "env", self.vec_env)
        seen.update(launches=self.rollout_step_launches, kernel=env.step_kernel_name, sensor=env.env_sensor.spec)
        return out
    monkeypatch.setattr(A2CAgent, "play_steps_rnn", play_and_keep)
    main(common + ["minibatch_size=2048", "max_iterations=2", "train.params.config.horizon_length=8",
                   "train.params.config.save_frequency=1", "train.params.config.save_best_after=0", "+train.params.config.print_stats=False",
                   "task.env.ENV_SENSOR={DELAY: [0, 3], HOLD: 0.1, NOISE_STD: 0.01, PER_EPISODE: True}",
                   "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "train")])
    torch.cuda.synchronize()
    monkeypatch.setattr(A2CAgent, "play_steps_rnn", play)
    assert seen["launches"] == 3 and seen["kernel"] == "vine_step_quad_kernel" and seen["sensor"]["PER_EPISODE"] is True
    run = tmp_path / "runs" / "sensed"
    (events,) = glob.glob(str(run / "summaries" / "events.out.tfevents.*"))
    assert all(np.isfinite(v) for _, v, _, _ in tfevents.read_scalars(events))
    ckpts = sorted(glob.glob(str(run / "nn" / "*.pth")))
    assert ckpts, "no checkpoint written"
    kept = {}
    finish = PpoPlayerContinuous._finish

    def finish_and_keep(self, *a):
        kept["player"] = self
        return finish(self, *a)
    monkeypatch.setattr(PpoPlayerContinuous, "_finish", finish_and_keep)
    capsys.readouterr()
    reward, steps = main(common + ["test=True", "checkpoint=" + ckpts[-1], "+train.params.config.player={max_steps: 40}",
                                   "task.env.ENV_SENSOR={DELAY: {values: [0, 2, 4]}}", "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "play")])
    out = capsys.readouterr().out
    assert np.isfinite(reward) and steps > 0
    assert "reached_ever_rate by param_SENSOR_DELAY:" in out
    delays, rate, count = kept["player"].report["by_param"]["param_SENSOR_DELAY"]
    assert delays.tolist() == [0.0, 2.0, 4.0] and int(count.sum()) == kept["player"].report["episodes"] and count.min() > 0
