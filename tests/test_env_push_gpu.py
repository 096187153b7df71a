"""ENV_PUSH on the GPU: the launch of include/vine_env_push.h alone (with and without a bound inertia table), behind real
steps, under env_id_offset and in a shard, in a replayed graph, through the task class (every step entry, with the sensor and
the per-episode redraw on, the episode log) and through train.py's entries -- each against utils/env_push.py push_replay.

The shapes are those of tests/test_env_params_gpu.py: 70 envs = two waves, the second partial, in one workgroup that is not
full; 12-step episodes, 40 steps.  Who is pushed, the impulse, the point, counts, table, ordinals, every field of the state
block but the six velocities and the velocities of every env not pushed are compared bit for bit.  The velocities of pushed
envs are compared with the metric of `velocity_error`: against the float64 replay, at most 4 times the worst the float32
restatement of the kernel's arithmetic shows on the same inputs."""
import ctypes as C
import glob

import numpy as np
import pytest
import torch

from tests.env_inertia_sets import table_of
from tests.test_env_params_gpu import MAX_LEN, N, T, actions_for, assert_bit_equal, own_table, saw_resets_and_timeouts
from tests.test_env_sensor_gpu import PAD, case_cfg, guarded, hand_flags, words
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params, env_push

pytestmark = pytest.mark.gpu

ND = 6
QD = slice(abi.VF_QD0, abi.VF_QD0 + ND)
REST = [f for f in range(abi.VF_COUNT) if not abi.VF_QD0 <= f < abi.VF_QD0 + ND]
SPEC = {"RATE": {"values": [0.0, 0.3, 1.0]}, "IMPULSE": {"values": [0.0, 0.002, 0.01]}, "POINTS": [0, 2, 5], "PER_EPISODE": True}
STATE = ("table", "episode_index", "push_count")
FACTOR = 4.0                                 # the float32 restatement is the yardstick; the factor covers the device's sincosf


def config(**keys):
    return env_push.push_config({"ENV_PUSH": keys})


def hand_state(t, n, seed=1):
    """A state block [VF_COUNT, n]: joints within +-10 degrees, the cart within +-0.3, velocities within +-3 (among them a
    signed zero and a denormal); every other field a recognisable pattern."""
    rng = np.random.default_rng(seed * 1000 + t)
    f, e = np.meshgrid(np.arange(abi.VF_COUNT), np.arange(n), indexing="ij")
    st = ((f + 1) / 8.0 + t / 1024.0 + e / 65536.0).astype(np.float32)
    st[abi.VF_Q0] = rng.uniform(-0.3, 0.3, n)
    st[abi.VF_Q0 + 1:abi.VF_Q0 + ND] = rng.uniform(-np.radians(10), np.radians(10), (ND - 1, n))
    st[QD] = rng.uniform(-3, 3, (ND, n))
    st[abi.VF_QD0 + 2, t % n], st[abi.VF_QD0 + 4, (t + 1) % n] = np.float32(-0.0), np.float32(1e-42)
    return st


def velocity_error(after, before, rep64, envs):
    """max over ``envs`` of max_k |qd_after - (qd_before + dqd64)_k| / max_k |dqd64_k|; 0 for no env."""
    if not len(envs):
        return 0.0
    want = before[QD].T[envs].astype(np.float64) + rep64["dqd"][envs]
    assert np.isfinite(after[QD].T[envs]).all() and np.isfinite(want).all()
    return float((np.abs(after[QD].T[envs].astype(np.float64) - want).max(axis=1) / np.abs(rep64["dqd"][envs]).max(axis=1)).max())


@pytest.fixture(scope="module")
def Pushed():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    from tests.hip_env import HipEnv as H

    def init(self, cfg, device_id=0):
        """HipEnv's set-up with the state block between sentinels."""
        self.lib = native.load()
        cfg = type(cfg).from_buffer_copy(cfg)
        cfg.set_flag(abi.FLAG_INTROSPECT, True)
        self.cfg, self.n, self.dev = cfg, cfg.num_envs, torch.device("cuda", device_id)
        self.num_obs = self.lib.vine_num_obs(C.byref(cfg))
        self.guards = {}
        whole, self.state_t, sentinel = guarded((abi.VF_COUNT, self.n), torch.float32, self.dev)
        self.guards["state"] = (whole, sentinel)
        h = C.c_void_p()
        native.check(self.lib.vine_create(C.byref(cfg), device_id, self.state_t.data_ptr(), C.byref(h)), self.lib)
        self.h = h
        self.obs_t = torch.zeros((self.n, self.num_obs), device=self.dev)
        self.rew_t = torch.zeros(self.n, device=self.dev)
        self.reset_t = torch.ones(self.n, device=self.dev, dtype=torch.long)
        self.progress_t = torch.zeros(self.n, device=self.dev, dtype=torch.long)
        self.timeouts_t = torch.zeros(self.n, device=self.dev, dtype=torch.bool)
        self.reward_matrix_t, self._rv, self.inertia = None, None, None

    def bind_tables(self, inertia):
        """The configuration's own parameter table and a heterogeneous inertia table (the step then takes the one-lane kernel)."""
        env_params.check_table(self.lib, self.cfg, own_table(self))
        env_params.check_inertia_table(self.lib, self.cfg, inertia)
        self.params_t = torch.as_tensor(np.ascontiguousarray(own_table(self), np.float32)).to(self.dev).contiguous()
        self.inertia_t = torch.as_tensor(np.ascontiguousarray(inertia, np.float32)).to(self.dev).contiguous()
        torch.cuda.synchronize(self.dev)
        native.check(self.lib.vine_bind_env_params(self.h, self.params_t.data_ptr()), self.lib)
        native.check(self.lib.vine_bind_env_inertia(self.h, self.inertia_t.data_ptr()), self.lib)
        self.inertia = np.ascontiguousarray(inertia, np.float32)

    def bind_push(self, spec, table=None):
        """The observer's state (guarded) and the checked spec; ``table``: float32 [2, n] instead of episode 0's draw."""
        self.push_cfg = spec
        self.gids = np.arange(self.n, dtype=np.int64) + int(self.cfg.env_id_offset)
        self.geometry = env_push.geometry_of(self.lib, self.cfg)
        _, values = env_push.push_names(spec)
        self.values_t = torch.as_tensor(values, dtype=torch.float64).to(self.dev) if len(values) else None
        self.pspec = env_push.push_spec(self.lib, self.cfg, spec, self.values_t.data_ptr() if len(values) else None)
        for name, shape, dtype in (("table", (2, self.n), torch.float32), ("episode_index", (self.n,), torch.int32),
                                   ("push_count", (self.n,), torch.int32)):
            whole, view, sentinel = guarded(shape, dtype, self.dev)
            self.guards[name] = (whole, sentinel)
            setattr(self, name, view)
        first = env_push.draw_push(spec, int(self.cfg.seed), self.gids, 0).astype(np.float32) if table is None else table
        self.table.copy_(torch.as_tensor(np.ascontiguousarray(first)))
        self.table0 = np.ascontiguousarray(first)
        torch.cuda.synchronize(self.dev)

    def push(self):
        """The launch, behind whatever is on the stream."""
        return self.lib.vine_env_push_scheduled(self.h, self.pspec, self.reset_t.data_ptr(), self.table.data_ptr(),
                                                self.episode_index.data_ptr(), self.push_count.data_ptr(),
                                                torch.cuda.current_stream(self.dev).cuda_stream)

    def guards_intact(self):
        for name, (whole, sentinel) in self.guards.items():
            w = whole.cpu().numpy()
            assert (w[:PAD] == sentinel).all() and (w[-PAD:] == sentinel).all(), name
        return True

    def replay(self, states, resets, steps, table=None, dtype=np.float64):
        return env_push.push_replay(states, resets, self.push_cfg, int(self.cfg.seed), self.gids, steps, self.geometry, self.inertia,
                                    self.table0 if table is None else table, dtype)

    def state_equals(self, want, what=""):
        for name in STATE:
            assert np.array_equal(words(getattr(self, name)), words(want[name].astype(getattr(self, name).cpu().numpy().dtype))), (what, name)
        return True

    return type("HipEnvPushed", (H,), {"__init__": init, "bind_tables": bind_tables, "bind_push": bind_push, "push": push,
                                       "guards_intact": guards_intact, "replay": replay, "state_equals": state_equals})


def check_launch(env, before, after, want64, want32, what):
    """One launch: everything that is exact, bit for bit; returns the two velocity errors of the envs it stored."""
    stored, quiet = np.flatnonzero(want64["stored"]), np.flatnonzero(~want64["stored"])
    assert np.array_equal(words(after[REST]), words(before[REST])), "%s: a field other than the velocities changed" % what
    assert np.array_equal(words(after[QD][:, quiet]), words(before[QD][:, quiet])), "%s: velocities of an env not pushed" % what
    assert env.state_equals(want64, what) and env.guards_intact()
    return velocity_error(after, before, want64, stored), velocity_error(np.ascontiguousarray(_with_qd(before, want32["qd"])), before, want64, stored)


def _with_qd(state, qd):
    out = state.copy()
    out[QD] = qd.T
    return out


# ------------------------------------------------------------------------------------------------------ the launch alone
@pytest.mark.parametrize("bound", [False, True])
def test_launch_alone_equals_the_replay_after_every_launch(Pushed, bound):
    """48 launches on hand-made states, reset set by hand, the step count set to the index the launch rides behind; rates
    {0, 0.3, 1} x impulses {0, 0.002, 0.01} in every wave, points [0, 2, 5]; without a table and with an inertia table of nine
    different mass sets.  Worst velocity error over all launches, of max |dqd|, measured on one MI355X:
    no table: kernel 9.4e-04, float32 restatement 9.4e-04;  table: kernel 1.09e-03, float32 restatement 1.09e-03.
    The two agree to the digits printed: the worst cases are the smallest impulses, where the rounding of qd + dqd to
    float32 (half an ulp of a velocity near 3 over a dqd of 1e-4) is the whole error, in the kernel as in the restatement."""
    env = Pushed(case_cfg("free"))
    if bound:
        env.bind_tables(table_of(env.lib, env.cfg, N))
    spec = config(RATE={"values": [0.0, 0.3, 1.0]}, IMPULSE={"values": [0.0, 0.002, 0.01]}, POINTS=[0, 2, 5])
    env.bind_push(spec)
    e = np.arange(N)
    assert np.array_equal(env.table0, np.stack([np.asarray([0.0, 0.3, 1.0], np.float32)[e % 3], np.asarray([0.0, 0.002, 0.01], np.float32)[(e // 3) % 3]]))
    steps = 48
    _, resets = hand_flags(steps, N)
    states = np.stack([hand_state(t, N) for t in range(steps)])
    index = np.arange(steps) + 3
    want64, want32 = env.replay(states, resets, index), env.replay(states, resets, index, dtype=np.float32)
    worst, worst32, pushed, stored, points = 0.0, 0.0, 0, 0, set()
    for t in range(steps):
        env.step_count = int(index[t]) + 1                       # the launch rides behind the step with this index
        env.set_state(states[t])
        env.set_flags(resets[t], np.zeros(N))
        assert env.push() == abi.OK
        torch.cuda.synchronize()
        after = env.state_t.cpu().numpy()
        err, err32 = check_launch(env, states[t], after, want64[t], want32[t], "launch %d" % t)
        worst, worst32 = max(worst, err), max(worst32, err32)
        assert not want64[t]["pushed"][resets[t] != 0].any()
        pushed, stored = pushed + int(want64[t]["pushed"].sum()), stored + int(want64[t]["stored"].sum())
        points |= set(want64[t]["point"][want64[t]["stored"]].tolist())
    print("launch alone (table bound: %s): worst velocity error %.3g of max |dqd|, float32 restatement %.3g" % (bound, worst, worst32))
    assert pushed > stored > 500 and points == {0, 2, 5} and worst32 > 0.0
    assert worst <= FACTOR * worst32, (worst, worst32)
    assert np.array_equal(words(env.table), words(env.table0)) and int(env.episode_index.abs().max()) == 0      # held: never rewritten
    assert np.array_equal(env.push_count.cpu().numpy(), sum(w["pushed"] for w in want64))
    env.close()


def test_per_episode_rewrites_flagged_envs_only(Pushed):
    env = Pushed(case_cfg("free", offset=1000))
    env.bind_push(config(**SPEC))
    steps = 30
    _, resets = hand_flags(steps, N)
    quiet = [5, 63, 64, N - 1]                                   # never flagged: their (hand-made) entries must survive
    resets[:, quiet] = 0
    table = env.table0.copy()
    table[:, quiet] = np.asarray([[0.625], [0.00456]], dtype=np.float32)
    env.table.copy_(torch.as_tensor(table))
    states = np.stack([hand_state(t, N, seed=2) for t in range(steps)])
    want = env.replay(states, resets, np.arange(steps), table=table)
    for t in range(steps):
        env.step_count = t + 1
        env.set_state(states[t])
        env.set_flags(resets[t], np.zeros(N))
        assert env.push() == abi.OK
        torch.cuda.synchronize()
        assert env.state_equals(want[t], "launch %d" % t) and env.guards_intact()
        assert np.array_equal(words(env.table[:, quiet]), words(table[:, quiet]))
    episodes = env.episode_index.cpu().numpy()
    assert np.array_equal(episodes, resets.sum(axis=0)) and episodes.max() >= 3 and (episodes[quiet] == 0).all()
    assert np.array_equal(words(env.table), words(np.where(episodes > 0, env_push.draw_push(env.push_cfg, int(env.cfg.seed), env.gids,
                                                                                          episodes).astype(np.float32), table)))
    assert int(env.push_count[quiet].min()) > 0
    env.close()


def test_refusals_on_a_handle(Pushed):
    env = Pushed(case_cfg("free"))
    env.bind_push(config(**SPEC))
    lib, stream = env.lib, torch.cuda.current_stream().cuda_stream
    args = [env.h, env.pspec, env.reset_t.data_ptr(), env.table.data_ptr(), env.episode_index.data_ptr(), env.push_count.data_ptr(), stream]
    for k in range(6):
        bad = list(args)
        bad[k] = None
        assert lib.vine_env_push_scheduled(*bad) == abi.ERR_INVALID_ARG and b"null argument" in lib.vine_last_error()
    unchecked = abi.VineEnvPushSpec.from_buffer_copy(env.pspec)
    unchecked.checked = 0
    bad = list(args)
    bad[1] = unchecked
    assert lib.vine_env_push_scheduled(*bad) == abi.ERR_INVALID_ARG and b"not filled by" in lib.vine_last_error()
    assert env.guards_intact()
    env.close()


# -------------------------------------------------------------------------------------------------- behind real steps
def run_pair(Pushed, case, offset=0, n=N, acts=None, follow=True):
    """Handle A with the launch behind every step; handle B without it, fed the same actions, into which A's six velocity
    rows are copied after every step (``follow``).  Per step everything both wrote, and A's state block before its launch."""
    acts = actions_for(N, T) if acts is None else acts
    a, b = Pushed(case_cfg(case, n, offset)), (Pushed(case_cfg(case, n, offset)) if follow else None)
    a.bind_push(config(**SPEC))
    keys = ("obs", "rew", "reset", "progress", "timeouts", "state")
    ra, rb, before = {k: [] for k in keys}, {k: [] for k in keys}, []
    for act in acts:
        for env, rec in ((a, ra), (b, rb)):
            if env is None:
                continue
            env.step_t(act.to(env.dev).contiguous(), sync=False)
            if env is a:
                before.append(a.state_t.clone())
                assert a.push() == abi.OK
            else:
                b.state_t[QD].copy_(a.state_t[QD])
            for k, t in zip(keys, (env.obs_t, env.rew_t, env.reset_t, env.progress_t, env.timeouts_t, env.state_t)):
                rec[k].append(t.clone())
    torch.cuda.synchronize()
    ra, rb = ({k: torch.stack(v).cpu().numpy() for k, v in r.items()} if r["obs"] else None for r in (ra, rb))
    return a, b, ra, rb, torch.stack(before).cpu().numpy()


@pytest.mark.parametrize("case,offset", [("free", 0), ("pipe", 0), ("free", 1000)])
def test_behind_real_steps_the_push_writes_nothing_but_the_velocities(Pushed, case, offset):
    """Worst velocity error over the 40 steps, of max |dqd|, measured (kernel = float32 restatement to the digits printed):
    free 1.11e-04, pipe 2.74e-04, free at offset 1000 8.72e-04."""
    a, b, ra, rb, before = run_pair(Pushed, case, offset)
    assert saw_resets_and_timeouts(ra), case
    assert_bit_equal(ra, rb, what=case)                              # state block, observations, rewards, flags, progress
    want64, want32 = a.replay(before, ra["reset"], np.arange(T)), a.replay(before, ra["reset"], np.arange(T), dtype=np.float32)
    worst, worst32, stored = 0.0, 0.0, 0
    for t in range(T):
        f, quiet = np.flatnonzero(want64[t]["stored"]), ~want64[t]["stored"]
        worst = max(worst, velocity_error(ra["state"][t], before[t], want64[t], f))
        worst32 = max(worst32, velocity_error(_with_qd(before[t], want32[t]["qd"]), before[t], want64[t], f))
        stored += len(f)
        assert np.array_equal(words(ra["state"][t][REST]), words(before[t][REST])), (case, t)
        assert np.array_equal(words(ra["state"][t][QD][:, quiet]), words(before[t][QD][:, quiet])), (case, t)
        assert not want64[t]["pushed"][ra["reset"][t] != 0].any()
    assert a.state_equals(want64[-1], case)                          # table, ordinals and counts behind the last launch
    print("%s at offset %d: worst velocity error %.3g of max |dqd|, float32 restatement %.3g" % (case, offset, worst, worst32))
    assert stored > 200 and worst <= FACTOR * worst32, (worst, worst32)
    assert want64[-1]["episode_index"].max() >= 2 and a.guards_intact() and b.guards_intact()
    a.close()
    b.close()
    if case == "free" and offset == 0:                               # a 35-env shard at offset 35 is the whole batch's upper half
        acts = actions_for(N, T)
        s, _, rs, _, _ = run_pair(Pushed, case, 35, 35, acts[:, 35:], follow=False)
        assert np.array_equal(words(rs["state"]), words(ra["state"][:, :, 35:])) and np.array_equal(words(rs["obs"]), words(ra["obs"][:, 35:]))
        assert np.array_equal(words(s.table), words(want64[-1]["table"][:, 35:]))
        assert np.array_equal(s.episode_index.cpu().numpy(), want64[-1]["episode_index"][35:])
        assert np.array_equal(s.push_count.cpu().numpy(), want64[-1]["push_count"][35:]) and s.guards_intact()
        s.close()


def test_captured_groups_of_four_steps_replay_like_eager_launches(Pushed):
    """Four (step + launch) pairs captured once, replayed ten times, against the same forty pairs launched eagerly."""
    acts = actions_for(N, T).cuda()
    envs = []
    for graphed in (False, True):
        env = Pushed(case_cfg("randomize-noise"))
        env.bind_push(config(**SPEC))
        env.slots = torch.zeros(4, N, 28, device="cuda")
        a_in = torch.zeros(4, N, 2, device="cuda")
        torch.cuda.synchronize()

        def group():
            for k in range(4):
                native.check(env.lib.vine_step(env.h, a_in[k].data_ptr(), env.slots[k].data_ptr(), env.rew_t.data_ptr(),
                                               env.reset_t.data_ptr(), env.progress_t.data_ptr(), env.timeouts_t.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), env.lib)
                assert env.push() == abi.OK
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
    assert int(eager.episode_index.max()) >= 2 and int(eager.push_count.sum()) > 200 and eager.guards_intact() and g_env.guards_intact()
    eager.close()
    g_env.close()


# ----------------------------------------------------------------------------------------------------- the task class
class Tap:
    """A step observer that keeps a copy of the state block and of the step's reset flags at its place in the order."""
    paused, copy_done = 0, None

    def __init__(self, env):
        self.env, self.state, self.reset = env, [], []

    def enqueue(self, stream, actions=None):
        self.state.append(self.env._state.clone())
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
        return tuple(torch.stack(v).cpu().numpy() for v in (self.state, self.reset))


def make_task(n, extra, push=None, env_params_spec=None, sensor=None, seed=42):
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_config(overrides=["num_envs=%d" % n, "task.env.CREATE_PIPE=False", "task.env.maxEpisodeLength=%d" % MAX_LEN] + list(extra))
    cfg["task"]["seed"] = seed
    cfg["task"]["env"]["ENV_PUSH"] = dict(SPEC if push is None else push)
    if env_params_spec:
        cfg["task"]["env"]["ENV_PARAMS"] = env_params_spec
    if sensor:
        cfg["task"]["env"]["ENV_SENSOR"] = sensor
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                  headless=True)
    front, behind = Tap(env), Tap(env)
    at = env._observers.index(env.env_push)
    env._observers.insert(at + 1, behind)
    env._observers.insert(at, front)
    return env, front, behind


def check_task_run(env, front, behind, steps):
    """Every launch of a task-class run against the replay of what the tap in front of it saw; the observer's final state;
    every episode-log row's param_PUSH_* against the replay's table for that episode."""
    before, resets = front.arrays()
    after, _ = behind.arrays()
    p = env.env_push
    assert len(before) == steps == int(env.step_count) and env._lib.vine_env_inertia_bound(env._handle) == 0
    gids, geometry = np.arange(env.num_envs) + p.env_id_offset, env_push.geometry_of(env._lib, env._vcfg)
    want64 = env_push.push_replay(before, resets, p.spec, p.seed, gids, np.arange(steps), geometry)
    want32 = env_push.push_replay(before, resets, p.spec, p.seed, gids, np.arange(steps), geometry, dtype=np.float32)
    worst, worst32, stored = 0.0, 0.0, 0
    for t in range(steps):
        f, quiet = np.flatnonzero(want64[t]["stored"]), ~want64[t]["stored"]
        assert np.array_equal(words(after[t][REST]), words(before[t][REST])), t
        assert np.array_equal(words(after[t][QD][:, quiet]), words(before[t][QD][:, quiet])), t
        worst = max(worst, velocity_error(after[t], before[t], want64[t], f))
        worst32 = max(worst32, velocity_error(_with_qd(before[t], want32[t]["qd"]), before[t], want64[t], f))
        stored += len(f)
    print("task class: worst velocity error %.3g of max |dqd|, float32 restatement %.3g" % (worst, worst32))
    assert stored > 200 and worst <= FACTOR * worst32, (worst, worst32)
    for name in STATE:
        assert np.array_equal(words(getattr(p, name)), words(want64[-1][name].astype(getattr(p, name).cpu().numpy().dtype))), name
    assert [t.data_ptr() for t in p.live_tensors()] == [t.data_ptr() for t in (p.table, p.episode_index, p.push_count)]
    live = [t.data_ptr() for t in env.live_tensors()]
    assert live[0] == env._state.data_ptr() and all(t.data_ptr() in live for t in p.live_tensors())      # the state block is the env's own
    env.episode_log.harvest()
    rows = env.episode_log.rows_with_params()
    assert len(rows["env"]) > env.num_envs and rows["episode"].max() >= 1
    first = env_push.draw_push(p.spec, p.seed, gids, 0).astype(np.float32)
    tables = np.stack([first] + [w["table"] for w in want64[:-1]])          # the values in force while the row's last step ran
    for slot, name in enumerate(env_push.DRAW_NAMES):
        assert np.array_equal(words(rows["param_" + name]), words(tables[rows["end_step"], slot, rows["env"]])), name
    return want64, rows


def test_every_step_entry_of_the_task_class_pushes_as_the_replay(tmp_path):
    """step, step_into, the fused rollout step and the evaluation step, ten of each in one run on the four-lane kernel, with
    ENV_SENSOR also on.  (With ENV_PARAMS_PER_EPISODE a parameter table is bound and the step takes the one-lane kernel:
    that combination is the next test's.)  Measured: kernel 3.43e-04 of max |dqd|, float32 restatement 3.43e-04."""
    from tests.test_eval_step import H, _eval_args, _eval_state, _head
    n = 256
    env, front, behind = make_task(n, ["task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_DIR=" + str(tmp_path)],
                                   sensor={"DELAY": [0, 3], "NOISE_STD": 0.01, "PER_EPISODE": True})
    try:
        lib, dev, st = env._lib, torch.device("cuda:0"), torch.cuda.current_stream().cuda_stream
        assert env.step_kernel_name == "vine_step_quad_kernel" and env.rollout_step_blocks() > 0 and env.eval_step_rows() > 0
        assert env.observers[-1] is behind and env.observers[-2] is env.env_push and env.observers[-4] is env.env_sensor
        assert env.episode_log.push is env.env_push
        p, rnd = _head(dev, lib, st)
        acts = actions_for(n, 20, seed=11).cuda()
        out = torch.zeros(10, n, env.num_obs, device=dev)
        for k in range(10):
            env.step(acts[k])
        for k in range(10):
            env.step_into(acts[10 + k], out[k])
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
            env.step_rollout_into(ra, out[k])
            torch.cuda.synchronize()
            p["counter"] += 1
        se = _eval_state(env, n, dev)
        for k in range(10):
            y = rnd(n, H)
            env.step_eval_into(_eval_args(se, p, y, 1), out[k])
            torch.cuda.synchronize()
        want, rows = check_task_run(env, front, behind, 40)
        assert np.array_equal(env.env_sensor.episodes_now(), env.env_push.episodes_now()) and env.env_push.episodes_now().max() >= 2
        path = env.episode_log.path
    finally:
        env.close()
    from vine_robot_isaacgymenvs_amd.utils import episodes
    back = episodes.load_rows_with_params(path)
    for name in env_push.DRAW_NAMES:
        assert np.array_equal(words(back["param_" + name]), words(rows["param_" + name]))
    assert "param_SENSOR_DELAY" in back


def test_with_the_sensor_and_the_redraw_on_the_three_ordinals_are_equal(tmp_path):
    plants = {"DAMPING": [0.01, 0.05], "ACTION_DELAY": [0, 3]}
    env, front, behind = make_task(N, ["task.env.ENV_PARAMS_PER_EPISODE=True", "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_DIR=" + str(tmp_path)],
                                   env_params_spec=plants, sensor={"DELAY": [0, 3], "HOLD": 0.1, "PER_EPISODE": True})
    try:
        assert env.observers[-1] is env.env_redraw and env.observers[-3] is env.env_push and env.observers[-5] is env.env_sensor
        acts = actions_for(N, T, seed=7).cuda()
        obs = torch.zeros(N, env.num_obs, device="cuda")
        for k in range(T):
            env.step_into(acts[k], obs)
        check_task_run(env, front, behind, T)
        ordinals = env.env_redraw.episodes_now()
        assert np.array_equal(env.env_push.episodes_now(), ordinals) and np.array_equal(env.env_sensor.episodes_now(), ordinals)
        assert ordinals.max() >= 2
        rows = env.episode_log.rows_with_params()
        assert "param_DAMPING" in rows and "param_SENSOR_DELAY" in rows and "param_PUSH_RATE" in rows and "param_PUSH_IMPULSE" in rows
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------ train.py's entry
def test_train_and_play_entries_with_pushes_on(tmp_path, monkeypatch, capsys):
    """Two training iterations (horizon 8) with pushes on: finite scalars, the fused rollout (3 launches per step, the
    observers' behind them) and the four-lane kernel in force.  Then test=True with IMPULSE {values: [0, 0.005, 0.01]} and the
    episode log: the printed report has a param_PUSH_IMPULSE block with three values."""
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    from vine_robot_isaacgymenvs_amd.learning.player import PpoPlayerContinuous
    from vine_robot_isaacgymenvs_amd.train import main
    from vine_robot_isaacgymenvs_amd.utils import tfevents
    monkeypatch.chdir(tmp_path)
    common = ["task=Vine5LinkMovingBase", "num_envs=512", "headless=True", "experiment=pushed", "task.env.CREATE_PIPE=False",
              "task.env.maxEpisodeLength=%d" % MAX_LEN, "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_CAPACITY=32768"]
    seen = {}
    play = A2CAgent.play_steps_rnn

    def play_and_keep(self):
        out = play(self)
        env = getattr(self.vec_env, "env", self.vec_env)
        seen.update(launches=self.rollout_step_launches, kernel=env.step_kernel_name, push=env.env_push.spec,
                    observers=[type(o).__name__ for o in env.observers], pushes=int(env.env_push.push_count.sum()))
        return out
    monkeypatch.setattr(A2CAgent, "play_steps_rnn", play_and_keep)
    main(common + ["minibatch_size=2048", "max_iterations=2", "train.params.config.horizon_length=8",
                   "train.params.config.save_frequency=1", "train.params.config.save_best_after=0", "+train.params.config.print_stats=False",
                   "task.env.ENV_PUSH={RATE: 0.2, IMPULSE: [0.0, 0.01], PER_EPISODE: True}",
                   "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "train")])
    torch.cuda.synchronize()
    monkeypatch.setattr(A2CAgent, "play_steps_rnn", play)
    assert seen["launches"] == 3 and seen["kernel"] == "vine_step_quad_kernel" and seen["push"]["PER_EPISODE"] is True
    assert seen["observers"] == ["EpisodeLog", "EnvPush"] and seen["pushes"] > 512
    run = tmp_path / "runs" / "pushed"
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
                                   "task.env.ENV_PUSH={RATE: 0.2, IMPULSE: {values: [0, 0.005, 0.01]}}",
                                   "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "play")])
    out = capsys.readouterr().out
    assert np.isfinite(reward) and steps > 0
    assert "reached_ever_rate by param_PUSH_IMPULSE:" in out
    impulses, rate, count = kept["player"].report["by_param"]["param_PUSH_IMPULSE"]
    assert np.array_equal(impulses, np.asarray([0.0, 0.005, 0.01], dtype=np.float32)) and count.min() > 0
    assert int(count.sum()) == kept["player"].report["episodes"]
