"""ENV_PARAMS_ADR on the GPU: the two launches of include/vine_env_adr.h alone against utils/env_params.py adr_replay, their
reduction to the redraw node, behind every step against the host writing the replay's columns between steps, under
env_id_offset, in a replayed graph, and through the task class, the episode log and train.py's entry points.

The shapes are those of tests/test_env_params_per_episode_gpu.py: 70 envs = two waves, the second partial; 12-step episodes,
40 steps; QUEUE 4, BOUNDARY_FRACTION 0.5.  Every comparison is on integers or on 32-bit words."""
import glob
import logging

import numpy as np
import pytest
import torch

from tests.helpers import base_cfg, f6_cfg
from tests.test_env_params_gpu import MAX_LEN, N, T, actions_for, assert_bit_equal
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params

pytestmark = pytest.mark.gpu

# the limits: the three mass names, DAMPING and the delay over all nine values under ADR; FPAM_K and FPAM_b redrawn as today
SPEC = {"DAMPING": [0.005, 0.1], "ACTION_DELAY": [0, 8], "FPAM_K": [0.9, 1.1], "FPAM_b": {"values": [0.9, 1.1]},
        "CART_MASS": [0.35, 0.7], "LINK_MASS": [0.7, 1.4], "TIP_LINK_MASS": [1.0, 2.0]}
# at most four steps from START to a limit, so that 40 launches get there and back; TIP_LINK_MASS starts AT its lower limit
NAMES = {"DAMPING": {"START": [0.02, 0.03], "STEP": 0.02}, "ACTION_DELAY": {"START": [2, 3], "STEP": 2},
         "CART_MASS": {"START": [0.5, 0.5], "STEP": 0.1}, "LINK_MASS": {"START": [1.0, 1.0], "STEP": 0.15},
         "TIP_LINK_MASS": {"START": [1.0, 1.2], "STEP": 0.4}}
ADR = {"NAMES": NAMES, "BOUNDARY_FRACTION": 0.5, "QUEUE": 4, "WIDEN_AT": 0.8, "NARROW_AT": 0.4, "HISTORY_CAPACITY": 64}
RING = slice(abi.VF_FIFO0, abi.VF_FIFO0 + 2 * abi.MAX_DELAY)
SENTINEL = np.float32(-777.25)
# SUCCESS_DIST, chosen so that some episodes reach and some do not (the tests assert both): under random actions, within 12
# steps, about three quarters of the free-space episodes come within 0.5 m of their target (a tenth within 0.3 m, nearly all
# within 0.8 m); the pipe's targets lie closer, half of its episodes come within 0.25 m
SUCCESS_DIST = 0.5
SUCCESS_DIST_PIPE = 0.25
STATE = ("widen", "counts", "probe", "reached", "episode_index")


def words(t):
    t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return t.view(np.uint32) if t.dtype == np.float32 else t


def adr_of(**keys):
    return env_params.adr_config({"ENV_PARAMS": SPEC, "ENV_PARAMS_PER_EPISODE": True, "ENV_PARAMS_ADR": dict(ADR, **keys)})


@pytest.fixture(scope="module")
def Lane():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    from tests.hip_env import HipEnv as H

    def bind_adr(self, adr, spec=SPEC):
        """Both tables of START at episode 0, uploaded and bound; a reward matrix; the ADR spec and its zeroed state."""
        off = int(self.cfg.env_id_offset)
        self.spec, self.adr = spec, adr
        start = env_params.adr_start_spec(spec, adr)
        self.table_t = torch.as_tensor(env_params.build_table(start, self.cfg, int(self.cfg.seed), self.n, off, lib=self.lib)).to(self.dev)
        self.inertia_t = torch.as_tensor(env_params.build_inertia_table(start, self.cfg, int(self.cfg.seed), self.n, off,
                                                                        lib=self.lib)).to(self.dev)
        torch.cuda.synchronize(self.dev)
        native.check(self.lib.vine_bind_env_params(self.h, self.table_t.data_ptr()), self.lib)
        native.check(self.lib.vine_bind_env_inertia(self.h, self.inertia_t.data_ptr()), self.lib)
        self.bind_reward_matrix()
        _, values = env_params.redraw_names(spec)
        self.values_t = torch.as_tensor(values, dtype=torch.float64).to(self.dev)
        self.aspec = env_params.adr_spec(self.lib, self.cfg, spec, adr, self.values_t.data_ptr())
        self.rspec = self.aspec.redraw
        i32 = dict(dtype=torch.int32, device=self.dev)
        self.episode_index_t = torch.zeros(self.n, **i32)
        self.widen_t, self.counts_t = torch.zeros((abi.VR_NAMES, 2), **i32), torch.zeros((abi.VR_NAMES, 2, 2), **i32)
        self.reached_t, self.probe_t = torch.zeros(self.n, **i32), torch.full((self.n,), -1, **i32)
        self.history_t = torch.zeros((adr["HISTORY_CAPACITY"], 4), **i32)
        self.cursor_t = torch.zeros(1, dtype=torch.int64, device=self.dev)
        torch.cuda.synchronize(self.dev)

    def adr_args(self):
        return [self.h, self.aspec, self.reset_t.data_ptr(), self.table_t.data_ptr(), self.inertia_t.data_ptr(),
                self.episode_index_t.data_ptr(), self.widen_t.data_ptr(), self.counts_t.data_ptr(), self.reached_t.data_ptr(),
                self.probe_t.data_ptr(), self.history_t.data_ptr(), self.cursor_t.data_ptr(),
                torch.cuda.current_stream(self.dev).cuda_stream]

    def node(self):
        """The two launches, behind whatever is on the stream."""
        return self.lib.vine_env_adr_scheduled(*adr_args(self))

    def redraw_node(self):
        return self.lib.vine_env_redraw_scheduled(self.h, self.rspec, self.reset_t.data_ptr(), self.table_t.data_ptr(),
                                                  self.inertia_t.data_ptr(), self.episode_index_t.data_ptr(),
                                                  torch.cuda.current_stream(self.dev).cuda_stream)

    def snapshot(self):
        """Clones of everything the node owns or writes, at this point of the stream."""
        return {k: getattr(self, k + "_t").clone() for k in STATE + ("table", "inertia", "history", "cursor")}

    return type("HipEnvAdr", (H,), {"kernel": "lane", "bind_adr": bind_adr, "adr_args": adr_args, "node": node,
                                    "redraw_node": redraw_node, "snapshot": snapshot})


def assert_equals_replay(got, want, capacity, what):
    """One snapshot (host arrays) against one step of adr_replay: the integers, both tables, the history rows and cursor."""
    for k in STATE:
        assert np.array_equal(got[k].astype(np.int64), want[k]), "%s: %s" % (what, k)
    assert np.array_equal(words(got["table"]), words(want["params"])), "%s: parameter table" % what
    assert np.array_equal(words(got["inertia"]), words(want["inertia"])), "%s: inertia table" % what
    assert int(got["cursor"][0]) == want["cursor"] <= capacity, what
    assert np.array_equal(got["history"][:want["cursor"]].astype(np.int64), want["history"]), "%s: history rows" % what
    assert not got["history"][want["cursor"]:].any(), "%s: the ring beyond the cursor" % what


def host(snap):
    return {k: v.cpu().numpy() for k, v in snap.items()}


def moves_of(history, max_widen):
    """What the history shows: a widening, a narrowing, a boundary arriving at its limit, a boundary back at START."""
    last, seen = {}, set()
    for _, b, w, _ in history:
        seen.add("widen" if w > last.get(b, 0) else "narrow")
        if w == max_widen[b >> 1, b & 1]:
            seen.add("limit")
        if w == 0:
            seen.add("start")
        last[b] = w
    return seen


def plain_cfg(seed=21, offset=0):
    cfg = base_cfg(N, 0, False, max_episode_length=MAX_LEN, seed=seed)
    cfg.env_id_offset, cfg.success_dist = offset, SUCCESS_DIST
    return cfg


# ------------------------------------------------------------------------------------------------------- the node alone
def test_node_alone_equals_the_replay_after_every_launch(Lane):
    """48 launch pairs on hand-set flags: two thirds of the envs flagged per launch, the first and the last lane and both
    sides of the wave boundary among them in turn; reward column 2 written by the test: all ones for 24 launches, then all
    zeros.  After EVERY launch all of the node's state equals adr_replay; the unflagged columns, the unnamed rows and the rest
    of the state block are untouched; the history shows a widening, a narrowing, a stop at a limit and a stop at START."""
    launches = 48
    adr = adr_of()
    env = Lane(plain_cfg())
    env.bind_adr(adr)
    flags = np.zeros((launches, N), dtype=np.int64)
    for t in range(launches):
        flags[t] = (np.arange(N) + t) % 3 != 0
        flags[t, [0, 63, 64, N - 1]] = [t % 2, (t + 1) % 2, t % 2, (t // 2) % 2]
    assert all(flags[:, e].min() == 0 and flags[:, e].max() == 1 for e in (0, 1, 62, 63, 64, 65, N - 1))
    reach = np.zeros((launches, N), dtype=np.int64)
    reach[:24] = 1
    reach[:, 5] = 0                                               # one env never reaches, one always
    reach[:, 66] = 1
    want = env_params.adr_replay(SPEC, adr, int(env.cfg.seed), np.arange(N), flags, reach, env.cfg, lib=env.lib,
                                 step_index=np.full(launches, -1))
    named = sorted(r for name in SPEC if name in abi.ENV_PARAM_ROWS for r in range(abi.ENV_PARAM_ROWS[name][0], sum(abi.ENV_PARAM_ROWS[name])))
    unnamed = [r for r in range(abi.VP_COUNT) if r not in named]
    env.table_t[unnamed] = float(SENTINEL)
    rng = np.random.default_rng(0)
    state0 = rng.uniform(-1.0, 1.0, (abi.VF_COUNT, N)).astype(np.float32)
    state0[RING][state0[RING] == 0.0] = 0.5
    env.state_t.copy_(torch.as_tensor(state0))
    rm0 = rng.uniform(-1.0, 1.0, (N, abi.NUM_REWARDS)).astype(np.float32)
    saw_ring = False
    for t in range(launches):
        rm0[:, 2] = reach[t]
        env.reward_matrix_t.copy_(torch.as_tensor(rm0))
        env.reset_t.copy_(torch.as_tensor(flags[t]))
        before = env.table_t.cpu().numpy()
        assert env.node() == abi.OK
        torch.cuda.synchronize()
        got = host(env.snapshot())
        w = dict(want[t], params=want[t]["params"].copy())
        w["params"][unnamed] = SENTINEL                            # rows the spec does not name are never written
        assert_equals_replay(got, w, adr["HISTORY_CAPACITY"], "launch %d" % t)
        clear = np.flatnonzero(flags[t] == 0)
        assert np.array_equal(words(got["table"][:, clear]), words(before[:, clear]))
        state0[RING][:, want[t]["delay_changed"]] = 0.0           # the ring is zeroed exactly where the delay changed,
        saw_ring = saw_ring or want[t]["delay_changed"].any()
        assert np.array_equal(words(env.state_t), words(state0)), "the state block, launch %d" % t      # nothing else is written
        assert np.array_equal(words(env.reward_matrix_t), words(rm0)) and np.array_equal(env.reset_t.cpu().numpy(), flags[t])
    assert saw_ring and want[-1]["cursor"] >= 12
    assert moves_of(want[-1]["history"], env_params.adr_max_widen(SPEC, adr)) == {"widen", "narrow", "limit", "start"}
    assert not want[-1]["widen"].any() and want[23]["widen"].sum() >= 12      # there and back
    probes = np.concatenate([w["probe"] for w in want])
    assert set(probes.tolist()) == {-1} | {2 * abi.ENV_REDRAW_NAMES.index(n) + s for n in NAMES for s in (0, 1)}
    env.close()


def test_refusals_on_a_handle(Lane):
    env = Lane(plain_cfg())
    lib = env.lib
    env.bind_adr(adr_of())
    args = env.adr_args()
    assert lib.vine_env_adr_scheduled(*args) == abi.OK
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11):
        bad = list(args)
        bad[k] = None
        assert lib.vine_env_adr_scheduled(*bad) == abi.ERR_INVALID_ARG and b"null argument" in lib.vine_last_error(), k
    bad = list(args)
    bad[4] = None
    assert lib.vine_env_adr_scheduled(*bad) == abi.ERR_INVALID_ARG and b"needs an inertia table" in lib.vine_last_error()
    other = env.table_t.clone()
    bad = list(args)
    bad[3] = other.data_ptr()
    assert lib.vine_env_adr_scheduled(*bad) == abi.ERR_INVALID_ARG and b"not the table bound" in lib.vine_last_error()
    unchecked = abi.VineEnvAdrSpec.from_buffer_copy(env.aspec)
    unchecked.checked = 0
    bad = list(args)
    bad[1] = unchecked
    assert lib.vine_env_adr_scheduled(*bad) == abi.ERR_INVALID_ARG and b"not filled by vine_env_adr_spec" in lib.vine_last_error()
    native.check(lib.vine_bind_reward_matrix(env.h, None), lib)
    assert lib.vine_env_adr_scheduled(*args) == abi.ERR_INVALID_ARG and b"needs a reward matrix" in lib.vine_last_error()
    native.check(lib.vine_bind_reward_matrix(env.h, env.reward_matrix_t.data_ptr()), lib)
    native.check(lib.vine_bind_env_inertia(env.h, None), lib)
    assert lib.vine_env_adr_scheduled(*args) == abi.ERR_INVALID_ARG and b"needs an inertia table" in lib.vine_last_error()
    native.check(lib.vine_bind_env_params(env.h, None), lib)
    assert lib.vine_env_adr_scheduled(*args) == abi.ERR_INVALID_ARG and b"needs a parameter table" in lib.vine_last_error()
    torch.cuda.synchronize()
    env.close()


def test_reduction_to_the_redraw_node_on_the_device(Lane):
    """BOUNDARY_FRACTION 0 and START = the limits: after every launch both tables, the rings and the episode counters equal
    those vine_env_redraw_scheduled writes on a second handle from the same flags."""
    names = {n: {"START": list(SPEC[n]), "STEP": NAMES[n]["STEP"]} for n in NAMES}
    adr = adr_of(NAMES=names, BOUNDARY_FRACTION=0.0)
    a, b = Lane(plain_cfg()), Lane(plain_cfg())
    a.bind_adr(adr)
    b.bind_adr(adr)
    rng = np.random.default_rng(1)
    state0 = rng.uniform(-1.0, 1.0, (abi.VF_COUNT, N)).astype(np.float32)
    for env in (a, b):
        env.state_t.copy_(torch.as_tensor(state0))
        env.reward_matrix_t.fill_(1.0)
    assert np.array_equal(words(a.table_t), words(b.table_t))
    for t in range(8):
        flags = torch.as_tensor((rng.uniform(size=N) < 0.4).astype(np.int64))
        flags[[0, 63, 64, N - 1]] = torch.as_tensor([t % 2, 1, (t + 1) % 2, 1])
        a.reset_t.copy_(flags)
        b.reset_t.copy_(flags)
        assert a.node() == abi.OK and b.redraw_node() == abi.OK
        torch.cuda.synchronize()
        for name in ("table_t", "inertia_t", "state_t", "episode_index_t"):
            assert np.array_equal(words(getattr(a, name)), words(getattr(b, name))), (name, t)
        assert not a.widen_t.any() and not a.counts_t.any() and (a.probe_t == -1).all() and int(a.cursor_t) == 0
    assert not np.array_equal(words(a.state_t), words(state0)) and int(a.episode_index_t.max()) >= 4
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- behind real steps
def equivalence_cfg(case):
    if case == "free":
        return plain_cfg()
    if case == "pipe":
        cfg = f6_cfg(N, 1, 0, "pipe")
        cfg.max_episode_length, cfg.seed, cfg.success_dist = MAX_LEN, 22, SUCCESS_DIST_PIPE
        return cfg
    cfg = base_cfg(N, 0, True, max_episode_length=MAX_LEN, seed=23)
    cfg.obs_noise_std, cfg.action_noise_std, cfg.dyn_scale_min, cfg.dyn_scale_max = 0.01, 0.02, 0.9, 1.1
    cfg.success_dist = SUCCESS_DIST
    if case == "offset":
        cfg.env_id_offset = 1000
    return cfg


def run_with(env, actions, after_step):
    keys = ("obs", "rew", "reset", "progress", "timeouts", "state")
    rec = {k: [] for k in keys + ("reach", "snap")}
    for t, a in enumerate(actions):
        env.step_t(a.to(env.dev).contiguous(), sync=False)
        rec["reach"].append(env.reward_matrix_t[:, 2].clone())      # what the launches behind this step see
        after_step(t)
        for k in keys:
            rec[k].append(getattr(env, k + "_t").clone())
        rec["snap"].append(env.snapshot())
    torch.cuda.synchronize(env.dev)
    out = {k: torch.stack(rec[k]).cpu().numpy() for k in keys + ("reach",)}
    out["snap"] = [host(s) for s in rec["snap"]]
    return out


def probing_outcomes(replay, resets, reach):
    """(reached, not reached) among the probing episodes that finished: an episode finishing behind step t probed the
    boundary the replay held in front of that step, and reached if it had before or does in that step."""
    hit = miss = 0
    for t in range(1, len(replay)):
        done = (resets[t] != 0) & (replay[t - 1]["probe"] >= 0)
        ever = (replay[t - 1]["reached"] != 0) | (reach[t] != 0)
        hit += int(np.count_nonzero(done & ever))
        miss += int(np.count_nonzero(done & ~ever))
    return hit, miss


@pytest.mark.parametrize("case", ["free", "pipe", "randomize-noise", "offset"])
def test_node_behind_every_step_equals_the_replay_and_the_host_writing_it(Lane, case):
    """Handle A: the node behind every step; its reset buffer and reward column 2 of every step go to adr_replay, and all of
    the node's state after every step equals the replay's.  Handle B: no node; after every step the host writes the replay's
    columns and zeroes the rings it names.  State block, obs, rew, reset, progress and timeouts after each of the 40 steps
    are those of A, bit for bit.  Among the probing episodes some reached and some did not."""
    acts = actions_for(N, T)
    adr = adr_of()
    a = Lane(equivalence_cfg(case))
    a.bind_adr(adr)

    def node(t):
        assert a.node() == abi.OK
    ra = run_with(a, acts, node)
    gids = np.arange(N) + int(a.cfg.env_id_offset)
    replay = env_params.adr_replay(SPEC, adr, int(a.cfg.seed), gids, ra["reset"], ra["reach"] != 0, a.cfg, lib=a.lib)
    for t in range(T):
        assert_equals_replay(ra["snap"][t], replay[t], adr["HISTORY_CAPACITY"], "%s, step %d" % (case, t))
    a.close()
    hit, miss = probing_outcomes(replay, ra["reset"], ra["reach"])
    print("%s: %d probing episodes reached, %d did not; %d history rows" % (case, hit, miss, replay[-1]["cursor"]))
    assert hit > 0 and miss > 0, case
    assert ra["reset"].sum() > N and ra["timeouts"].sum() > 0 and replay[-1]["episode_index"].max() >= 2
    if case == "offset":
        assert gids[0] == 1000

    b = Lane(equivalence_cfg(case))
    b.bind_adr(adr)

    def host_write(t):
        torch.cuda.synchronize()
        b.table_t.copy_(torch.as_tensor(replay[t]["params"]))
        b.inertia_t.copy_(torch.as_tensor(replay[t]["inertia"]))
        changed = np.flatnonzero(replay[t]["delay_changed"])
        if len(changed):
            ring = b.state_t[RING]
            ring[:, torch.as_tensor(changed, device=b.dev)] = 0.0
    rb = run_with(b, acts, host_write)
    b.close()
    keys = ("obs", "rew", "reset", "progress", "timeouts", "state")
    assert_bit_equal({k: ra[k] for k in keys}, {k: rb[k] for k in keys}, what=case)
    assert np.array_equal(words(ra["reach"]), words(rb["reach"]))


# ------------------------------------------------------------------------------------------------------------- replay
def test_captured_step_and_node_groups_replay_like_eager_launches(Lane):
    """Four (step + two launches) groups captured once and replayed ten times against the same 40 groups launched eagerly."""
    acts = actions_for(N, T).cuda()
    adr = adr_of()
    eager = Lane(equivalence_cfg("randomize-noise"))
    eager.bind_adr(adr)
    for k in range(T):
        eager.step_t(acts[k].contiguous(), sync=False)
        assert eager.node() == abi.OK
    torch.cuda.synchronize()
    g_env = Lane(equivalence_cfg("randomize-noise"))
    g_env.bind_adr(adr)
    a_in = torch.zeros(4, N, 2, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for k in range(4):
            g_env.step_t(a_in[k], sync=False)
            assert g_env.node() == abi.OK
    for r in range(10):
        a_in.copy_(acts[4 * r:4 * r + 4])
        graph.replay()
    torch.cuda.synchronize()
    assert g_env.step_count == eager.step_count == T
    for name in ("state_t", "obs_t", "rew_t", "reset_t", "progress_t", "timeouts_t", "table_t", "inertia_t", "episode_index_t",
                 "widen_t", "counts_t", "reached_t", "probe_t", "history_t", "cursor_t"):
        assert np.array_equal(words(getattr(g_env, name)), words(getattr(eager, name))), name
    assert int(eager.episode_index_t.max()) >= 2 and int(eager.cursor_t) >= 1 and int((eager.probe_t >= 0).sum()) > 0
    eager.close()
    g_env.close()


# ----------------------------------------------------------------------------------------------------- the task class
def make_env(tmp_path, extra=()):
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_config(overrides=["num_envs=%d" % N, "task.env.CREATE_PIPE=False", "task.env.maxEpisodeLength=%d" % MAX_LEN,
                                 "task.env.SUCCESS_DIST=%g" % SUCCESS_DIST, "task.env.ENV_PARAMS_PER_EPISODE=True",
                                 "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_DIR=" + str(tmp_path)] + list(extra))
    cfg["task"]["seed"] = 42
    cfg["task"]["env"]["ENV_PARAMS"] = SPEC
    cfg["task"]["env"]["ENV_PARAMS_ADR"] = ADR
    return isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                  headless=True)


def test_task_class_counts_the_log_rows_and_every_row_has_the_replays_plant(tmp_path):
    """40 steps through the task class with EPISODE_LOG: the observer is an EnvAdr, last in launch order; its state equals the
    replay of the recorded flags; counts plus what decisions consumed = the number (and the reached_ever sum) of the log rows
    whose probe >= 0; every row's param_* is the replay's column of that episode; set_env_params raises; an env reset from
    outside keeps its plant and is not counted."""
    from vine_robot_isaacgymenvs_amd.utils import env_adr, episodes
    env = make_env(tmp_path)
    try:
        adr = env.env_adr
        assert isinstance(adr, env_adr.EnvAdr) and env.env_redraw is adr and env.observers[-1] is adr
        live = {t.data_ptr() for t in adr.live_tensors()}
        for t in (adr.widen, adr.reached, adr.probe, adr.episode_index, adr.cursor, env.env_params, env.env_inertia):
            assert t.data_ptr() in live
        assert adr.counts.data_ptr() == adr.widen.data_ptr() + 4 * adr.widen.numel()      # (one block: widen, then counts)
        start = env_params.adr_start_spec(SPEC, adr.adr)
        assert np.array_equal(words(env.env_params), words(env_params.build_table(start, env._vcfg, 42, N, 0, lib=env._lib)))
        acts = actions_for(N, T, seed=7).cuda()
        obs = torch.zeros(N, env.num_obs, device="cuda")
        resets, reach = [], []
        for k in range(T):
            env.step_into(acts[k], obs)
            resets.append(env.reset_buf.cpu().numpy().copy())
            reach.append(env._reward_matrix[:, 2].cpu().numpy() != 0)
        resets = np.array(resets)
        replay = env_params.adr_replay(SPEC, adr.adr, 42, np.arange(N), resets, reach, env._vcfg, lib=env._lib)
        last = replay[-1]
        got = {"widen": adr.widen, "counts": adr.counts, "probe": adr.probe, "reached": adr.reached,
               "episode_index": adr.episode_index, "table": env.env_params, "inertia": env.env_inertia, "history": adr.history,
               "cursor": adr.cursor}
        assert_equals_replay(host(got), last, adr.capacity, "the task class")
        with pytest.raises(RuntimeError, match="the spec owns the tables"):
            env.set_env_params({"DAMPING": 0.03})
        env.episode_log.harvest()
        assert np.array_equal(adr.history_rows, last["history"]) and last["cursor"] >= 1
        rows = env.episode_log.rows_with_params()
        assert env.episode_log.unknown_plants == 0 and len(rows["env"]) == resets.sum()
        # per boundary: the device's counts + what decisions have consumed = the number, and the reached_ever sum, of the
        # log's rows that probed it
        probing = rows["probe"] >= 0
        counted = adr.counts.cpu().numpy().astype(np.int64) + last["consumed"]
        assert last["consumed"].sum() > 0
        per_boundary = np.bincount(rows["probe"][probing], minlength=2 * abi.VR_NAMES).reshape(abi.VR_NAMES, 2)
        hit = np.bincount(rows["probe"][probing], weights=rows["reached_ever"][probing], minlength=2 * abi.VR_NAMES).reshape(abi.VR_NAMES, 2)
        assert np.array_equal(counted[..., 0], per_boundary) and np.array_equal(counted[..., 1], hit.astype(np.int64))
        assert 0 < hit.sum() < per_boundary.sum()
        # every row's plant is the replay's column of (env, episode): the table behind the step that drew the episode
        at = episodes.drawn_at(rows["env"], rows["episode"], rows["end_step"])
        for r in range(len(rows["env"])):
            e = rows["env"][r]
            want = replay[at[r]] if rows["episode"][r] else None
            p = want["params"][:, e] if want else env_params.build_table(start, env._vcfg, 42, N, 0, lib=env._lib)[:, e]
            assert rows["param_DAMPING"][r] == p[abi.VP_DAMPING] and rows["param_ACTION_DELAY"][r] == p[abi.VP_ACTION_DELAY], r
            assert rows["param_FPAM_K"][r] == p[abi.VP_FPAM_K0], r
            if want:
                assert rows["param_CART_MASS"][r] == want["inertia"][abi.VI_CART_MASS, e] and rows["probe"][r] == want["probe"][e]
                assert rows["param_LINK_MASS"][r] == want["inertia"][abi.VI_LINK_MASS0, e]
        # an env reset from outside keeps its plant, and its running episode is not counted
        e = int(np.flatnonzero(last["probe"] >= 0)[0])
        before = env.env_params[:, e].clone()
        env.reset_idx(torch.tensor([e], device="cuda"))
        torch.cuda.synchronize()
        assert int(adr.probe[e]) == -1 and int(adr.reached[e]) == 0 and torch.equal(env.env_params[:, e], before)
        assert int(adr.episode_index[e]) == last["episode_index"][e]
        scalars = adr.scalars()
        ranges = env_params.adr_ranges(SPEC, adr.adr, last["widen"])
        assert all(scalars["adr/%s_lo" % n] == ranges[n][0] and scalars["adr/%s_hi" % n] == ranges[n][1] for n in NAMES)
        path = env.episode_log.path
    finally:
        env.close()
    back = episodes.load_rows_with_params(path)                   # the offline reader rebuilds the same columns, no device
    assert np.array_equal(back["probe"], rows["probe"]) and np.array_equal(back["param_DAMPING"], rows["param_DAMPING"])
    config, history, dropped, widen0, _ = episodes.load_env_adr(path)
    assert config == adr.adr and dropped == 0 and len(history) >= last["cursor"] and not widen0.any()


def test_train_and_play_entries_adr(tmp_path, monkeypatch, caplog):
    """Two training iterations (horizon 8) through train.py's entry point with ADR on: finite scalars, the adr/* scalars among
    them, the adr entry in the checkpoint, configuration and history in the .npz; test=True from that checkpoint logs that ADR
    is off and plays on the full limits."""
    from vine_robot_isaacgymenvs_amd.train import main
    from vine_robot_isaacgymenvs_amd.utils import episodes, tfevents
    monkeypatch.chdir(tmp_path)
    common = ["task=Vine5LinkMovingBase", "num_envs=512", "headless=True", "experiment=adr", "task.env.CREATE_PIPE=False",
              "task.env.maxEpisodeLength=%d" % MAX_LEN, "task.env.SUCCESS_DIST=%g" % SUCCESS_DIST,
              "task.env.ENV_PARAMS_PER_EPISODE=True",
              "task.env.ENV_PARAMS={DAMPING: [0.005, 0.1], ACTION_DELAY: [0, 6], LINK_MASS: [0.7, 1.4], FPAM_K: [0.9, 1.1]}",
              "task.env.ENV_PARAMS_ADR={NAMES: {DAMPING: {START: [0.02, 0.02], STEP: 0.005}, ACTION_DELAY: {START: [1, 1], STEP: 1}, "
              "LINK_MASS: {START: [1.0, 1.0], STEP: 0.05}}, BOUNDARY_FRACTION: 0.25, QUEUE: 8, WIDEN_AT: 0.8, NARROW_AT: 0.4}",
              "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_CAPACITY=32768", "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "train")]
    main(common + ["minibatch_size=2048", "max_iterations=2", "train.params.config.horizon_length=8",
                   "train.params.config.save_frequency=1", "train.params.config.save_best_after=0",
                   "+train.params.config.print_stats=False"])
    torch.cuda.synchronize()
    run = tmp_path / "runs" / "adr"
    (events,) = glob.glob(str(run / "summaries" / "events.out.tfevents.*"))
    scalars = tfevents.read_scalars(events)
    assert all(np.isfinite(v) for _, v, _, _ in scalars)
    tags = {tag for tag, _, _, _ in scalars}
    for name in ("DAMPING", "ACTION_DELAY", "LINK_MASS"):
        assert "adr/%s_lo" % name in tags and "adr/%s_hi" % name in tags, sorted(tags)
    assert "adr/FPAM_K_lo" not in tags
    damping_lo = [v for tag, v, _, _ in scalars if tag == "adr/DAMPING_lo"]
    assert len(damping_lo) == 2 and all(np.float32(0.005) <= np.float32(v) <= np.float32(0.02) for v in damping_lo)      # (stored as float32)
    (npz,) = glob.glob(str(tmp_path / "train" / "*_episodes.npz"))
    config, history, dropped, widen0, _ = episodes.load_env_adr(npz)
    assert list(config["NAMES"]) == ["DAMPING", "ACTION_DELAY", "LINK_MASS"] and config["QUEUE"] == 8 and dropped == 0
    assert not widen0.any()
    rows = episodes.load_rows_with_params(npz)
    assert len(rows["env"]) >= 512 and (rows["probe"] >= 0).any() and (rows["probe"] == -1).any()
    known = rows["probe"] > -2                                    # (a name under ADR has a column once its range is no point)
    k0 = rows["param_FPAM_K"][known] / rows["param_FPAM_K"][known].mean()
    assert known.all() and k0.min() >= 0.9 / 1.1 and k0.max() <= 1.1 / 0.9 and len(np.unique(k0)) > 100
    if "param_DAMPING" in rows:
        assert (rows["param_DAMPING"] >= np.float32(0.005)).all() and (rows["param_DAMPING"] <= np.float32(0.1)).all()
    ckpts = sorted(glob.glob(str(run / "nn" / "*.pth")))
    assert ckpts, "no checkpoint written"
    ckpt = torch.load(ckpts[-1], map_location="cpu", weights_only=False)
    assert ckpt["adr"]["names"] == ["DAMPING", "ACTION_DELAY", "LINK_MASS"] and ckpt["adr"]["widen"].shape == (abi.VR_NAMES, 2)
    # a training resumed from that checkpoint starts from its ranges: with a QUEUE no boundary fills, every adr/* scalar of
    # the resumed run is the checkpoint's, and the resumed run's episode file says where its history starts
    assert ckpt["adr"]["widen"].sum() > 0
    k = [i for i, o in enumerate(common) if o.startswith("task.env.ENV_PARAMS_ADR=")][0]
    resumed = list(common)
    resumed[k] = common[k].replace("QUEUE: 8", "QUEUE: 1000000")
    resumed[3], resumed[-1] = "experiment=adr_resumed", "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "resumed")
    main(resumed + ["minibatch_size=2048", "max_iterations=4", "train.params.config.horizon_length=8", "checkpoint=" + ckpts[-1],
                    "+train.params.config.print_stats=False"])
    torch.cuda.synchronize()
    (events,) = glob.glob(str(tmp_path / "runs" / "adr_resumed" / "summaries" / "events.out.tfevents.*"))
    spec = {"DAMPING": [0.005, 0.1], "ACTION_DELAY": [0, 6], "LINK_MASS": [0.7, 1.4], "FPAM_K": [0.9, 1.1]}
    want = env_params.adr_ranges(spec, config, ckpt["adr"]["widen"])
    seen = [(tag, v) for tag, v, _, _ in tfevents.read_scalars(events) if tag.startswith("adr/") and tag[-3:] in ("_lo", "_hi")]
    assert len(seen) >= 6
    for tag, v in seen:
        assert np.float32(v) == np.float32(want[tag[4:-3]][0 if tag.endswith("_lo") else 1]), tag
    (npz,) = glob.glob(str(tmp_path / "resumed" / "*_episodes.npz"))
    _, history, _, widen0, _ = episodes.load_env_adr(npz)
    assert np.array_equal(widen0, ckpt["adr"]["widen"]) and len(history) == 0
    rows = episodes.load_rows_with_params(npz)
    if "param_DAMPING" in rows:                                   # drawn from the restored range, which is wider than START
        d = rows["param_DAMPING"][rows["episode"] > 0]
        assert d.min() >= np.float32(want["DAMPING"][0]) and d.max() <= np.float32(want["DAMPING"][1])
        assert want["DAMPING"][0] == 0.02 or d.min() < np.float32(0.02)
    common[-1] = "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "play")
    with caplog.at_level(logging.INFO):
        reward, steps = main(common + ["test=True", "checkpoint=" + ckpts[-1], "+train.params.config.player={max_steps: 40}"])
    assert np.isfinite(reward) and steps > 0
    assert any("ENV_PARAMS_ADR is forced off" in r.getMessage() for r in caplog.records)
    (npz,) = glob.glob(str(tmp_path / "play" / "*_episodes.npz"))
    assert episodes.load_env_adr(npz) == (None, None, 0, None, None) and episodes.load_env_redraw(npz)[0] is not None
