"""ENV_DRAW_ADR on the GPU: the two launches of include/vine_env_draw_adr.h alone against utils/env_draw_adr.py
draw_adr_replay, their reduction to the three observers' own draws, behind real steps with all three observers, beside
ENV_PARAMS_ADR, under env_id_offset, in a replayed graph, and through the task class, the episode log and train.py's entry.

The shapes are those of tests/test_env_params_adr_gpu.py: 70 envs = two waves, the second partial; 12-step episodes, 40 steps;
QUEUE 4, BOUNDARY_FRACTION 0.5, HISTORY_CAPACITY 64.  Every comparison is on integers or on 32-bit words."""
import ctypes as C
import glob
import logging

import numpy as np
import pytest
import torch

from tests.test_env_params_adr_gpu import SUCCESS_DIST, SUCCESS_DIST_PIPE, moves_of
from tests.test_env_params_gpu import MAX_LEN, N, T, actions_for
from tests.test_env_sensor_gpu import PAD, case_cfg, guarded, words
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_draw_adr, env_params, env_push, env_sensor, env_target, named_draw

pytestmark = pytest.mark.gpu

# the limits: at least one [lo, hi] name per observer; SENSOR_HOLD and TARGET_SPAN_ALONG are ranges that stay their observer's
SENSOR = {"DELAY": [0, 3], "HOLD": [0.0, 0.2], "NOISE_STD": [0.0, 0.01], "PER_EPISODE": True}
PUSH = {"RATE": 0.2, "IMPULSE": [0.0, 0.01], "PER_EPISODE": True}
TARGET = {"VEL_ALONG": [-0.3, 0.3], "SPAN_ALONG": [0.03, 0.04], "PER_EPISODE": True}
# at most two steps from START to a limit, so that 48 launches get there and back; SENSOR_NOISE_STD starts AT its lower limit
NAMES = {"SENSOR_DELAY": {"START": [1, 1], "STEP": 1}, "SENSOR_NOISE_STD": {"START": [0.0, 0.0], "STEP": 0.005},
         "PUSH_IMPULSE": {"START": [0.002, 0.004], "STEP": 0.004}, "TARGET_VEL_ALONG": {"START": [0.0, 0.0], "STEP": 0.15}}
ADR = {"NAMES": NAMES, "BOUNDARY_FRACTION": 0.5, "QUEUE": 4, "WIDEN_AT": 0.8, "NARROW_AT": 0.4, "HISTORY_CAPACITY": 64}
STATE = ("widen", "counts", "probe", "reached", "episode_index")
SENTINEL = np.float32(-777.25)
MODULES = (env_sensor, env_push, env_target)


def observer_cfgs(cfg, num_obs):
    """The three observers' checked mappings for a handle's configuration."""
    pipe = bool(cfg.flags & abi.FLAG_CREATE_PIPE)
    cdt = np.float32(cfg.dt) * np.float32(cfg.control_freq_inv)
    return (env_sensor.sensor_config({"ENV_SENSOR": SENSOR}, num_obs), env_push.push_config({"ENV_PUSH": PUSH}),
            env_target.target_config({"ENV_TARGET": TARGET, "CREATE_PIPE": pipe}, cdt))


def adr_of(cfgs, **keys):
    return env_draw_adr.draw_adr_config({"ENV_DRAW_ADR": dict(ADR, **keys)}, *cfgs)


def limits_adr(cfgs):
    """START = the limits and nobody probes: the reduction."""
    names = {"SENSOR_DELAY": {"START": [0, 3], "STEP": 1}, "SENSOR_NOISE_STD": {"START": [0.0, 0.01], "STEP": 0.005},
             "PUSH_IMPULSE": {"START": [0.0, 0.01], "STEP": 0.004}, "TARGET_VEL_ALONG": {"START": [-0.3, 0.3], "STEP": 0.15}}
    return adr_of(cfgs, NAMES=names, BOUNDARY_FRACTION=0.0)


def host(snap):
    return {k: ([None if x is None else x.cpu().numpy() for x in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in snap.items()}


def assert_equals_replay(got, want, capacity, what):
    """One snapshot (host arrays) against one step of draw_adr_replay: the integers, the three tables, the history and cursor."""
    for k in STATE:
        assert np.array_equal(got[k].astype(np.int64), want[k]), "%s: %s" % (what, k)
    for g in range(abi.VDA_GROUPS):
        if want["tables"][g] is not None:
            assert np.array_equal(words(got["tables"][g]), words(want["tables"][g])), "%s: the table of %s" % (what, env_draw_adr.GROUPS[g])
    assert int(got["cursor"][0]) == want["cursor"] <= capacity, what
    assert np.array_equal(got["history"][:want["cursor"]].astype(np.int64), want["history"]), "%s: history rows" % what
    assert not got["history"][want["cursor"]:].any(), "%s: the ring beyond the cursor" % what


class Rig:
    """A handle with the three observers behind its steps (their launch order: target, sensor, push) and, with ``adr``, the
    ENV_DRAW_ADR observer behind them."""

    def __init__(self, cfg, adr=None, observers=True):
        from tests.hip_env import HipEnv
        if not torch.cuda.is_available():
            pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
        self.env = env = HipEnv(cfg)
        env.bind_reward_matrix()
        self.cfgs = observer_cfgs(env.cfg, env.num_obs)
        self.gids = np.arange(env.n, dtype=np.int64) + int(env.cfg.env_id_offset)
        self.seed = int(env.cfg.seed)
        self.sensor = self.push = self.target = self.draw = None
        if observers:
            self.target = env_target.EnvTarget(env.lib, env.h, env.cfg, self.cfgs[2], env.reset_t, env.progress_t, env.n, env.num_obs, env.dev)
            self.sensor = env_sensor.EnvSensor(env.lib, env.h, env.cfg, self.cfgs[0], env.reset_t, env.progress_t, env.n, env.num_obs, env.dev)
            self.push = env_push.EnvPush(env.lib, env.h, env.cfg, self.cfgs[1], env.reset_t, env.n, env.dev)
        self.adr = adr(self.cfgs) if callable(adr) else adr
        if self.adr is not None:
            self.draw = env_draw_adr.EnvDrawAdr(env.lib, env.h, env.cfg, self.adr, env.reset_t, self.sensor, self.push, self.target, env.dev)
        torch.cuda.synchronize(env.dev)
        self.tables0 = [o.table.cpu().numpy() for o in (self.sensor, self.push, self.target)] if observers else None

    def behind(self):
        """The observers' launches behind the step just enqueued."""
        env, stream = self.env, torch.cuda.current_stream(self.env.dev).cuda_stream
        self.target.enqueue(stream, None, obs=env.obs_t.data_ptr())
        self.sensor.enqueue(stream, None, obs=env.obs_t.data_ptr())
        self.push.enqueue(stream)
        if self.draw is not None:
            self.draw.enqueue(stream)

    def snapshot(self):
        d = self.draw
        out = {"tables": [o.table.clone() for o in (self.sensor, self.push, self.target)]}
        if d is not None:
            out.update(widen=d.widen.clone(), counts=d.counts.clone(), probe=d.probe.clone(), reached=d.reached.clone(),
                       episode_index=d.episode_index.clone(), history=d.history.clone(), cursor=d.cursor.clone())
        return out

    def run(self, actions, extra=None):
        env = self.env
        keys = ("obs", "rew", "reset", "progress", "timeouts", "state")
        rec = {k: [] for k in keys + ("reach", "snap")}
        for a in actions:
            env.step_t(a.to(env.dev).contiguous(), sync=False)
            rec["reach"].append(env.reward_matrix_t[:, 2].clone())      # what the launches behind this step see
            rec["reset"].append(env.reset_t.clone())
            self.behind()
            if extra is not None:
                extra()
            for k in keys:
                if k != "reset":
                    rec[k].append(getattr(env, k + "_t").clone())
            rec["snap"].append(self.snapshot())
        torch.cuda.synchronize(env.dev)
        out = {k: torch.stack(rec[k]).cpu().numpy() for k in keys + ("reach",)}
        out["snap"] = [host(s) for s in rec["snap"]]
        return out

    def replay(self, resets, reach, **keys):
        return env_draw_adr.draw_adr_replay(self.adr, self.seed, self.gids, resets, reach, self.tables0, self.cfgs, **keys)

    def close(self):
        self.env.close()


def step_cfg(case):
    cfg = case_cfg("pipe" if case == "pipe" else "free", N, 1000 if case == "offset" else 0)
    cfg.success_dist = SUCCESS_DIST_PIPE if case == "pipe" else SUCCESS_DIST
    return cfg


# ------------------------------------------------------------------------------------------------------- the pair alone
def test_pair_alone_equals_the_replay_after_every_launch():
    """48 launch pairs on hand-set flags: two thirds of the envs flagged per launch, the first and the last lane and both
    sides of the wave boundary among them in turn; reward column 2 written by the test: all ones for 24 launches, then all
    zeros.  Every buffer lies between sentinels.  After EVERY launch all state and the three tables equal draw_adr_replay; the
    unflagged columns, the rows not under ADR and the state block are untouched; the history shows a widening, a narrowing, a
    stop at a limit and a stop at START."""
    launches = 48
    rig = Rig(step_cfg("free"), observers=False)
    env, lib = rig.env, rig.env.lib
    adr = adr_of(rig.cfgs)
    specs = (env_sensor.sensor_spec(lib, env.cfg, rig.cfgs[0]), env_push.push_spec(lib, env.cfg, rig.cfgs[1]),
             env_target.target_spec(lib, env.cfg, rig.cfgs[2]))
    aspec = env_draw_adr.draw_adr_spec(lib, env.cfg, adr, *specs)
    guards, buf = {}, {}
    shapes = [("table0", (abi.VSN_NAMES, N), torch.float32, 0), ("table1", (abi.VPU_NAMES, N), torch.float32, 0),
              ("table2", (abi.VTG_NAMES, N), torch.float32, 0), ("widen", (abi.VDA_NAMES, 2), torch.int32, 0),
              ("counts", (abi.VDA_NAMES, 2, 2), torch.int32, 0), ("reached", (N,), torch.int32, 0), ("probe", (N,), torch.int32, -1),
              ("episode_index", (N,), torch.int32, 0), ("history", (64, 4), torch.int32, 0)]
    for name, shape, dtype, fill in shapes:
        whole, view, sentinel = guarded(shape, dtype, env.dev, fill)
        guards[name], buf[name] = (whole, sentinel), view
    buf["cursor"] = torch.zeros(1, dtype=torch.int64, device=env.dev)
    tables0 = [np.full(tuple(buf["table%d" % g].shape), SENTINEL, dtype=np.float32) for g in range(3)]      # rows not under ADR: a sentinel
    for name, row in env_draw_adr.start_rows(adr, rig.seed, rig.gids).items():
        g, r, _ = env_draw_adr.place_of(name)
        tables0[g][r] = row
    for g in range(3):
        buf["table%d" % g].copy_(torch.as_tensor(tables0[g]))
    flags = np.zeros((launches, N), dtype=np.int64)
    for t in range(launches):
        flags[t] = (np.arange(N) + t) % 3 != 0
        flags[t, [0, 63, 64, N - 1]] = [t % 2, (t + 1) % 2, t % 2, (t // 2) % 2]
    reach = np.zeros((launches, N), dtype=np.int64)
    reach[:24] = 1
    reach[:, 5] = 0                                               # one env never reaches, one always
    reach[:, 66] = 1
    want = env_draw_adr.draw_adr_replay(adr, rig.seed, rig.gids, flags, reach, tables0, step_index=np.full(launches, -1))
    rng = np.random.default_rng(0)
    state0 = rng.uniform(-1.0, 1.0, (abi.VF_COUNT, N)).astype(np.float32)
    env.state_t.copy_(torch.as_tensor(state0))
    rm0 = rng.uniform(-1.0, 1.0, (N, abi.NUM_REWARDS)).astype(np.float32)
    tables = (C.c_void_p * 3)(*[buf["table%d" % g].data_ptr() for g in range(3)])
    args = [env.h, aspec, env.reset_t.data_ptr(), tables, None] + [buf[k].data_ptr() for k in ("widen", "counts", "reached", "probe",
                                                                                                "episode_index", "history", "cursor")]
    under = {(g, r) for g, r, _ in map(env_draw_adr.place_of, adr["NAMES"])}
    for t in range(launches):
        rm0[:, 2] = reach[t]
        env.reward_matrix_t.copy_(torch.as_tensor(rm0))
        env.reset_t.copy_(torch.as_tensor(flags[t]))
        before = [buf["table%d" % g].cpu().numpy() for g in range(3)]
        assert lib.vine_env_draw_adr_scheduled(*(args + [torch.cuda.current_stream(env.dev).cuda_stream])) == abi.OK
        torch.cuda.synchronize()
        got = {k: buf[k].cpu().numpy() for k in STATE + ("history", "cursor")}
        got["tables"] = [buf["table%d" % g].cpu().numpy() for g in range(3)]
        assert_equals_replay(got, want[t], 64, "launch %d" % t)
        clear = np.flatnonzero(flags[t] == 0)
        for g in range(3):
            assert np.array_equal(words(got["tables"][g][:, clear]), words(before[g][:, clear])), "unflagged columns, launch %d" % t
            for r in range(got["tables"][g].shape[0]):
                if (g, r) not in under:
                    assert (got["tables"][g][r] == SENTINEL).all(), "a row that is not under ADR, launch %d" % t
        assert np.array_equal(words(env.state_t), words(state0)), "the state block, launch %d" % t
        assert np.array_equal(words(env.reward_matrix_t), words(rm0)) and np.array_equal(env.reset_t.cpu().numpy(), flags[t])
    for name, (whole, sentinel) in guards.items():
        w = whole.cpu().numpy()
        assert (w[:PAD] == sentinel).all() and (w[-PAD:] == sentinel).all(), name
    assert want[-1]["cursor"] >= 8
    assert moves_of(want[-1]["history"], env_draw_adr.draw_adr_max_widen(adr)) == {"widen", "narrow", "limit", "start"}
    assert not want[-1]["widen"].any() and want[23]["widen"].sum() >= 8      # there and back
    probes = np.concatenate([w["probe"] for w in want])
    assert set(probes.tolist()) == {-1} | {2 * env_draw_adr.NAMES.index(n) + s for n in NAMES for s in (0, 1)}
    # a probing episode's value is exactly its boundary, SENSOR_DELAY's at both integer ends among them
    delay_probes = {(int(w["probe"][e]), float(w["tables"][0][0, e])) for w in want for e in np.flatnonzero((w["probe"] == 0) | (w["probe"] == 1))}
    assert (0, 0.0) in delay_probes and (1, 3.0) in delay_probes
    rig.close()


def test_refusals_on_a_handle():
    rig = Rig(step_cfg("free"), adr=adr_of)
    env, lib, d = rig.env, rig.env.lib, rig.draw
    stream = torch.cuda.current_stream(env.dev).cuda_stream
    args = [env.h, d.aspec, env.reset_t.data_ptr(), d.tables, None, d.widen.data_ptr(), d.counts.data_ptr(), d.reached.data_ptr(),
            d.probe.data_ptr(), d.episode_index.data_ptr(), d.history.data_ptr(), d.cursor.data_ptr(), stream]
    assert lib.vine_env_draw_adr_scheduled(*args) == abi.OK
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11):
        bad = list(args)
        bad[k] = None
        assert lib.vine_env_draw_adr_scheduled(*bad) == abi.ERR_INVALID_ARG and b"null argument" in lib.vine_last_error(), k
    for g in range(3):                                            # every group has a name under ADR: its table is needed
        bad = list(args)
        bad[3] = (C.c_void_p * 3)(*[None if j == g else d.tables[j] for j in range(3)])
        assert lib.vine_env_draw_adr_scheduled(*bad) == abi.ERR_INVALID_ARG
        assert b"null argument" in lib.vine_last_error() and env_draw_adr.GROUPS[g].encode() in lib.vine_last_error()
    for change, text in ((dict(checked=0), b"not filled by vine_env_draw_adr_spec"), (dict(abi_version=7), b"abi_version mismatch"),
                         (dict(num_adr=0), b"lies outside what vine_env_draw_adr_spec fills")):
        spec = abi.VineEnvDrawAdrSpec.from_buffer_copy(d.aspec)
        for k, v in change.items():
            setattr(spec, k, v)
        bad = list(args)
        bad[1] = spec
        assert lib.vine_env_draw_adr_scheduled(*bad) == abi.ERR_INVALID_ARG and text in lib.vine_last_error(), change
    native.check(lib.vine_bind_reward_matrix(env.h, None), lib)
    assert lib.vine_env_draw_adr_scheduled(*args) == abi.ERR_INVALID_ARG and b"needs a reward matrix" in lib.vine_last_error()
    torch.cuda.synchronize()
    rig.close()


# ----------------------------------------------------------------------------------------------------- the reduction
@pytest.mark.parametrize("case", ["free", "pipe"])
def test_start_at_the_limits_and_no_probe_is_the_run_without_the_key(case):
    """START = the limits and BOUNDARY_FRACTION 0 behind 40 real steps: the three tables, the observation, the state block and
    the step's buffers after every step are those of the same run without the observer, bit for bit."""
    acts = actions_for(N, T)
    a, b = Rig(step_cfg(case), adr=limits_adr), Rig(step_cfg(case))
    for g in range(3):
        assert np.array_equal(words(a.tables0[g]), words(b.tables0[g])), "episode 0 from START = the limits is the observer's own draw"
    ra, rb = a.run(acts), b.run(acts)
    for k in ("obs", "rew", "reset", "progress", "timeouts", "state"):
        assert np.array_equal(words(ra[k]), words(rb[k])), (case, k)
    for t in range(T):
        for g in range(3):
            assert np.array_equal(words(ra["snap"][t]["tables"][g]), words(rb["snap"][t]["tables"][g])), (case, t, g)
    last = ra["snap"][-1]
    assert not last["widen"].any() and not last["counts"].any() and (last["probe"] == -1).all() and int(last["cursor"][0]) == 0
    assert np.array_equal(last["episode_index"], a.sensor.episode_index.cpu().numpy()) and last["episode_index"].max() >= 2
    assert len(np.unique(last["tables"][2][abi.VTG_VEL_ALONG])) > N // 2 and ra["reset"].sum() > N
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- behind real steps
def probing_outcomes(replay, resets, reach):
    hit = miss = 0
    for t in range(1, len(replay)):
        done = (resets[t] != 0) & (replay[t - 1]["probe"] >= 0)
        ever = (replay[t - 1]["reached"] != 0) | (reach[t] != 0)
        hit += int(np.count_nonzero(done & ever))
        miss += int(np.count_nonzero(done & ~ever))
    return hit, miss


@pytest.mark.parametrize("case", ["free", "pipe", "offset"])
def test_pair_behind_every_step_equals_the_replay(case):
    """All three observers and the pair behind each of 40 real steps; the device's reset buffer and reward column 2 of every
    step go to draw_adr_replay, and all state and the three tables after every step equal the replay's.  The episode ordinals
    are the three observers' own; every value lies in the range in force when it was drawn."""
    rig = Rig(step_cfg(case), adr=adr_of)
    ra = rig.run(actions_for(N, T))
    replay = rig.replay(ra["reset"], ra["reach"] != 0)
    for t in range(T):
        assert_equals_replay(ra["snap"][t], replay[t], 64, "%s, step %d" % (case, t))
    hit, miss = probing_outcomes(replay, ra["reset"], ra["reach"])
    print("%s: %d probing episodes reached, %d did not; %d history rows" % (case, hit, miss, replay[-1]["cursor"]))
    assert hit + miss > 0 and ra["reset"].sum() > N and replay[-1]["episode_index"].max() >= 2
    for o in (rig.sensor, rig.push, rig.target):
        assert np.array_equal(o.episode_index.cpu().numpy(), replay[-1]["episode_index"])
    limits = rig.adr["LIMITS"]
    for name in NAMES:
        g, r, _ = env_draw_adr.place_of(name)
        row = replay[-1]["tables"][g][r]
        assert row.min() >= np.float32(limits[name][0]) and row.max() <= np.float32(limits[name][1]), name
    assert rig.gids[0] == (1000 if case == "offset" else 0)
    rig.close()


def test_beside_env_params_adr_each_equals_its_own_replay():
    """ENV_PARAMS_ADR on the same handle, last in launch order: each pair's state equals its own replay of the same flags, and
    the two probe draws differ (their keys do)."""
    from tests.test_env_params_adr_gpu import ADR as PLANT_ADR, SPEC as PLANT_SPEC
    from vine_robot_isaacgymenvs_amd.utils import env_adr
    rig = Rig(step_cfg("free"), adr=adr_of)
    env = rig.env
    plant = env_params.adr_config({"ENV_PARAMS": PLANT_SPEC, "ENV_PARAMS_PER_EPISODE": True, "ENV_PARAMS_ADR": PLANT_ADR})
    start = env_params.adr_start_spec(PLANT_SPEC, plant)
    table = torch.as_tensor(env_params.build_table(start, env.cfg, rig.seed, N, 0, lib=env.lib)).to(env.dev)
    inertia = torch.as_tensor(env_params.build_inertia_table(start, env.cfg, rig.seed, N, 0, lib=env.lib)).to(env.dev)
    torch.cuda.synchronize()
    native.check(env.lib.vine_bind_env_params(env.h, table.data_ptr()), env.lib)
    native.check(env.lib.vine_bind_env_inertia(env.h, inertia.data_ptr()), env.lib)
    other = env_adr.EnvAdr(env.lib, env.h, env.cfg, PLANT_SPEC, plant, env.reset_t, table, inertia, env.dev)
    ra = rig.run(actions_for(N, T), extra=lambda: other.enqueue(torch.cuda.current_stream(env.dev).cuda_stream))
    replay = rig.replay(ra["reset"], ra["reach"] != 0)
    for t in range(T):
        assert_equals_replay(ra["snap"][t], replay[t], 64, "beside ENV_PARAMS_ADR, step %d" % t)
    want = env_params.adr_replay(PLANT_SPEC, plant, rig.seed, rig.gids, ra["reset"], ra["reach"] != 0, env.cfg, lib=env.lib)[-1]
    for k, t in (("widen", other.widen), ("counts", other.counts), ("probe", other.probe), ("reached", other.reached),
                 ("episode_index", other.episode_index)):
        assert np.array_equal(t.cpu().numpy().astype(np.int64), want[k]), k
    assert np.array_equal(words(table), words(want["params"])) and np.array_equal(words(inertia), words(want["inertia"]))
    assert np.array_equal(want["episode_index"], replay[-1]["episode_index"])
    assert not np.array_equal(want["probe"] >= 0, replay[-1]["probe"] >= 0)      # the two pick independently
    rig.close()


# ------------------------------------------------------------------------------------------------------------- replay
def test_captured_step_and_observer_groups_replay_like_eager_launches():
    """Four (step + the observers' launches + the pair) groups captured once and replayed ten times against the same 40
    groups launched eagerly."""
    acts = actions_for(N, T).cuda()
    eager = Rig(step_cfg("free"), adr=adr_of)
    for k in range(T):
        eager.env.step_t(acts[k].contiguous(), sync=False)
        eager.behind()
    torch.cuda.synchronize()
    g = Rig(step_cfg("free"), adr=adr_of)
    a_in = torch.zeros(4, N, 2, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for k in range(4):
            g.env.step_t(a_in[k], sync=False)
            g.behind()
    for r in range(10):
        a_in.copy_(acts[4 * r:4 * r + 4])
        graph.replay()
    torch.cuda.synchronize()
    assert g.env.step_count == eager.env.step_count == T
    for name in ("state_t", "obs_t", "rew_t", "reset_t", "progress_t", "timeouts_t"):
        assert np.array_equal(words(getattr(g.env, name)), words(getattr(eager.env, name))), name
    sa, sb = host(g.snapshot()), host(eager.snapshot())
    for k in STATE + ("history", "cursor"):
        assert np.array_equal(sa[k], sb[k]), k
    for t in range(3):
        assert np.array_equal(words(sa["tables"][t]), words(sb["tables"][t])), t
    assert sb["episode_index"].max() >= 2 and int(sb["cursor"][0]) >= 1 and (sb["probe"] >= 0).sum() > 0
    eager.close()
    g.close()


# ----------------------------------------------------------------------------------------------------- the task class
def make_env(tmp_path, extra=()):
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_config(overrides=["num_envs=%d" % N, "task.env.CREATE_PIPE=False", "task.env.maxEpisodeLength=%d" % MAX_LEN,
                                 "task.env.SUCCESS_DIST=%g" % SUCCESS_DIST, "task.env.EPISODE_LOG=True",
                                 "task.env.EPISODE_LOG_DIR=" + str(tmp_path)] + list(extra))
    cfg["task"]["seed"] = 42
    cfg["task"]["env"].update(ENV_SENSOR=SENSOR, ENV_PUSH=PUSH, ENV_TARGET=TARGET, ENV_DRAW_ADR=ADR)
    return isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                  headless=True)


def test_task_class_counts_the_log_rows_and_every_row_has_the_replays_values(tmp_path):
    """40 steps through the task class with EPISODE_LOG: the observer stands behind the target, the sensor and the push; its
    state equals the replay of the recorded flags; per boundary, counts plus what decisions consumed = the number (and the
    reached_ever sum) of the log rows with that draw_probe; every row's param_* of a name under ADR is the replay's value of that
    episode; an env reset from outside keeps its values and is not counted."""
    from vine_robot_isaacgymenvs_amd.utils import episodes
    env = make_env(tmp_path)
    try:
        d = env.env_draw_adr
        assert isinstance(d, env_draw_adr.EnvDrawAdr)
        assert [type(o).__name__ for o in env.observers] == ["EpisodeLog", "EnvTarget", "EnvSensor", "EnvPush", "EnvDrawAdr"]
        live = {t.data_ptr() for t in d.live_tensors()}
        for t in (d.widen, d.reached, d.probe, d.episode_index, d.cursor):
            assert t.data_ptr() in live
        assert d.counts.data_ptr() == d.widen.data_ptr() + 4 * d.widen.numel()      # (one block: widen, then counts)
        cfgs = (env.env_sensor.spec, env.env_push.spec, env.env_target.spec)
        tables0 = [o.table.cpu().numpy() for o in (env.env_sensor, env.env_push, env.env_target)]
        gids = np.arange(N)
        for name, row in env_draw_adr.start_rows(d.adr, 42, gids).items():      # episode 0 is the host's, from START
            g, r, _ = env_draw_adr.place_of(name)
            assert np.array_equal(words(tables0[g][r]), words(row)), name
        acts = actions_for(N, T, seed=7).cuda()
        obs = torch.zeros(N, env.num_obs, device="cuda")
        resets, reach = [], []
        for k in range(T):
            env.step_into(acts[k], obs)
            resets.append(env.reset_buf.cpu().numpy().copy())
            reach.append(env._reward_matrix[:, 2].cpu().numpy() != 0)
        resets = np.array(resets)
        replay = env_draw_adr.draw_adr_replay(d.adr, 42, gids, resets, reach, tables0, cfgs)
        last = replay[-1]
        got = {"widen": d.widen, "counts": d.counts, "probe": d.probe, "reached": d.reached, "episode_index": d.episode_index,
               "history": d.history, "cursor": d.cursor, "tables": [env.env_sensor.table, env.env_push.table, env.env_target.table]}
        assert_equals_replay(host(got), last, d.capacity, "the task class")
        env.episode_log.harvest()
        assert np.array_equal(d.history_rows, last["history"]) and last["cursor"] >= 1
        rows = env.episode_log.rows_with_params()
        assert env.episode_log.unknown_draws == 0 and len(rows["env"]) == resets.sum()
        probing = rows["draw_probe"] >= 0
        counted = d.counts.cpu().numpy().astype(np.int64) + last["consumed"]
        assert last["consumed"].sum() > 0
        per_boundary = np.bincount(rows["draw_probe"][probing], minlength=2 * abi.VDA_NAMES).reshape(abi.VDA_NAMES, 2)
        hit = np.bincount(rows["draw_probe"][probing], weights=rows["reached_ever"][probing], minlength=2 * abi.VDA_NAMES).reshape(abi.VDA_NAMES, 2)
        assert np.array_equal(counted[..., 0], per_boundary) and np.array_equal(counted[..., 1], hit.astype(np.int64))
        assert per_boundary.sum() > 0
        at = episodes.drawn_at(rows["env"], rows["episode"], rows["end_step"])
        for r in range(len(rows["env"])):
            e = rows["env"][r]
            tables = replay[at[r]]["tables"] if rows["episode"][r] else tables0
            for name in NAMES:
                g, row, _ = env_draw_adr.place_of(name)
                assert rows["param_" + name][r] == tables[g][row, e], (r, name)
            assert rows["param_SENSOR_HOLD"][r] == tables[0][abi.VSN_HOLD, e]      # not under ADR: the observer's own draw
            assert rows["draw_probe"][r] == (replay[at[r]]["probe"][e] if rows["episode"][r] else -1)
        e = int(np.flatnonzero(last["probe"] >= 0)[0])
        before = [o.table[:, e].clone() for o in (env.env_sensor, env.env_push, env.env_target)]
        env.reset_idx(torch.tensor([e], device="cuda"))
        torch.cuda.synchronize()
        assert int(d.probe[e]) == -1 and int(d.reached[e]) == 0 and int(d.episode_index[e]) == last["episode_index"][e]
        assert all(torch.equal(o.table[:, e], b) for o, b in zip((env.env_sensor, env.env_push, env.env_target), before))
        scalars = d.scalars()
        ranges = env_draw_adr.draw_adr_ranges(d.adr, last["widen"])
        assert all(scalars["draw_adr/%s_lo" % n] == ranges[n][0] and scalars["draw_adr/%s_hi" % n] == ranges[n][1] for n in NAMES)
        path = env.episode_log.path
    finally:
        env.close()
    back = episodes.load_rows_with_params(path)                   # the offline reader rebuilds the same columns, no device
    assert np.array_equal(back["draw_probe"], rows["draw_probe"])
    for name in NAMES:
        assert np.array_equal(back["param_" + name], rows["param_" + name]), name
    config, history, dropped, widen0, _ = episodes.load_env_draw_adr(path)
    assert config == d.adr and dropped == 0 and len(history) >= last["cursor"] and not widen0.any()


def test_the_key_off_constructs_nothing(tmp_path):
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_config(overrides=["num_envs=%d" % N, "task.env.CREATE_PIPE=False"])
    cfg["task"]["env"].update(ENV_SENSOR=SENSOR, ENV_PUSH=PUSH, ENV_TARGET=TARGET)
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0, headless=True)
    try:
        assert env.env_draw_adr is None and [type(o).__name__ for o in env.observers] == ["EnvTarget", "EnvSensor", "EnvPush"]
    finally:
        env.close()


def test_train_resume_and_play_entries(tmp_path, monkeypatch, caplog):
    """Two training iterations (horizon 8) through train.py's entry with the key on: finite scalars, the draw_adr/* scalars among
    them, the draw_adr entry in the checkpoint, configuration and history in the .npz; a training resumed from that checkpoint
    starts from its ranges (every draw_adr/* scalar equals the checkpoint's ranges); test=True logs that the key is forced off."""
    from vine_robot_isaacgymenvs_amd.train import main
    from vine_robot_isaacgymenvs_amd.utils import episodes, tfevents
    monkeypatch.chdir(tmp_path)
    common = ["task=Vine5LinkMovingBase", "num_envs=512", "headless=True", "experiment=draw_adr", "task.env.CREATE_PIPE=False",
              "task.env.maxEpisodeLength=%d" % MAX_LEN, "task.env.SUCCESS_DIST=0.8",      # (nearly every episode reaches: the ranges widen)
              "task.env.ENV_SENSOR={DELAY: [0, 3], NOISE_STD: [0.0, 0.01], PER_EPISODE: True}",
              "task.env.ENV_PUSH={RATE: 0.05, IMPULSE: [0.0, 0.01], PER_EPISODE: True}",
              "task.env.ENV_TARGET={VEL_ALONG: [-0.3, 0.3], SPAN_ALONG: 0.05, PER_EPISODE: True}",
              "task.env.ENV_DRAW_ADR={NAMES: {SENSOR_DELAY: {START: [0, 0], STEP: 1}, PUSH_IMPULSE: {START: [0, 0], STEP: 0.002}, "
              "TARGET_VEL_ALONG: {START: [0, 0], STEP: 0.05}}, BOUNDARY_FRACTION: 0.25, QUEUE: 8, WIDEN_AT: 0.8, NARROW_AT: 0.4}",
              "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_CAPACITY=32768", "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "train")]
    main(common + ["minibatch_size=2048", "max_iterations=2", "train.params.config.horizon_length=8",
                   "train.params.config.save_frequency=1", "train.params.config.save_best_after=0",
                   "+train.params.config.print_stats=False"])
    torch.cuda.synchronize()
    run = tmp_path / "runs" / "draw_adr"
    (events,) = glob.glob(str(run / "summaries" / "events.out.tfevents.*"))
    scalars = tfevents.read_scalars(events)
    assert all(np.isfinite(v) for _, v, _, _ in scalars)
    tags = {tag for tag, _, _, _ in scalars}
    for name in ("SENSOR_DELAY", "PUSH_IMPULSE", "TARGET_VEL_ALONG"):
        assert "draw_adr/%s_lo" % name in tags and "draw_adr/%s_hi" % name in tags, sorted(tags)
    assert "draw_adr/SENSOR_NOISE_STD_lo" not in tags and not any(t.startswith("adr/") for t in tags)
    hi = [v for tag, v, _, _ in scalars if tag == "draw_adr/TARGET_VEL_ALONG_hi"]
    assert len(hi) == 2 and all(np.float32(0.0) <= np.float32(v) <= np.float32(0.3) for v in hi)
    (npz,) = glob.glob(str(tmp_path / "train" / "*_episodes.npz"))
    config, history, dropped, widen0, _ = episodes.load_env_draw_adr(npz)
    assert list(config["NAMES"]) == ["SENSOR_DELAY", "PUSH_IMPULSE", "TARGET_VEL_ALONG"] and config["QUEUE"] == 8 and dropped == 0
    assert not widen0.any()
    rows = episodes.load_rows_with_params(npz)
    assert len(rows["env"]) >= 512 and (rows["draw_probe"] >= 0).any() and (rows["draw_probe"] == -1).any() and (rows["draw_probe"] > -2).all()
    assert (rows["param_TARGET_VEL_ALONG"] >= np.float32(-0.3)).all() and (rows["param_TARGET_VEL_ALONG"] <= np.float32(0.3)).all()
    assert (rows["param_TARGET_VEL_ALONG"][rows["episode"] == 0] == 0.0).all()      # episode 0 is START's
    assert len(np.unique(rows["param_SENSOR_NOISE_STD"])) > 100                      # not under ADR: drawn from its whole range
    ckpts = sorted(glob.glob(str(run / "nn" / "*.pth")))
    assert ckpts, "no checkpoint written"
    ckpt = torch.load(ckpts[-1], map_location="cpu", weights_only=False)
    assert ckpt["draw_adr"]["names"] == ["SENSOR_DELAY", "PUSH_IMPULSE", "TARGET_VEL_ALONG"] and ckpt["draw_adr"]["widen"].shape == (abi.VDA_NAMES, 2)
    assert "adr" not in ckpt and ckpt["draw_adr"]["widen"].sum() > 0
    # resumed with a QUEUE no boundary fills: every draw_adr/* scalar of the resumed run is the checkpoint's
    k = [i for i, o in enumerate(common) if o.startswith("task.env.ENV_DRAW_ADR=")][0]
    resumed = list(common)
    resumed[k] = common[k].replace("QUEUE: 8", "QUEUE: 1000000")
    resumed[3], resumed[-1] = "experiment=draw_adr_resumed", "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "resumed")
    main(resumed + ["minibatch_size=2048", "max_iterations=4", "train.params.config.horizon_length=8", "checkpoint=" + ckpts[-1],
                    "+train.params.config.print_stats=False"])
    torch.cuda.synchronize()
    (events,) = glob.glob(str(tmp_path / "runs" / "draw_adr_resumed" / "summaries" / "events.out.tfevents.*"))
    want = env_draw_adr.draw_adr_ranges(config, ckpt["draw_adr"]["widen"])
    seen = [(tag, v) for tag, v, _, _ in tfevents.read_scalars(events) if tag.startswith("draw_adr/") and tag[-3:] in ("_lo", "_hi")]
    assert len(seen) >= 6
    for tag, v in seen:
        assert np.float32(v) == np.float32(want[tag[len("draw_adr/"):-3]][0 if tag.endswith("_lo") else 1]), tag
    (npz,) = glob.glob(str(tmp_path / "resumed" / "*_episodes.npz"))
    _, history, _, widen0, _ = episodes.load_env_draw_adr(npz)
    assert np.array_equal(widen0, ckpt["draw_adr"]["widen"]) and len(history) == 0
    # a checkpoint that does not fit is refused before the first step
    misfit = dict(ckpt, draw_adr={"widen": np.full((abi.VDA_NAMES, 2), 99, dtype=np.int64), "names": ckpt["draw_adr"]["names"]})
    torch.save(misfit, str(tmp_path / "misfit.pth"))
    with pytest.raises(ValueError, match="ENV_DRAW_ADR: the checkpoint's widen does not fit"):
        main(resumed + ["minibatch_size=2048", "max_iterations=3", "train.params.config.horizon_length=8",
                        "checkpoint=" + str(tmp_path / "misfit.pth"), "+train.params.config.print_stats=False"])
    common[-1] = "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "play")
    with caplog.at_level(logging.INFO):
        reward, steps = main(common + ["test=True", "checkpoint=" + ckpts[-1], "+train.params.config.player={max_steps: 40}"])
    assert np.isfinite(reward) and steps > 0
    assert any("ENV_DRAW_ADR is forced off" in r.getMessage() for r in caplog.records)
    (npz,) = glob.glob(str(tmp_path / "play" / "*_episodes.npz"))
    assert episodes.load_env_draw_adr(npz) == (None, None, 0, None, None)
