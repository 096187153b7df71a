"""ENV_TARGET on the GPU: the launch of include/vine_env_target.h alone (free space, shelf, pipe), behind real steps, under
env_id_offset, in a replayed graph, through the task class (every step entry, with the sensor, the push and the per-episode
redraw on, reset_idx, the episode log) and through train.py's entries -- each against utils/env_target.py target_replay.

The shapes are those of tests/test_env_push_gpu.py: 70 envs = two waves, the second partial, in one workgroup that is not
full; 12-step episodes, 40 steps.  "Bit for bit" is literal: float tensors are compared as 32-bit words.  The one statement
numpy does not reproduce in every bit is the pipe's sincosf: the replay is handed the device's AXIS rows, and those are held
to POS_ULPS ulps of 1 against float64 cos / sin of the stored angle."""
import ctypes as C
import glob

import numpy as np
import pytest
import torch

from tests.test_env_params_gpu import MAX_LEN, N, T, actions_for, assert_bit_equal, saw_resets_and_timeouts
from tests.test_env_sensor_gpu import PAD, case_cfg, guarded, hand_flags, words
from tests.test_trajectory_gpu import POS_ULPS
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_target

pytestmark = pytest.mark.gpu

F = abi
f32 = np.float32
R_PIPE = 0.0735                              # PIPE_RADIUS = 0.07 * 1.05 (the step's task_obstacle_poses)
STATE = ("table", "motion", "fresh", "episode_index")
WRITTEN = {F.TARGET_FREE: (F.VF_TARGET_Y, F.VF_TARGET_Z), F.TARGET_SHELF: (F.VF_TARGET_Y, F.VF_OBJ_DEPTH),
           F.TARGET_PIPE: (F.VF_TARGET_Y, F.VF_TARGET_Z, F.VF_OBJ_DEPTH)}
# value lists with zero and both signs; 0.4 m/s * cdt = 0.0133 m a step over a path of +-0.03 m: a reflection every few steps
SPECS = {"free": dict(VEL_ALONG={"values": [0.0, 0.4, -0.4]}, VEL_ACROSS={"values": [0.0, 0.25, -0.3]}, SPAN_ALONG=0.03, SPAN_ACROSS=[0.02, 0.03],
                      PER_EPISODE=True),
         "shelf": dict(VEL_ALONG={"values": [0.0, 0.4, -0.4]}, SPAN_ALONG=[0.02, 0.03], PER_EPISODE=True),
         "pipe": dict(VEL_ALONG={"values": [0.0, 0.4, -0.4]}, SPAN_ALONG={"values": [0.03, 0.02]}, PER_EPISODE=True)}
RESTING = dict(VEL_ALONG=0.0, PER_EPISODE=True)


def mode_name(cfg):
    return "pipe" if cfg.flags & abi.FLAG_CREATE_PIPE else "shelf" if cfg.flags & abi.FLAG_CREATE_SHELF else "free"


def config_for(cfg, keys):
    env = {"ENV_TARGET": dict(keys), "CREATE_SHELF": mode_name(cfg) == "shelf", "CREATE_PIPE": mode_name(cfg) == "pipe"}
    return env_target.target_config(env, f32(cfg.dt) * f32(cfg.control_freq_inv))


def shelf_cfg(n=N):
    from tests.helpers import f6_cfg
    cfg = f6_cfg(n, 1, 0, "shelf")
    cfg.max_episode_length, cfg.seed = MAX_LEN, 25
    return cfg


def cfg_of(case, n=N, offset=0):
    if case == "shelf":
        cfg = shelf_cfg(n)
        cfg.env_id_offset = offset
        return cfg
    return case_cfg(case, n, offset)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=f32))).astype(np.float64)


@pytest.fixture(scope="module")
def Moved():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    from tests.hip_env import HipEnv as H

    def init(self, cfg, device_id=0):
        """HipEnv's set-up with the state block and the observation between sentinels."""
        self.lib = native.load()
        cfg = type(cfg).from_buffer_copy(cfg)
        cfg.set_flag(abi.FLAG_INTROSPECT, True)
        self.cfg, self.n, self.dev = cfg, cfg.num_envs, torch.device("cuda", device_id)
        self.num_obs = self.lib.vine_num_obs(C.byref(cfg))
        self.guards = {}
        whole, self.state_t, sentinel = guarded((abi.VF_COUNT, self.n), torch.float32, self.dev)
        self.guards["state"] = (whole, sentinel)
        whole, self.obs_t, sentinel = guarded((self.n, self.num_obs), torch.float32, self.dev)
        self.guards["obs"] = (whole, sentinel)
        h = C.c_void_p()
        native.check(self.lib.vine_create(C.byref(cfg), device_id, self.state_t.data_ptr(), C.byref(h)), self.lib)
        self.h = h
        self.rew_t = torch.zeros(self.n, device=self.dev)
        self.reset_t = torch.ones(self.n, device=self.dev, dtype=torch.long)
        self.progress_t = torch.zeros(self.n, device=self.dev, dtype=torch.long)
        self.timeouts_t = torch.zeros(self.n, device=self.dev, dtype=torch.bool)
        self.reward_matrix_t, self._rv = None, None

    def bind_target(self, keys, table=None):
        """The observer's state (guarded) and the checked spec; ``table``: float32 [4, n] instead of episode 0's draw."""
        self.target_cfg = spec = config_for(self.cfg, keys)
        self.gids = np.arange(self.n, dtype=np.int64) + int(self.cfg.env_id_offset)
        _, values = env_target.target_names(spec)
        self.values_t = torch.as_tensor(values, dtype=torch.float64).to(self.dev) if len(values) else None
        self.tspec = env_target.target_spec(self.lib, self.cfg, spec, self.values_t.data_ptr() if len(values) else None)
        self.layout = env_target.layout_of(self.tspec)
        for name, shape, dtype, fill in (("table", (abi.VTG_NAMES, self.n), torch.float32, 0), ("motion", (abi.VTM_COUNT, self.n), torch.float32, 0),
                                         ("fresh", (self.n,), torch.uint8, 1), ("episode_index", (self.n,), torch.int32, 0)):
            whole, view, sentinel = guarded(shape, dtype, self.dev, fill)
            self.guards[name] = (whole, sentinel)
            setattr(self, name, view)
        first = env_target.draw_target(spec, int(self.cfg.seed), self.gids, 0).astype(np.float32) if table is None else table
        self.table.copy_(torch.as_tensor(np.ascontiguousarray(first)))
        self.table0 = np.ascontiguousarray(first)
        torch.cuda.synchronize(self.dev)

    def target(self, obs=None):
        """The launch, behind whatever is on the stream, on ``obs`` (default: the step's own buffer)."""
        obs = self.obs_t if obs is None else obs
        return self.lib.vine_env_target_scheduled(
            self.h, self.tspec, obs.data_ptr(), self.reset_t.data_ptr(), self.progress_t.data_ptr(), self.table.data_ptr(),
            self.motion.data_ptr(), self.fresh.data_ptr(), self.episode_index.data_ptr(), torch.cuda.current_stream(self.dev).cuda_stream)

    def guards_intact(self):
        for name, (whole, sentinel) in self.guards.items():
            w = whole.cpu().numpy()
            assert (w[:PAD] == sentinel).all() and (w[-PAD:] == sentinel).all(), name
        return True

    def replay(self, states, obs, progress, resets, axis, external=None, table=None):
        return env_target.target_replay(self.target_cfg, int(self.cfg.seed), self.gids, self.layout, states, obs, progress, resets,
                                        axis=axis, external_resets=external, table=self.table0 if table is None else table)

    def state_equals(self, want, what=""):
        for name in STATE:
            assert np.array_equal(words(getattr(self, name)), words(want[name].astype(getattr(self, name).cpu().numpy().dtype))), (what, name)
        return True

    return type("HipEnvMoved", (H,), {"__init__": init, "bind_target": bind_target, "target": target, "guards_intact": guards_intact,
                                      "replay": replay, "state_equals": state_equals})


def axis_ulps(motion, angle):
    """The device's AXIS rows against float64 cos / sin of the stored angle, in ulps of 1 (2^-23)."""
    angle = np.asarray(angle, dtype=np.float64)
    err = np.maximum(np.abs(motion[F.VTM_AXIS_C].astype(np.float64) - np.cos(angle)), np.abs(motion[F.VTM_AXIS_S].astype(np.float64) - np.sin(angle)))
    return err / 2.0 ** -23


def pose_error(mode, state):
    """|the pose a reset would derive in float64 from the target, the depth and the angle of ``state`` - the stored pose|, in
    ulps (float32) of the largest term: [n] for the shelf, the worse of y and z for the pipe."""
    ty, tz, depth, angle = (state[f].astype(np.float64) for f in (F.VF_TARGET_Y, F.VF_TARGET_Z, F.VF_OBJ_DEPTH, F.VF_OBJ_ANGLE))
    if mode == F.TARGET_SHELF:
        terms = [ty, depth, np.full_like(ty, 0.2), state[F.VF_SHELF_Y].astype(np.float64)]
        return np.abs(ty + (depth - 0.2) - state[F.VF_SHELF_Y]) / ulp32(np.max(np.abs(terms), axis=0))
    c, s = np.cos(angle), np.sin(angle)
    ey = np.abs(ty + depth * c + R_PIPE * s - state[F.VF_PIPE_Y]) / ulp32(np.max(np.abs([ty, depth * c, R_PIPE * s, state[F.VF_PIPE_Y]]), axis=0))
    ez = np.abs(tz + depth * s - R_PIPE * c - state[F.VF_PIPE_Z]) / ulp32(np.max(np.abs([tz, depth * s, R_PIPE * c, state[F.VF_PIPE_Z]]), axis=0))
    return np.maximum(ey, ez)


def hand_reset(rng, mode, n):
    """What a reset leaves in the fields the observer reads, with the obstacle's pose derived in float64 and rounded once."""
    ty, tz = rng.uniform(-0.3, -0.1, n).astype(f32), rng.uniform(0.55, 0.67, n).astype(f32)
    depth, angle = rng.uniform(0.0, 0.1, n).astype(f32), rng.uniform(-0.6, 0.6, n).astype(f32)
    ty[0], tz[1] = f32(-0.0), f32(-0.0)                             # signed zeros a resting env must keep
    out = {F.VF_TARGET_Y: ty, F.VF_TARGET_Z: tz, F.VF_OBJ_DEPTH: depth, F.VF_OBJ_ANGLE: angle}
    t64, z64, d64, a64 = (x.astype(np.float64) for x in (ty, tz, depth, angle))
    out[F.VF_SHELF_Y] = (t64 + (d64 - 0.2)).astype(f32)
    out[F.VF_PIPE_Y] = (t64 + d64 * np.cos(a64) + R_PIPE * np.sin(a64)).astype(f32)
    out[F.VF_PIPE_Z] = (z64 + d64 * np.sin(a64) - R_PIPE * np.cos(a64)).astype(f32)
    return out


# ------------------------------------------------------------------------------------------------------ the launch alone
@pytest.mark.parametrize("case", ["free", "shelf", "pipe"])
def test_launch_alone_equals_the_replay_after_every_launch(Moved, case):
    """40 launches; progress and reset by hand (episodes of 5 + e % 7 steps), the observation a pattern plus noise-like values in
    the velocity columns; the state block is the device's own from launch to launch, but for the envs whose progress is 0,
    which get a hand-made reset.  After every launch: state block, observation, table, motion, fresh and ordinals equal the
    replay bit for bit; every field the mode does not write and every env at rest keeps every bit; the pipe's axis lies
    within POS_ULPS ulps of 1 of float64 cos / sin; the pose a reset would derive from what the launch left is the stored
    pose within POS_ULPS ulps of the largest term.  Measured on one MI355X (profiles/env_target/axis_ulps.txt): 589 / 511 /
    542 reflections (free / shelf / pipe); axis 0.38 ulp of 1; pose 0.93 ulp (shelf), 1.18 ulp (pipe) of the largest term."""
    env = Moved(cfg_of(case))
    env.bind_target(SPECS[case])
    mode = env.layout["mode"]
    assert mode == {"free": F.TARGET_FREE, "shelf": F.TARGET_SHELF, "pipe": F.TARGET_PIPE}[case] and env.layout["vel_column"] == 22
    e = np.arange(N)
    assert np.array_equal(env.table0[0], np.asarray([0.0, 0.4, -0.4], f32)[e % 3])
    progress, resets = hand_flags(T, N)
    quiet = [5, 63, 64, N - 1]                                      # never flagged: their hand-made entries must survive
    resets[:, quiet] = 0
    table = env.table0.copy()
    table[:, quiet] = np.asarray([[-0.35], [0.0], [0.025], [0.0]], f32)
    if case == "free":
        table[1, quiet[0]], table[3, quiet[0]] = f32(0.2), f32(0.0125)
    env.table.copy_(torch.as_tensor(table))
    rng = np.random.default_rng(17)
    fd, ed = np.meshgrid(np.arange(F.VF_COUNT), e, indexing="ij")
    env.set_state(((fd + 1) / 8.0 + ed / 65536.0).astype(f32))
    before, raw, after, obs_after, motion_after = [], [], [], [], []
    for t in range(T):
        fresh_envs = e if t == 0 else np.flatnonzero(progress[t] == 0)       # (every env's first launch is a first frame)
        st = env.state_t.cpu().numpy()
        for field, values in hand_reset(rng, mode, N).items():
            st[field, fresh_envs] = values[fresh_envs]
        env.set_state(st)
        ob = rng.uniform(-1, 1, (N, env.num_obs)).astype(f32)
        ob[:, 22:24] = np.where(e[:, None] % 2 == 0, f32(0.0), ob[:, 22:24] * f32(0.01))      # without and with the step's noise
        ob[4, 22], ob[6, 23] = f32(4.95), f32(-4.999)                                             # near the clip
        env.obs_t.copy_(torch.as_tensor(ob))
        env.set_flags(resets[t], progress[t])
        env.step_count = t + 1
        assert env.target() == abi.OK
        torch.cuda.synchronize()
        before.append(st), raw.append(ob)
        after.append(env.state_t.cpu().numpy()), obs_after.append(env.obs_t.cpu().numpy()), motion_after.append(env.motion.cpu().numpy())
        assert env.guards_intact()
    axis = np.stack(motion_after)[:, F.VTM_AXIS_C:F.VTM_AXIS_S + 1]
    want = env.replay(np.stack(before), np.stack(raw), progress, resets, axis, table=table)
    worst_axis, worst_pose, reflections, moved, clamped = 0.0, 0.0, 0, 0, 0
    rest = [f for f in range(F.VF_COUNT) if f not in WRITTEN[mode]]
    for t in range(T):
        w = want[t]
        assert np.array_equal(words(after[t]), words(w["state"])), (case, t, "state")
        assert np.array_equal(words(obs_after[t]), words(w["obs"])), (case, t, "obs")
        assert np.array_equal(words(motion_after[t]), words(w["motion"])), (case, t, "motion")
        assert np.array_equal(words(after[t][rest]), words(before[t][rest])), (case, t, "a field the mode does not write")
        still = ~w["moving"]
        assert np.array_equal(words(after[t][:, still]), words(before[t][:, still])) and np.array_equal(words(obs_after[t][still]), words(raw[t][still]))
        others = [j for j in range(env.num_obs) if j not in (22, 23)]
        assert np.array_equal(words(obs_after[t][:, others]), words(raw[t][:, others]))
        reflections, moved = reflections + int(w["reflected"].sum()), moved + int(w["moving"].sum())
        clamped += int((np.abs(obs_after[t][:, 22:24]) == f32(env.cfg.clip_observations)).sum())
        if mode == F.TARGET_PIPE:
            worst_axis = max(worst_axis, float(axis_ulps(motion_after[t], after[t][F.VF_OBJ_ANGLE]).max()))
        if mode != F.TARGET_FREE:
            worst_pose = max(worst_pose, float(pose_error(mode, after[t]).max()))
    assert env.state_equals(want[-1], case)
    assert np.array_equal(words(env.table[:, quiet]), words(table[:, quiet])) and (env.episode_index.cpu().numpy()[quiet] == 0).all()
    assert np.array_equal(env.episode_index.cpu().numpy(), resets.sum(axis=0)) and int(env.episode_index.max()) >= 3 and int(env.fresh.max()) == 0
    assert reflections > 50 and moved > 1000 and any((~w["moving"]).sum() > 10 for w in want), (reflections, moved)
    assert case != "free" or clamped >= 1
    assert not want[0]["moving"][0] and after[0][F.VF_TARGET_Y].view(np.uint32)[0] == 0x80000000      # env 0 rests: its -0 stays
    print("launch alone, %s: %d reflections; axis %.3g ulp of 1; pose %.3g ulp of the largest term" % (case, reflections, worst_axis, worst_pose))
    assert worst_axis <= POS_ULPS and worst_pose <= POS_ULPS, (worst_axis, worst_pose)
    env.close()


def test_refusals_on_a_handle(Moved):
    env = Moved(cfg_of("free"))
    env.bind_target(SPECS["free"])
    lib, stream = env.lib, torch.cuda.current_stream().cuda_stream
    args = [env.h, env.tspec, env.obs_t.data_ptr(), env.reset_t.data_ptr(), env.progress_t.data_ptr(), env.table.data_ptr(),
            env.motion.data_ptr(), env.fresh.data_ptr(), env.episode_index.data_ptr(), stream]
    for k in range(9):
        bad = list(args)
        bad[k] = None
        assert lib.vine_env_target_scheduled(*bad) == abi.ERR_INVALID_ARG and b"null argument" in lib.vine_last_error()
    for field, value, word in (("checked", 0, b"not filled by"), ("mode", abi.TARGET_PIPE, b"obstacle flags"), ("vel_column", 27, b"vel_column")):
        bad_spec = abi.VineEnvTargetSpec.from_buffer_copy(env.tspec)
        setattr(bad_spec, field, value)
        bad = list(args)
        bad[1] = bad_spec
        assert lib.vine_env_target_scheduled(*bad) == abi.ERR_INVALID_ARG and word in lib.vine_last_error(), field
    assert env.guards_intact() and int(env.fresh.min()) == 1
    env.close()


# -------------------------------------------------------------------------------------------------- behind real steps
KEYS = ("obs", "rew", "reset", "progress", "timeouts", "state")


def run_moved(Moved, case, offset, keys, acts=None):
    """A handle with the launch behind every step.  Per step: everything the step wrote, the state block and the raw
    observation before the launch, and the observer's motion rows behind it."""
    acts = actions_for(N, T) if acts is None else acts
    env = Moved(cfg_of(case, N, offset))
    env.bind_target(keys)
    rec, before, raw, motion = {k: [] for k in KEYS}, [], [], []
    for act in acts:
        env.step_t(act.to(env.dev).contiguous(), sync=False)
        before.append(env.state_t.clone()), raw.append(env.obs_t.clone())
        assert env.target() == abi.OK
        motion.append(env.motion.clone())
        for k, t in zip(KEYS, (env.obs_t, env.rew_t, env.reset_t, env.progress_t, env.timeouts_t, env.state_t)):
            rec[k].append(t.clone())
    torch.cuda.synchronize()
    rec = {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}
    return env, rec, torch.stack(before).cpu().numpy(), torch.stack(raw).cpu().numpy(), torch.stack(motion).cpu().numpy()


def run_plain(Moved, case, offset):
    env = Moved(cfg_of(case, N, offset))
    rec = {k: [] for k in KEYS}
    for act in actions_for(N, T):
        env.step_t(act.to(env.dev).contiguous(), sync=False)
        for k, t in zip(KEYS, (env.obs_t, env.rew_t, env.reset_t, env.progress_t, env.timeouts_t, env.state_t)):
            rec[k].append(t.clone())
    torch.cuda.synchronize()
    env.close()
    return {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}


@pytest.mark.parametrize("case,offset", [("free", 0), ("pipe", 0), ("free", 1000), ("pipe", 1000)])
def test_behind_real_steps_the_next_step_reads_the_moved_target(Moved, case, offset):
    """Every launch equals the replay of what it found, bit for bit.  The target and depth columns of the observation step
    k + 1 writes are the words the launch stored behind step k, scaled and clamped as the step does.  A run with all
    velocities zero equals a run without the observer in every bit.  Measured on one MI355X: 536 to 694 reflections per run;
    pipe: axis 0.42 ulp of 1, pose 1.7 ulp of the largest term (offset 0), 0.41 / 1.39 (offset 1000)."""
    env, rec, before, raw, motion = run_moved(Moved, case, offset, SPECS[case])
    assert saw_resets_and_timeouts(rec), case
    mode = env.layout["mode"]
    want = env.replay(before, raw, rec["progress"], rec["reset"], motion[:, F.VTM_AXIS_C:F.VTM_AXIS_S + 1])
    rest = [f for f in range(F.VF_COUNT) if f not in WRITTEN[mode]]
    inv = (1.0 / np.asarray(env.cfg.obs_scaling[:env.num_obs], dtype=np.float64)).astype(f32)
    clip = f32(env.cfg.clip_observations)
    ty_col, tz_col, depth_col = env.num_obs - 16 + 7, env.num_obs - 16 + 8, env.num_obs - 16 + 14
    reflections, worst_pose, worst_axis, carried = 0, 0.0, 0.0, 0
    for t in range(T):
        w = want[t]
        assert np.array_equal(words(rec["state"][t]), words(w["state"])), (case, t, "state")
        assert np.array_equal(words(rec["obs"][t]), words(w["obs"])), (case, t, "obs")
        assert np.array_equal(words(motion[t]), words(w["motion"])), (case, t, "motion")
        assert np.array_equal(words(rec["state"][t][rest]), words(before[t][rest])), (case, t)
        reflections += int(w["reflected"].sum())
        if t + 1 < T:                                # the envs step t + 1 did not reset read what this launch stored
            held = np.flatnonzero(rec["progress"][t + 1] != 0)
            for col, field in ((ty_col, F.VF_TARGET_Y), (tz_col, F.VF_TARGET_Z)) + (((depth_col, F.VF_OBJ_DEPTH),) if mode else ()):
                stored = rec["state"][t][field][held]
                assert np.array_equal(words(raw[t + 1][held, col]), words(np.minimum(np.maximum(stored * inv[col], -clip), clip))), (case, t, col)
            moved = held[w["moving"][held]]
            carried += int((rec["state"][t][F.VF_TARGET_Y][moved] != before[t][F.VF_TARGET_Y][moved]).sum())
        if mode == F.TARGET_PIPE:
            worst_pose = max(worst_pose, float(pose_error(mode, rec["state"][t]).max()))
            worst_axis = max(worst_axis, float(axis_ulps(motion[t], rec["state"][t][F.VF_OBJ_ANGLE]).max()))
    assert env.state_equals(want[-1], case) and env.guards_intact()
    assert reflections >= 1 and carried > 500 and want[-1]["episode_index"].max() >= 2, (reflections, carried)
    print("%s at offset %d: %d reflections; axis %.3g ulp of 1; pose %.3g ulp of the largest term" % (case, offset, reflections, worst_axis, worst_pose))
    assert worst_pose <= POS_ULPS and worst_axis <= POS_ULPS, (worst_pose, worst_axis)
    env.close()
    # all velocities zero (per episode, so that the spec is one): not a bit differs from a run without the observer
    rest_env, rest_rec, rest_before, rest_raw, _ = run_moved(Moved, case, offset, RESTING)
    assert_bit_equal(rest_rec, run_plain(Moved, case, offset), what=case + " at rest")
    assert np.array_equal(words(rest_rec["state"]), words(rest_before)) and np.array_equal(words(rest_rec["obs"]), words(rest_raw))
    assert int(rest_env.episode_index.max()) >= 2 and rest_env.guards_intact()
    rest_env.close()
    # and the moving run differs from it in where the target is and in what the policy is shown of its velocity (the default
    # reward is sparse: in 40 steps of random actions it does not tell the two runs apart)
    assert not np.array_equal(rest_rec["state"][:, F.VF_TARGET_Y], rec["state"][:, F.VF_TARGET_Y])
    assert not rest_rec["obs"][:, :, 22:24].any() and np.count_nonzero(rec["obs"][:, :, 22]) > 500


def test_captured_groups_of_four_steps_replay_like_eager_launches(Moved):
    """Four (step + launch) pairs captured once, replayed ten times, against the same forty pairs launched eagerly; with the
    step's own observation noise on, which the launch adds the velocity to."""
    acts = actions_for(N, T).cuda()
    envs = []
    for graphed in (False, True):
        env = Moved(case_cfg("randomize-noise"))
        env.bind_target(SPECS["free"])
        env.slots = torch.zeros(4, N, 28, device="cuda")
        a_in = torch.zeros(4, N, 2, device="cuda")
        torch.cuda.synchronize()

        def group():
            for k in range(4):
                native.check(env.lib.vine_step(env.h, a_in[k].data_ptr(), env.slots[k].data_ptr(), env.rew_t.data_ptr(),
                                               env.reset_t.data_ptr(), env.progress_t.data_ptr(), env.timeouts_t.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), env.lib)
                assert env.target(env.slots[k]) == abi.OK
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
    assert float(eager.motion[F.VTM_OFF_ALONG].abs().max()) > 0.0 and float(eager.slots[:, :, 22].abs().max()) > 0.1
    eager.close()
    g_env.close()


# ----------------------------------------------------------------------------------------------------- the task class
class Tap:
    """A step observer that keeps copies of the state block, the observation the test says the step writes, and the step's
    flags, at its place in the order."""
    paused, copy_done = 0, None

    def __init__(self, env):
        self.env, self.obs, self.state, self.seen, self.reset, self.progress = env, None, [], [], [], []

    def enqueue(self, stream, actions=None):
        self.state.append(self.env._state.clone()), self.seen.append(self.obs.clone())
        self.reset.append(self.env.reset_buf.clone()), self.progress.append(self.env.progress_buf.clone())

    def before(self, n):
        pass

    advance = set_steps = before

    def live_tensors(self):
        return []

    def drain(self):
        pass

    close = drain

    def arrays(self):
        return tuple(torch.stack(v).cpu().numpy() for v in (self.state, self.seen, self.reset, self.progress))


def make_task(n, extra, target, env_params_spec=None, sensor=None, push=None, seed=42):
    from vine_robot_isaacgymenvs_amd import load_config
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_config(overrides=["num_envs=%d" % n, "task.env.CREATE_PIPE=False", "task.env.maxEpisodeLength=%d" % MAX_LEN] + list(extra))
    cfg["task"]["seed"] = seed
    cfg["task"]["env"]["ENV_TARGET"] = dict(target)
    for key, value in (("ENV_PARAMS", env_params_spec), ("ENV_SENSOR", sensor), ("ENV_PUSH", push)):
        if value:
            cfg["task"]["env"][key] = value
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                  headless=True)
    front, behind = Tap(env), Tap(env)
    at = env._observers.index(env.env_target)
    env._observers.insert(at + 1, behind)
    env._observers.insert(at, front)
    return env, front, behind


def check_task_run(env, front, behind, steps, external=None):
    """Every launch of a task-class run against the replay of what the tap in front of it saw; the observer's final state;
    every episode-log row's param_TARGET_* against the replay's table for that episode."""
    before, raw, resets, progress = front.arrays()
    after, delivered, _, _ = behind.arrays()
    p = env.env_target
    assert len(before) == steps == int(env.step_count)
    gids = np.arange(env.num_envs) + p.env_id_offset
    want = env_target.target_replay(p.spec, p.seed, gids, env_target.layout_of(p.tspec), before, raw, progress, resets, external_resets=external)
    reflections = 0
    for t in range(steps):
        assert np.array_equal(words(after[t]), words(want[t]["state"])), (t, "state")
        assert np.array_equal(words(delivered[t]), words(want[t]["obs"])), (t, "obs")
        reflections += int(want[t]["reflected"].sum())
    for name in STATE:
        assert np.array_equal(words(getattr(p, name)), words(want[-1][name].astype(getattr(p, name).cpu().numpy().dtype))), name
    assert reflections >= 1
    assert [t.data_ptr() for t in p.live_tensors()] == [t.data_ptr() for t in (p.motion, p.table, p.fresh, p.episode_index)]
    for view, rows in ((p.anchor, 2), (p.axis, 2), (p.off, 2), (p.vel, 2)):       # the named state is the block the launch takes
        assert view.shape == (rows, env.num_envs) and p.motion.data_ptr() <= view.data_ptr() < p.motion.data_ptr() + p.motion.numel() * 4
    assert p.depth0.data_ptr() == p.motion[abi.VTM_DEPTH0].data_ptr()
    live = [t.data_ptr() for t in env.live_tensors()]
    assert live[0] == env._state.data_ptr() and all(t.data_ptr() in live for t in p.live_tensors())
    env.episode_log.harvest()
    rows = env.episode_log.rows_with_params()
    assert len(rows["env"]) > env.num_envs and rows["episode"].max() >= 1
    first = env_target.draw_target(p.spec, p.seed, gids, 0).astype(np.float32)
    tables = np.stack([first] + [w["table"] for w in want[:-1]])            # the values in force while the row's last step ran
    for name in env_target.varying_names(p.spec):
        slot = env_target.NAMES.index(name)
        assert np.array_equal(words(rows["param_TARGET_" + name]), words(tables[rows["end_step"], slot, rows["env"]])), name
    return want, rows


def test_every_step_entry_of_the_task_class_moves_the_target_as_the_replay(tmp_path):
    """step, step_into, the fused rollout step and the evaluation step, ten of each in one run on the four-lane kernel; then
    reset_idx from outside, which sets fresh.  (free space: with no obstacle sincosf is not called and the replay needs no
    axis from the device.)"""
    from tests.test_eval_step import H, _eval_args, _eval_state, _head
    n = 256
    env, front, behind = make_task(n, ["task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_DIR=" + str(tmp_path)], SPECS["free"])
    try:
        lib, dev, st = env._lib, torch.device("cuda:0"), torch.cuda.current_stream().cuda_stream
        assert env.step_kernel_name == "vine_step_quad_kernel" and env.rollout_step_blocks() > 0 and env.eval_step_rows() > 0
        assert [type(o).__name__ for o in env.observers] == ["EpisodeLog", "Tap", "EnvTarget", "Tap"] and env.episode_log.target is env.env_target
        p, rnd = _head(dev, lib, st)
        acts = actions_for(n, 20, seed=11).cuda()
        out = torch.zeros(10, n, env.num_obs, device=dev)
        for k in range(10):
            front.obs = behind.obs = env._obs_ring[env._obs_slot ^ 1]
            env.step(acts[k])
        for k in range(10):
            front.obs = behind.obs = out[k]
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
            front.obs = behind.obs = out[k]
            env.step_rollout_into(ra, out[k])
            torch.cuda.synchronize()
            p["counter"] += 1
        se = _eval_state(env, n, dev)
        for k in range(10):
            y = rnd(n, H)
            front.obs = behind.obs = out[k]
            env.step_eval_into(_eval_args(se, p, y, 1), out[k])
            torch.cuda.synchronize()
        want, rows = check_task_run(env, front, behind, 40)
        assert env.env_target.episodes_now().max() >= 2
        # reset_idx from outside: fresh is set, and the next launch takes the anchor from where that reset put the target
        ids = [1, 7, 200]
        assert int(env.env_target.fresh.sum()) == 0
        env.reset_idx(ids)
        assert sorted(np.flatnonzero(env.env_target.fresh.cpu().numpy()).tolist()) == ids
        target_y = env._state[abi.VF_TARGET_Y].clone()
        front.obs = behind.obs = out[0]
        env.step_into(acts[0], out[0])
        torch.cuda.synchronize()
        assert int(env.env_target.fresh.sum()) == 0
        for e in ids:       # (reset_idx clears the flag and the progress: the step does not reset them again)
            assert float(env.env_target.anchor[0, e]) == float(target_y[e]) and float(env.env_target.off[0, e].abs()) <= 0.4 * 0.03332 * 1.001
        path = env.episode_log.path
    finally:
        env.close()
    from vine_robot_isaacgymenvs_amd.utils import episodes
    back = episodes.load_rows_with_params(path)
    done = len(rows["env"])                       # (the file also holds the episodes the step after reset_idx ended)
    assert np.array_equal(words(back["param_TARGET_VEL_ALONG"][:done]), words(rows["param_TARGET_VEL_ALONG"])) and len(back["env"]) >= done
    assert "param_TARGET_VEL_ACROSS" in back and "param_TARGET_SPAN_ACROSS" in back and "param_TARGET_SPAN_ALONG" not in back


def test_with_the_sensor_the_push_and_the_redraw_on_all_ordinals_are_equal(tmp_path):
    plants = {"DAMPING": [0.01, 0.05], "ACTION_DELAY": [0, 3]}
    env, front, behind = make_task(N, ["task.env.ENV_PARAMS_PER_EPISODE=True", "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_DIR=" + str(tmp_path)],
                                   SPECS["free"], env_params_spec=plants, sensor={"DELAY": [0, 3], "HOLD": 0.1, "PER_EPISODE": True},
                                   push={"RATE": 0.2, "IMPULSE": [0.0, 0.01], "PER_EPISODE": True})
    try:
        assert [type(o).__name__ for o in env.observers] == ["EpisodeLog", "Tap", "EnvTarget", "Tap", "EnvSensor", "EnvPush", "EnvRedraw"]
        acts = actions_for(N, T, seed=7).cuda()
        obs = torch.zeros(N, env.num_obs, device="cuda")
        front.obs = behind.obs = obs
        for k in range(T):
            env.step_into(acts[k], obs)
        check_task_run(env, front, behind, T)
        ordinals = env.env_redraw.episodes_now()
        for other in (env.env_target, env.env_push, env.env_sensor):
            assert np.array_equal(other.episodes_now(), ordinals)
        assert ordinals.max() >= 2
        rows = env.episode_log.rows_with_params()
        for column in ("param_DAMPING", "param_SENSOR_DELAY", "param_PUSH_IMPULSE", "param_TARGET_VEL_ALONG", "param_TARGET_SPAN_ACROSS"):
            assert column in rows, column
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------ train.py's entry
def test_train_and_play_entries_with_moving_targets(tmp_path, monkeypatch, capsys):
    """Two training iterations (horizon 8) with moving targets: finite scalars, the fused rollout (3 launches per step, the
    observers' behind them) and the four-lane kernel in force.  Then test=True with VEL_ALONG {values: [0, 0.2, -0.2]} and the
    episode log: the printed report has a param_TARGET_VEL_ALONG block with three values."""
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    from vine_robot_isaacgymenvs_amd.learning.player import PpoPlayerContinuous
    from vine_robot_isaacgymenvs_amd.train import main
    from vine_robot_isaacgymenvs_amd.utils import tfevents
    monkeypatch.chdir(tmp_path)
    common = ["task=Vine5LinkMovingBase", "num_envs=512", "headless=True", "experiment=moving", "task.env.CREATE_PIPE=False",
              "task.env.maxEpisodeLength=%d" % MAX_LEN, "task.env.EPISODE_LOG=True", "task.env.EPISODE_LOG_CAPACITY=32768"]
    seen = {}
    play = A2CAgent.play_steps_rnn

    def play_and_keep(self):
        out = play(self)
        env = getattr(self.vec_env, "env", self.vec_env)
        seen.update(launches=self.rollout_step_launches, kernel=env.step_kernel_name, target=env.env_target.spec,
                    observers=[type(o).__name__ for o in env.observers], moved=float(env.env_target.off.abs().max()))
        return out
    monkeypatch.setattr(A2CAgent, "play_steps_rnn", play_and_keep)
    main(common + ["minibatch_size=2048", "max_iterations=2", "train.params.config.horizon_length=8",
                   "train.params.config.save_frequency=1", "train.params.config.save_best_after=0", "+train.params.config.print_stats=False",
                   "task.env.ENV_TARGET={VEL_ALONG: [-0.2, 0.2], SPAN_ALONG: 0.05, PER_EPISODE: True}",
                   "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "train")])
    torch.cuda.synchronize()
    monkeypatch.setattr(A2CAgent, "play_steps_rnn", play)
    assert seen["launches"] == 3 and seen["kernel"] == "vine_step_quad_kernel" and seen["target"]["PER_EPISODE"] is True
    assert seen["observers"] == ["EpisodeLog", "EnvTarget"] and 0.0 < seen["moved"] <= 0.0501
    run = tmp_path / "runs" / "moving"
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
                                   "task.env.ENV_TARGET={VEL_ALONG: {values: [0, 0.2, -0.2]}, SPAN_ALONG: 0.05}",
                                   "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "play")])
    out = capsys.readouterr().out
    assert np.isfinite(reward) and steps > 0
    assert "reached_ever_rate by param_TARGET_VEL_ALONG:" in out
    velocities, rate, count = kept["player"].report["by_param"]["param_TARGET_VEL_ALONG"]
    assert np.array_equal(velocities, np.asarray([-0.2, 0.0, 0.2], dtype=np.float32)) and count.min() > 0
    assert int(count.sum()) == kept["player"].report["episodes"]
