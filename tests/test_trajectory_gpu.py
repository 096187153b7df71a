"""RECORD_TRAJECTORIES on the GPU: the record kernel against the state it copies (bit for bit) and against a float64
forward kinematics, the explicit-slot entry against the scheduled one, the player's graph replay against its eager twin
and against a run without the recorder, a training through train.py's entry with the recorder on and off, and the round
trip of a written file through MAT_FILE."""
import glob
import os

import numpy as np
import pytest
import scipy.io
import torch

from vine_robot_isaacgymenvs_amd import abi, load_config, load_task_config, native

pytestmark = pytest.mark.gpu

ENVS = [159, 0, 64, 63, 7]       # unsorted, both ends of 160 envs, a workgroup boundary of the four-lane kernel (64 envs each)
EVERY, STEPS = 9, 6
SENTINEL = -7777.0
# fp32 roundings charged to a tip coordinate, in ulps of the largest magnitude met in its sum (see the kernel test)
POS_ULPS, VEL_ULPS = 12, 58

KINDS = {
    # name: (env overrides, VINE_STEP_KERNEL, step kernel expected, seed)
    "free": (dict(CREATE_PIPE=False), None, "vine_step_quad_kernel", 1),
    "pipe": (dict(CREATE_PIPE=True), None, "vine_step_quad_kernel", 2),
    # the F6 shelf fixture's placements (tests/helpers.f6_cfg): targets inside the shelf, so that the vine touches it
    "shelf": (dict(CREATE_PIPE=False, CREATE_SHELF=True, USE_NONZERO_CONTACT_FORCE_RESET=True, SUCCESS_DIST=0.12,
                   RAIL_SOFT_LIMIT=0.2, MIN_TARGET_Y=-0.12, MAX_TARGET_Y=-0.02, MIN_TARGET_Z=0.56, MAX_TARGET_Z=0.66,
                   MIN_TARGET_DEPTH_IN_OBSTACLE=0.0, MAX_TARGET_DEPTH_IN_OBSTACLE=0.1, RANDOM_INIT_CART_MIN_Y=-0.02,
                   RANDOM_INIT_CART_MAX_Y=0.2), None, "vine_step_quad_kernel", 3),
    "lane": (dict(CREATE_PIPE=False), "lane", "vine_step_kernel", 4),
    "pos_only": (dict(CREATE_PIPE=False, OBSERVATION_TYPE="POS_ONLY", SCALE_OBSERVATIONS=False), None, "vine_step_kernel", 5),
}


def _task(n, seed=42, **env_over):
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % n])
    cfg["seed"] = seed
    cfg["env"].update(env_over)
    return isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg, rl_device="cuda:0", sim_device="cuda:0", graphics_device_id=0,
                                                    headless=True)


def _recorded(tmp_path, **over):
    return dict(RECORD_TRAJECTORIES=True, RECORD_TRAJECTORIES_EVERY=EVERY, RECORD_TRAJECTORIES_STEPS=STEPS,
                RECORD_TRAJECTORIES_ENVS=list(ENVS), RECORD_TRAJECTORIES_DIR=str(tmp_path), **over)


def _guard(rec):
    """The ring and the step list re-bound to the front of larger buffers: sentinel everywhere, tails to watch."""
    n = rec.ring.numel()
    big = torch.full((n + 1024,), SENTINEL, dtype=torch.float32, device=rec.device)
    rec.ring = big[:n].view(rec.ring.shape)
    bigs = torch.full((rec.steps.numel() + 64,), -99, dtype=torch.int64, device=rec.device)
    rec.steps = bigs[:rec.steps.numel()]
    return big[n:], bigs[rec.steps.numel():]


def _fk64(q, qd, L, z1, phi0):
    """Tip y, z, vy, vz of joint states q, qd [K, 6] in float64, and per row the largest magnitude met in the position sums
    and in the velocity sums (partial sums and terms)."""
    phi = phi0 + np.cumsum(q[:, 1:], axis=1)
    w = np.cumsum(qd[:, 1:], axis=1)
    ys = np.concatenate([q[:, :1], -L * np.sin(phi)], axis=1)
    zs = np.concatenate([np.full((len(q), 1), z1), L * np.cos(phi)], axis=1)
    vys = np.concatenate([qd[:, :1], -L * w * np.cos(phi)], axis=1)
    vzs = np.concatenate([np.zeros((len(q), 1)), -L * w * np.sin(phi)], axis=1)
    tip = np.stack([ys.sum(1), zs.sum(1), vys.sum(1), vzs.sum(1)], axis=1)

    def largest(*parts):
        return np.max(np.abs(np.concatenate([np.cumsum(p, axis=1) for p in parts] + list(parts), axis=1)), axis=1)
    return tip, largest(ys, zs), np.maximum(largest(vys, vzs), L * np.abs(w).max(axis=1))


def _ulp32(x):
    return np.spacing(np.maximum(np.abs(x), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def _check_rows(env, rows, actions, shelf):
    """Everything a row copies, bit for bit against the device buffers it was copied from."""
    e = torch.as_tensor(ENVS, device=env.device)
    st, f = env.state, abi
    assert torch.equal(rows[:, f.VRF_Q0:f.VRF_Q0 + 12], st[f.VF_Q0:f.VF_Q0 + 12][:, e].t())
    assert torch.equal(rows[:, f.VRF_TARGET_Y:f.VRF_TARGET_Z + 1], st[f.VF_TARGET_Y:f.VF_TARGET_Z + 1][:, e].t())
    assert torch.equal(rows[:, f.VRF_ACTION0:f.VRF_ACTION0 + 2], actions[e])
    assert torch.equal(rows[:, f.VRF_SMOOTHED_U], st[f.VF_SMOOTHED_U, e])
    assert torch.equal(rows[:, f.VRF_REWARD], env.rew_buf[e])
    assert torch.equal(rows[:, f.VRF_RESET], env.reset_buf[e].float())
    assert torch.equal(rows[:, f.VRF_TIMEOUT], env.timeout_buf[e].float())
    assert torch.equal(rows[:, f.VRF_PROGRESS], env.progress_buf[e].float())
    assert torch.equal(rows[:, f.VRF_OBJ_DEPTH], st[f.VF_OBJ_DEPTH, e]) and torch.equal(rows[:, f.VRF_OBJ_ANGLE], st[f.VF_OBJ_ANGLE, e])
    assert torch.equal(rows[:, f.VRF_CONTACT], st[f.VF_CONTACT, e] if shelf else torch.zeros_like(rows[:, 0]))
    assert not rows[:, f.VRF_RESERVED0:].any()


@pytest.mark.parametrize("kind", list(KINDS))
def test_kernel_copies_the_state_bit_for_bit(kind, tmp_path, monkeypatch, capsys):
    """160 envs (2.5 workgroups of the four-lane kernel in a grid of 4), 8-step episodes, 20 eager VecTask.step calls with
    random actions, windows of 6 steps every 9.  After every step the slot the schedule names holds the copied fields bit
    for bit and steps[slot] == s; a step outside a window changes nothing; sentinel tails behind both buffers survive.

    Tip fields against a float64 forward kinematics of the recorded q, qd.  The tolerance is N ulps of M, the largest
    magnitude met in the coordinate's sum (partial sums and terms, taken from the float64 evaluation; ulp = fp32 spacing at
    M), with every fp32 rounding on the path charged half an ulp of the magnitude it happens at.  Link k = 1..5 costs:
      the running angle th_k: k additions at |th| < 4, i.e. 4k half-ulps of 1 in the angle, hence in sin and cos;
      sincosf: one ulp = 2 half-ulps of 1; the rotation by phi0: two products and a sum, 3 half-ulps of 1;
      positions (y = q0 - L sum sin phi_k, z = z1 + L sum cos phi_k): the product by L, 1; all of the above enter scaled by
        L = 0.0885 < 0.1 and are half-ulps of 1 <= 2 M (M >= z1 - 5 L > 0.5); the accumulation, 1 half-ulp of M:
        sum_k [1 + 0.2 (4k + 6)] = 23 half-ulps of M                                            -> POS_ULPS = 12
      velocities (vy = qd0 - L sum w_k cos phi_k, |L w_k| <= M, so an absolute error of cos counts in full): the running
        rate w_k, k; two products, 2; the accumulation, 1: sum_k [(4k + 5) + k + 3] = 115 half-ulps  -> VEL_ULPS = 58
    These are worst cases with every rounding at its bound and of one sign.
    The sharper check is relative: on the same states the step kernel's own stored VF_TIP_* (a twin env with
    introspection on; rows of envs reset in that step excluded: their stored body state is stale by design,
    VINE_FLAG_STALE_BODY_STATE_AFTER_RESET) deviates from the same float64 values by some amount; the recorder's worst
    deviation must not exceed twice that (both are fp32 sums of five terms with independent rounding).  One figure each for
    the positions (the larger of y and z, metres) and for the velocities (the larger of vy and vz, metres per second): the
    maxima are one fp32 ulp or less of the coordinate, where a single coordinate's ratio is the ratio of two rounding
    accidents (half an ulp against one).  All eight figures are printed."""
    over, kernel, kernel_name, seed = KINDS[kind]
    if kernel:
        monkeypatch.setenv("VINE_STEP_KERNEL", kernel)          # read by vine_create
    env = _task(160, seed=seed, maxEpisodeLength=8, **_recorded(tmp_path, **over))
    twin = _task(160, seed=seed, maxEpisodeLength=8, introspection=True, **over)
    try:
        assert env.step_kernel_name == kernel_name == twin.step_kernel_name
        rec = env.trajectory
        assert twin.trajectory is None and rec.env_ids == ENVS and rec.ring.shape == (STEPS, len(ENVS), abi.RECORD_FIELDS)
        tail, stail = _guard(rec)
        vc = env._vcfg
        L, z1, phi0 = float(vc.link_length), float(vc.joint1_z), float(vc.phi0)
        g = torch.Generator(device=env.device).manual_seed(seed)
        actions = torch.rand((20, 160, 2), device=env.device, generator=g) * 2.4 - 1.2
        e = torch.as_tensor(ENVS, device=env.device)
        worst = {"recorder": np.zeros(4), "step kernel": np.zeros(4)}
        budget_ok, contacts, live = True, 0, 0
        restarts = torch.zeros(len(ENVS), dtype=torch.long, device=env.device)
        for s in range(20):
            ring0, steps0 = rec.ring.clone(), rec.steps.clone()
            env.step(actions[s])
            twin.step(actions[s])
            torch.cuda.synchronize()
            restarts += env.progress_buf[e] == 0                # the env was reset inside this step
            slot = s % EVERY
            if slot >= STEPS:                                   # outside a window: nothing moved
                assert torch.equal(rec.ring, ring0) and torch.equal(rec.steps, steps0), s
                continue
            live += 1
            keep = [i for i in range(STEPS) if i != slot]
            assert torch.equal(rec.ring[keep], ring0[keep]) and torch.equal(rec.steps[keep], steps0[keep]), s
            assert int(rec.steps[slot]) == s
            rows = rec.ring[slot]
            _check_rows(env, rows, actions[s], shelf=kind == "shelf")
            contacts += int((rows[:, abi.VRF_CONTACT] != 0).sum())
            # the tip: float64 forward kinematics of the recorded joint state
            r = rows.cpu().numpy().astype(np.float64)
            want, m_pos, m_vel = _fk64(r[:, 0:6], r[:, 6:12], L, z1, phi0)
            tol = np.stack([POS_ULPS * _ulp32(m_pos)] * 2 + [VEL_ULPS * _ulp32(m_vel)] * 2, axis=1)
            err = np.abs(r[:, 12:16] - want)
            budget_ok &= bool((err <= tol).all())
            worst["recorder"] = np.maximum(worst["recorder"], err.max(0))
            # the twin walked through the same states; its stored tip is valid where the env was not reset in this step
            assert torch.equal(twin.state[abi.VF_Q0:abi.VF_Q0 + 12][:, e], env.state[abi.VF_Q0:abi.VF_Q0 + 12][:, e])
            fresh = (twin.progress_buf[e] != 0).cpu().numpy()
            stored = twin.state[abi.VF_TIP_Y:abi.VF_TIP_VZ + 1][:, e].t().cpu().numpy().astype(np.float64)
            if fresh.any():
                worst["step kernel"] = np.maximum(worst["step kernel"], np.abs(stored - want)[fresh].max(0))
        with capsys.disabled():
            for who, w in worst.items():
                print("\n%-8s %-11s max |fp32 - float64 FK| over %d recorded steps x %d envs: tip y %.3e z %.3e m, vy %.3e vz %.3e m/s"
                      % (kind, who, live, len(ENVS), w[0], w[1], w[2], w[3]), end="")
            print()
        assert live == 14 and int(restarts.min()) >= 2          # every recorded env began several episodes
        assert bool((tail == SENTINEL).all()) and bool((stail == -99).all())
        if kind == "shelf":
            assert contacts > 0                                  # (contact is common in this placement; the seed is fixed so that it stays so)
        assert budget_ok
        pos = max(worst["recorder"][:2]) <= 2 * max(worst["step kernel"][:2])
        vel = max(worst["recorder"][2:]) <= 2 * max(worst["step kernel"][2:])
        assert pos and vel, worst
    finally:
        env.close()
        twin.close()


def test_explicit_slot_equals_scheduled(tmp_path):
    """vine_record into a named slot of a second ring, right behind a step whose scheduled launch wrote its own: same rows,
    same step index, nothing else touched; a slot past the ring is refused on the host."""
    env = _task(160, seed=1, maxEpisodeLength=8, **_recorded(tmp_path, CREATE_PIPE=False))
    try:
        rec = env.trajectory
        ring2 = torch.full_like(rec.ring, SENTINEL)
        steps2 = torch.full_like(rec.steps, -99)
        g = torch.Generator(device=env.device).manual_seed(9)
        stream = torch.cuda.current_stream(env.device).cuda_stream

        def record(slot, a):
            return rec.lib.vine_record(rec.handle, rec.rcfg, slot, rec.envs.data_ptr(), a.data_ptr(), env.rew_buf.data_ptr(),
                                       env.reset_buf.data_ptr(), env.progress_buf.data_ptr(), env.timeout_buf.data_ptr(),
                                       ring2.data_ptr(), steps2.data_ptr(), stream)
        for s, slot2 in ((0, 4), (1, 0), (2, 5)):
            a = torch.rand((160, 2), device=env.device, generator=g) * 2 - 1
            env.step(a)
            assert record(slot2, a) == abi.OK
            torch.cuda.synchronize()
            assert torch.equal(ring2[slot2], rec.ring[s]) and int(steps2[slot2]) == s == int(rec.steps[s])
        assert bool((ring2[[1, 2, 3]] == SENTINEL).all()) and steps2[[1, 2, 3]].tolist() == [-99] * 3
        assert record(STEPS, a) == abi.ERR_INVALID_ARG and b"slot" in rec.lib.vine_last_error()
        assert record(-1, a) == abi.ERR_INVALID_ARG
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------- the player
def _player(tmp_path, graph_steps, record):
    from vine_robot_isaacgymenvs_amd.learning.player import PpoPlayerContinuous
    from vine_robot_isaacgymenvs_amd.tasks import isaacgym_task_map

    class Paced(PpoPlayerContinuous):
        """Keeps what every EAGER device step wrote, and paces the loop to the writer thread (a harvest that finds the
        host buffer taken is, rightly, skipped)."""
        def _device_step(self):
            super()._device_step()
            if not torch.cuda.is_current_stream_capturing():
                self.seen.append((self._dev["action"].clone(), self._dev["dones"].clone()))
                if self.trajectory is not None and not self.trajectory.paused:
                    self.trajectory.drain()

    cfg = load_config(overrides=["num_envs=512", "task.env.maxEpisodeLength=8"])
    cfg["task"]["seed"] = 42
    if record:
        cfg["task"]["env"].update(RECORD_TRAJECTORIES=True, RECORD_TRAJECTORIES_EVERY=16, RECORD_TRAJECTORIES_STEPS=12,
                                  RECORD_TRAJECTORIES_ENVS=3, RECORD_TRAJECTORIES_DIR=str(tmp_path))
    env = isaacgym_task_map["Vine5LinkMovingBase"](cfg=cfg["task"], rl_device="cuda:0", sim_device="cuda:0",
                                                  graphics_device_id=0, headless=True)
    params = cfg["train"]["params"]
    params["config"]["player"] = {"graph_steps": graph_steps}
    torch.manual_seed(0)
    player = Paced(params, vec_env=env)
    player.seen, player.trajectory = [], env.trajectory
    if record:
        replayed = env.observers_replayed

        def paced(n_steps, before=False):
            replayed(n_steps, before=before)
            if not before:
                env.trajectory.drain()
        env.observers_replayed = paced
    return player, env


def _mats(directory):
    return {os.path.basename(p).split("_trajectory_")[1]: scipy.io.loadmat(p) for p in glob.glob(os.path.join(directory, "*.mat"))}


def test_player_graph_replay_equals_eager_and_recording_perturbs_nothing(tmp_path):
    """The device player at 512 envs, 40 steps (two replays of a 16-step graph and 8 eager steps, or 40 eager steps),
    windows of 12 steps every 16, three envs from index_to_view on: ring, step list and every array of the written files
    are bit-identical between the two; totals, episode accumulators, last observation and LSTM state also equal those of
    the graphed run WITHOUT the recorder; recorded actions are the player's action buffer of the eager run and the
    recorded reset flags add up to its done flags."""
    runs = {}
    for name, graph_steps, record in (("graph", 16, True), ("eager", 0, True), ("off", 16, False)):
        player, env = _player(tmp_path / name, graph_steps, record)
        try:
            player.run(n_steps=40)
            torch.cuda.synchronize()
            assert player.device_path is True
            d = player._dev
            out = dict(totals=d["totals"].clone(), episode=d["episode"].clone(), obs=d["obs_ring"][d["slot"]].clone(),
                       h=player.rnn_states[0].clone(), c=player.rnn_states[1].clone(), seen=player.seen)
            if record:
                rec = env.trajectory
                assert not rec.skipped and rec.steps_done == 40 == env.step_count
                assert rec.env_ids == [(env.index_to_view + k) % 512 for k in range(3)]
                out.update(ring=rec.ring.clone(), steps=rec.steps.clone(), ids=rec.env_ids, mats=_mats(str(tmp_path / name)))
                assert len(rec.written) == 6 and sorted(out["mats"]) == sorted("%d_env%d.mat" % (last, e) for last in (11, 27)
                                                                              for e in rec.env_ids)
            else:
                assert env.trajectory is None and not (tmp_path / name).exists()
            runs[name] = out
        finally:
            env.close()
    g, e, off = runs["graph"], runs["eager"], runs["off"]
    assert len(e["seen"]) == 40 and len(g["seen"]) == 16 + 8        # (the warm-up pass and the eager tail)
    assert torch.equal(g["ring"], e["ring"]) and torch.equal(g["steps"], e["steps"])
    assert g["steps"].tolist() == list(range(32, 40)) + list(range(24, 28))
    for name, m in g["mats"].items():
        for key, value in m.items():
            if not key.startswith("__"):
                assert np.array_equal(value, e["mats"][name][key]), (name, key)
    for k in ("totals", "episode", "obs", "h", "c"):
        assert torch.equal(g[k], e[k]) and torch.equal(g[k], off[k]), k
    for k, env_id in enumerate(e["ids"]):
        for last in (11, 27):
            m = e["mats"]["%d_env%d.mat" % (last, env_id)]
            window = range(last - 11, last + 1)
            assert m["step"][0].tolist() == list(window) and m["Q"].shape == (5, 12)
            assert np.array_equal(m["action"], np.stack([e["seen"][s][0][env_id].cpu().numpy() for s in window], 1))
            assert m["reset"].sum() == sum(int(e["seen"][s][1][env_id]) for s in window)
    assert sum(m["reset"].sum() for m in e["mats"].values()) >= 6       # 8-step episodes: every window holds an episode's end


def test_unpaced_harvest_accounts_for_every_window(tmp_path):
    """Nothing paces the loop to the writer here: 48 eager steps, windows of 4 steps every 4 (the launch that opens a
    window follows the one that closed the last, so ``before`` meets copies that are genuinely in flight).  Every
    completed window is either written whole or skipped because the writer still held the host buffer; a written file
    holds exactly its window's steps, copied before the next window overwrote the ring."""
    env = _task(64, seed=3, maxEpisodeLength=8, RECORD_TRAJECTORIES=True, RECORD_TRAJECTORIES_EVERY=4,
                RECORD_TRAJECTORIES_STEPS=4, RECORD_TRAJECTORIES_ENVS=[9, 2], RECORD_TRAJECTORIES_DIR=str(tmp_path),
                CREATE_PIPE=False)
    try:
        rec = env.trajectory
        g = torch.Generator(device=env.device).manual_seed(2)
        actions = torch.rand((48, 64, 2), device=env.device, generator=g) * 2 - 1
        for s in range(48):
            env.step(actions[s])
        torch.cuda.synchronize()
        rec.drain()
        assert rec.windows_written + rec.windows_skipped == 12 and rec.windows_written >= 1
        assert len(rec.written) == 2 * rec.windows_written and len(rec.skipped) == rec.windows_skipped
        assert sorted(list(rec.skipped) + [int(os.path.basename(p).split("_trajectory_")[1].split("_")[0]) for p in rec.written if p.endswith("env9.mat")]) \
            == [4 * w + 3 for w in range(12)]
        for path in rec.written:
            m = scipy.io.loadmat(path)
            last, e = int(os.path.basename(path).split("_trajectory_")[1].split("_")[0]), int(m["env"][0, 0])
            assert m["step"][0].tolist() == list(range(last - 3, last + 1))
            assert np.array_equal(m["action"], actions[last - 3:last + 1, e].t().cpu().numpy().astype(np.float64))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------- training
def _train(tmp_path, monkeypatch, name, record):
    from vine_robot_isaacgymenvs_amd import train
    from vine_robot_isaacgymenvs_amd.learning.a2c_continuous import A2CAgent
    run = tmp_path / name
    run.mkdir()
    monkeypatch.chdir(run)
    seen = {"actions": []}
    play = A2CAgent.play_steps_rnn

    def play_and_keep(self):
        out = play(self)
        seen["agent"] = self
        seen["actions"].append(self.buf["actions"].clone())          # [horizon, envs, 2] of this rollout
        return out
    monkeypatch.setattr(A2CAgent, "play_steps_rnn", play_and_keep)
    argv = ["num_envs=512", "minibatch_size=2048", "seed=5", "max_iterations=6", "headless=True",
            "+train.params.config.print_stats=False"]
    if record:
        argv += ["task.env.RECORD_TRAJECTORIES=True", "task.env.RECORD_TRAJECTORIES_EVERY=64",
                 "task.env.RECORD_TRAJECTORIES_STEPS=24", "task.env.RECORD_TRAJECTORIES_ENVS=2"]
    train.main(argv)
    torch.cuda.synchronize()
    monkeypatch.setattr(A2CAgent, "play_steps_rnn", play)
    root = run / "runs" / "Vine5LinkMovingBase"
    ckpt = sorted(glob.glob(str(root / "nn" / "last_*ep6*.pth")))
    assert ckpt, os.listdir(str(root / "nn"))
    return torch.load(ckpt[-1], map_location="cpu", weights_only=False), seen, root


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _same(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, path + "/" + str(i))
    elif torch.is_tensor(a):
        assert torch.equal(a, b), path
    else:
        assert a == b or (a != a and b != b), path


def test_training_with_the_recorder_on_and_off(tmp_path, monkeypatch):
    """Two trainings through train.py's entry (512 envs, six iterations of 16 steps, same seed), RECORD_TRAJECTORIES on
    and off: weights and optimiser state are bit-identical.  With it on, the windows opened at steps 0 and 64 are complete
    (files ..._23_... and ..._87_... of both envs, 24 consecutive steps each) and their action columns are the agent's
    rollout-buffer actions of that env; the fused rollout step still counts three launches."""
    off, off_seen, off_root = _train(tmp_path, monkeypatch, "off", False)
    on, on_seen, root = _train(tmp_path, monkeypatch, "on", True)
    _same(on, off)
    agent = on_seen["agent"]
    assert agent.rollout_step_launches == 3 == off_seen["agent"].rollout_step_launches
    assert getattr(off_seen["agent"].vec_env, "env", off_seen["agent"].vec_env).trajectory is None
    assert not glob.glob(str(off_root / "*_trajectory_*"))
    actions = torch.cat(on_seen["actions"]).cpu().numpy()            # [96, 512, 2]
    assert actions.shape == (96, 512, 2)
    ids = [51, 52]                                                   # index_to_view = int(0.1 * 512) and the next
    files = sorted(os.path.basename(p).split("_trajectory_")[1] for p in glob.glob(str(root / "*_trajectory_*.mat")))
    assert files == sorted("%d_env%d.mat" % (last, e) for last in (23, 87) for e in ids)
    for path in glob.glob(str(root / "*_trajectory_*.mat")):
        m = scipy.io.loadmat(path)
        last, env_id = int(m["step"][0, -1]), int(m["env"][0, 0])
        assert m["step"][0].tolist() == list(range(last - 23, last + 1)) and last in (23, 87) and env_id in ids
        assert m["Q"].shape == (5, 24) and m["cart_pos"].shape == (1, 24)
        assert np.array_equal(m["action"], actions[last - 23:last + 1, env_id].T.astype(np.float64))
        assert m["dt"][0, 0] == pytest.approx(4 * 0.00833)


# ------------------------------------------------------------------------------------------------------ round trip
def test_a_recorded_file_replays_through_mat_file(tmp_path):
    """A written file handed back as task.env.MAT_FILE loads, and the replay table is the recorded rows' q(6), target(2),
    tip(2), tip velocity(2) exactly (float32 -> float64 -> float32).  The recorder also runs beside the replay, which is
    eager by construction."""
    env = _task(64, seed=7, maxEpisodeLength=8, RECORD_TRAJECTORIES=True, RECORD_TRAJECTORIES_EVERY=6,
                RECORD_TRAJECTORIES_STEPS=6, RECORD_TRAJECTORIES_ENVS=[5], RECORD_TRAJECTORIES_DIR=str(tmp_path / "a"),
                CREATE_PIPE=False)
    try:
        g = torch.Generator(device=env.device).manual_seed(1)
        for _ in range(6):
            env.step(torch.rand((64, 2), device=env.device, generator=g) * 2 - 1)
        torch.cuda.synchronize()
        env.trajectory.drain()
        path = env.trajectory.path(5, 5)
        assert list(env.trajectory.written) == [path] and env.trajectory.windows_written == 1
        assert torch.equal(env.trajectory.steps.cpu(), torch.arange(6))
        rows = env.trajectory.ring[:, 0].cpu().numpy()               # the window is still in the ring
    finally:
        env.close()
    replay = _task(64, seed=7, maxEpisodeLength=8, MAT_FILE=path, CREATE_PIPE=False, RECORD_TRAJECTORIES=True,
                   RECORD_TRAJECTORIES_EVERY=6, RECORD_TRAJECTORIES_STEPS=6, RECORD_TRAJECTORIES_ENVS=[5],
                   RECORD_TRAJECTORIES_DIR=str(tmp_path / "b"))
    try:
        assert replay.graph_capturable is False
        cols = list(range(0, 6)) + [abi.VRF_TARGET_Y, abi.VRF_TARGET_Z, abi.VRF_TIP_Y, abi.VRF_TIP_Z, abi.VRF_TIP_VY, abi.VRF_TIP_VZ]
        assert np.array_equal(replay._mat_table.cpu().numpy(), rows[:, cols])
        for _ in range(6):
            replay.step(torch.zeros((64, 2), device=replay.device))
        torch.cuda.synchronize()
        replay.trajectory.drain()
        again = scipy.io.loadmat(replay.trajectory.path(5, 5))
        assert again["step"][0].tolist() == list(range(6)) and again["Q"].shape == (5, 6)
    finally:
        replay.close()
