"""MPC_TRACK on the GPU (include/vine_mpc_track.h, utils/mpc_track.py): the plan alone against ``plan_replay`` and against the
plant's own observer k steps later; the node alone behind real model steps against ``node_replay``; samples fed the plant's
actions stay the plant while its target moves (and do not without the node); ``held`` against the plain controller; the
captured graph against eager launches; and ``play`` and the command line.  There is no "it tracks" test: the float64 oracle shows
no clear margin at a shape that runs in seconds (scripts/mpc_track_oracle_check.py, profiles/mpc_track/it_tracks_oracle.txt,
DESIGN.md section 30).

Shapes (M plants, K samples, H steps) are tests/test_mpc_gpu.py's: (5, 14, 12), (2, 300, 3), (1, 2, 1).  The ENV_TARGET values are
tests/test_env_target_gpu.py's ``SPECS``: |VEL| = 0.4 m/s over a SPAN of 0.02 .. 0.03 m turns round within 12 steps of the tests'
control period.  The plant's and the model's state blocks, ``path`` and ``live`` lie between sentinels.  "Bit for bit" is literal:
floats are compared as words."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.helpers import f6_cfg
from tests.test_env_sensor_gpu import PAD, guarded
from tests.test_env_target_gpu import Moved  # noqa: F401  (the fixture: HipEnv between sentinels, with the target's observer)
from tests.test_mpc_gpu import NOT_RING, SENTINEL, SHAPES, Rig, _bits, _cfg, _plant_cfg, _random_nominal, _same, _stream
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import mpc, mpc_track
from vine_robot_isaacgymenvs_amd.utils.config import ConfigError

pytestmark = pytest.mark.gpu

F = abi
f32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["free", "shelf", "pipe"]
MODE = {"free": F.TARGET_FREE, "shelf": F.TARGET_SHELF, "pipe": F.TARGET_PIPE}
WORDS = [F.VF_TARGET_Y, F.VF_TARGET_Z, F.VF_OBJ_DEPTH]
WRITTEN = {F.TARGET_FREE: (F.VF_TARGET_Y, F.VF_TARGET_Z), F.TARGET_SHELF: (F.VF_TARGET_Y, F.VF_OBJ_DEPTH),
           F.TARGET_PIPE: (F.VF_TARGET_Y, F.VF_TARGET_Z, F.VF_OBJ_DEPTH)}
# tests/test_env_target_gpu.py's SPECS, copied: value lists with zero and both signs; 0.4 m/s * cdt = 0.0133 m a step
SPECS = {"free": dict(VEL_ALONG={"values": [0.0, 0.4, -0.4]}, VEL_ACROSS={"values": [0.0, 0.25, -0.3]}, SPAN_ALONG=0.03, SPAN_ACROSS=[0.02, 0.03],
                      PER_EPISODE=True),
         "shelf": dict(VEL_ALONG={"values": [0.0, 0.4, -0.4]}, SPAN_ALONG=[0.02, 0.03], PER_EPISODE=True),
         "pipe": dict(VEL_ALONG={"values": [0.0, 0.4, -0.4]}, SPAN_ALONG={"values": [0.03, 0.02]}, PER_EPISODE=True)}
MAX_LEN = 100                   # episodes far longer than a horizon: the time-out alone leaves every plant of a plan compared


def track_cfg(case, n):
    """tests/test_mpc_gpu.py's configuration (ACTION_DELAY 1, none of the optional resets) in the three modes, with
    POSITION_REWARD_WEIGHT 1 (the planner's default cost): the reward then follows the target wherever the tip is."""
    if case != "shelf":
        cfg = _cfg(n, pipe=case == "pipe")
    else:
        cfg = f6_cfg(n, 1, 0, "shelf")
        cfg.max_episode_length = MAX_LEN
        for flag in (abi.FLAG_USE_TARGET_REACHED_RESET, abi.FLAG_USE_TIP_LIMIT_HIT_RESET, abi.FLAG_USE_NONZERO_CONTACT_FORCE_RESET):
            cfg.set_flag(flag, False)
    assert cfg.max_episode_length == MAX_LEN
    cfg.reward_weights[0] = 1.0
    return cfg


class TrackRig(Rig):
    """tests/test_mpc_gpu.py's ``Rig`` with a plant that carries ENV_TARGET: both handles between sentinels (``Moved``), the
    plant's observer bound, and ``path`` and ``live`` guarded and sentinel-filled."""

    def __init__(self, Moved, case, M, K, H, kind="exact", sigma=(0.5, 0.25), lam=0.05, seed=77):
        self.M, self.K, self.H, self.N, self.case, self.mode = M, K, H, M * K, case, MODE[case]
        self.lib = native.load()
        self.plant = Moved(track_cfg(case, M))
        self.plant.bind_target(SPECS[case])
        self.model = Moved(track_cfg(case, M * K))
        d = self.dev = self.plant.dev
        self.mcfg = mpc.mpc_config(M, K, H, lam, list(sigma), seed)
        self.sigma, self.lam, self.seed, self.clip = list(sigma), lam, seed, float(self.model.cfg.clip_actions)
        self.nominal = torch.zeros((M, H, 2), device=d)
        self.history = torch.zeros((M, F.MAX_DELAY, 2), device=d)
        self.tick = torch.zeros(M, dtype=torch.long, device=d)
        self.cost = torch.full((self.N,), SENTINEL, dtype=torch.float64, device=d)
        self.alive = torch.full((self.N,), 9, dtype=torch.uint8, device=d)
        self.window = torch.full((1,), -99, dtype=torch.long, device=d)
        self.actions = torch.full((self.N, 2), SENTINEL, device=d)
        self.plant_actions = torch.full((M, 2), SENTINEL, device=d)
        self.weights = torch.full((self.N,), SENTINEL, dtype=torch.float64, device=d)
        self.guards = {}
        for name, shape, dtype in (("path", (M, H, F.MPC_TRACK_WORDS), torch.float32), ("live", (M,), torch.uint8)):
            whole, view, sentinel = guarded(shape, dtype, d, SENTINEL if dtype == torch.float32 else 0x5A)
            self.guards[name] = (whole, sentinel)
            setattr(self, name, view)
        self.kspec = mpc_track.track_spec(self.lib, self.plant.tspec, self.mcfg, kind)
        assert self.kspec.mode == self.mode and _same(f32(self.kspec.cdt), f32(self.plant.layout["cdt"]))

    def warm_plant(self, steps=10, seed=3, scale=1.3):
        """``Rig.warm_plant`` with the plant's observer behind every step."""
        rng = np.random.default_rng(seed)
        acts = rng.uniform(-scale, scale, (steps, self.M, 2)).astype(np.float32)
        for a in acts:
            self.plant_step(a)
        torch.cuda.synchronize()
        self.history.copy_(torch.as_tensor(np.ascontiguousarray(acts[::-1][:F.MAX_DELAY].transpose(1, 0, 2))))
        return acts

    def plant_step(self, actions):
        self.plant.step(actions, sync=False)
        assert self.plant.target() == abi.OK, self.lib.vine_last_error()

    def plan(self, kspec=None):
        p = self.plant
        rc = self.lib.vine_mpc_track_plan(p.h, kspec or self.kspec, p.reset_t.data_ptr(), p.fresh.data_ptr(), p.table.data_ptr(),
                                          p.motion.data_ptr(), self.path.data_ptr(), self.live.data_ptr(), _stream(self.dev))
        assert rc == abi.OK, self.lib.vine_last_error()

    def track_node(self):
        rc = self.lib.vine_mpc_track_scheduled(self.model.h, self.kspec, self.window.data_ptr(), self.alive.data_ptr(),
                                               self.path.data_ptr(), self.live.data_ptr(), _stream(self.dev))
        assert rc == abi.OK, self.lib.vine_last_error()

    def plan_replay(self, kind):
        p = self.plant
        return mpc_track.plan_replay(self.mode, kind, p.layout["cdt"], self.H, p.state_t.cpu().numpy(), p.motion.cpu().numpy(),
                                     p.table.cpu().numpy(), p.fresh.cpu().numpy(), p.reset_t.cpu().numpy())

    def guards_intact(self):
        for name, (whole, sentinel) in self.guards.items():
            w = whole.cpu().numpy()
            assert (w[:PAD] == sentinel).all() and (w[-PAD:] == sentinel).all(), name
        return self.plant.guards_intact() and self.model.guards_intact()


def plant_snapshot(plant):
    return {name: getattr(plant, name).cpu().numpy().copy() for name in ("state_t", "motion", "table", "fresh", "episode_index", "reset_t", "progress_t")}


# -------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("case", CASES)
def test_the_plan_alone_against_the_replay_and_against_the_plants_own_observer(Moved, case):
    """At the three shapes: ``path`` and ``live`` of the three kinds equal ``plan_replay`` bit for bit (one plant made fresh by hand
    as well), and nothing of the plant's state block, motion, table, fresh or flags changes.  Then the plant takes H - 1 real steps
    with its observer behind each: its three state words behind step k equal ``path[:, k]`` of the ``exact`` plan for every plant
    that raised no reset meanwhile -- against the existing kernel, through reflections, on at least half of M * H entries."""
    for shape_index, (M, K, H) in enumerate(SHAPES):
        rig = TrackRig(Moved, case, M, K, H)
        try:
            rig.warm_plant(8, seed=5 + shape_index, scale=0.6)
            plant = rig.plant
            for fresh_plant in (None, M - 1):
                if fresh_plant is not None:
                    plant.fresh[fresh_plant] = 1
                before = plant_snapshot(plant)
                for kind in mpc_track.PATHS:
                    rig.path.fill_(SENTINEL)
                    rig.live.fill_(0x5A)
                    rig.plan(mpc_track.track_spec(rig.lib, plant.tspec, rig.mcfg, kind))
                    torch.cuda.synchronize()
                    want = rig.plan_replay(kind)
                    assert _same(rig.path.cpu().numpy(), want["path"]), (M, kind)
                    assert np.array_equal(rig.live.cpu().numpy(), want["live"]), (M, kind)
                    after = plant_snapshot(plant)
                    for name in before:
                        assert _same(before[name], after[name]), (M, kind, name)
                    assert rig.guards_intact()
                    if kind == "held":
                        assert not want["live"].any()
                    if fresh_plant is not None:
                        assert want["live"][fresh_plant] == 0
                if fresh_plant is not None:
                    plant.fresh[fresh_plant] = 0
            rig.plan()                                                     # exact, from the motion block as it stands
            torch.cuda.synchronize()
            want = rig.plan_replay("exact")
            path = rig.path.cpu().numpy()
            assert _same(path, want["path"])
            ok = plant.reset_t.cpu().numpy() == 0
            compared, reflections = int(ok.sum()), 0
            assert _same(path[:, 0], plant.state_t.cpu().numpy()[WORDS].T)
            rng = np.random.default_rng(31)
            for k in range(1, H):
                rig.plant_step(rng.uniform(-0.6, 0.6, (M, 2)).astype(f32))
                torch.cuda.synchronize()
                ok &= plant.reset_t.cpu().numpy() == 0
                words = plant.state_t.cpu().numpy()[WORDS].T
                assert _same(words[ok], path[ok, k]), (M, k)
                compared += int(ok.sum())
                reflections += int(want["reflected"][ok, k].sum())
            assert compared * 2 >= M * H, (compared, M, H)
            if shape_index == 0:
                assert want["live"].sum() >= 2 and reflections >= 2 * int(want["live"].sum()), (reflections, want["live"])
            assert rig.guards_intact()
        finally:
            rig.close()


# -------------------------------------------------------------------------------------------------------------- the node
@pytest.mark.parametrize("case", CASES)
def test_the_node_alone_behind_real_model_steps(Moved, case):
    """Fork, then H + 2 x (model step, scoring node, track node) at the three shapes, with a few samples dead by hand and whatever
    the plan found not live: behind every launch the model's state block equals ``node_replay``'s of the block in front of it;
    every field the mode does not write, every dead sample and every sample of a plant that is not live keeps every bit; the
    launches at k = 0 (behind the fork), H and beyond store nothing."""
    for shape_index, (M, K, H) in enumerate(SHAPES):
        rig = TrackRig(Moved, case, M, K, H)
        try:
            rig.warm_plant(9, seed=2 + shape_index, scale=0.6)
            _random_nominal(rig, seed=13, scale=0.9)
            rig.model.step_count = 3
            rig.plan()
            assert rig.fork() == abi.OK, rig.lib.vine_last_error()
            dead = sorted({1 % rig.N, (K + 3) % rig.N, rig.N - 1}) if rig.N > 2 else [1]
            rig.alive[dead] = 0
            torch.cuda.synchronize()
            path, live = rig.path.cpu().numpy(), rig.live.cpu().numpy()
            plant_of = np.arange(rig.N) // K
            forked = rig.model.state_t.cpu().numpy().copy()
            rig.track_node()                                               # k = 0
            torch.cuda.synchronize()
            assert _same(rig.model.state_t.cpu().numpy(), forked)
            wrote = 0
            for k in range(1, H + 3):
                rig.model.step_t(rig.actions, sync=False)
                rig.node()
                torch.cuda.synchronize()
                assert rig.model.step_count - int(rig.window[0]) == k
                before, alive = rig.model.state_t.cpu().numpy().copy(), rig.alive.cpu().numpy().copy()
                rig.track_node()
                torch.cuda.synchronize()
                got = rig.model.state_t.cpu().numpy()
                assert _same(got, mpc_track.node_replay(rig.mode, K, k, before, alive, path, live)), (M, k)
                keep = (live[plant_of] == 0) | (alive == 0)
                assert not alive[dead].any() and _same(got[:, keep], before[:, keep]), (M, k)
                for field in range(F.VF_COUNT):
                    if field not in WRITTEN[rig.mode]:
                        assert _same(got[field], before[field]), (M, k, field)
                if k >= H:
                    assert _same(got, before), (M, k)
                else:
                    for field in WRITTEN[rig.mode]:
                        assert _same(got[field][~keep], path[plant_of[~keep], k, WORDS.index(field)]), (M, k, field)
                    wrote += int((~keep).sum())
            if shape_index == 0:
                assert wrote >= (H - 1) * K and (live == 0).any() and live.any()      # (neither branch ran empty)
            assert rig.guards_intact()
        finally:
            rig.close()


# ------------------------------------------------------------------------------------------------ the feature's own test
@pytest.mark.parametrize("case", ["free", "pipe"])
def test_forked_samples_fed_the_plants_actions_stay_the_plant_while_its_target_moves(Moved, case):
    """The moving-target twin of tests/test_mpc_gpu.py test_forked_samples_fed_the_plants_actions_stay_the_plant.  sigma = 0, the
    plant carries ENV_TARGET, the path kind is ``exact``: every sample's state-block column (the ring compared slot-rotated), rew,
    progress and reset equal the plant's in every bit over H steps, until a first reset.  Behind step H the plant's observer has
    moved its target to entry H, which no model step reads and the table does not hold: there the three target words are left
    out.  WITHOUT the track node the same comparison differs in ``rew``: that is what the feature exists for."""
    M, K, H = SHAPES[0]
    differs = {}
    for tracked in (True, False):
        rig = TrackRig(Moved, case, M, K, H, sigma=(0.0, 0.0))
        try:
            rig.warm_plant(11, seed=5, scale=0.6)
            _random_nominal(rig, seed=13, scale=0.9)
            rig.model.step_count = 3
            if tracked:
                rig.plan()
            assert rig.fork() == abi.OK, rig.lib.vine_last_error()
            nominal = rig.nominal.cpu().numpy()
            plant_of = np.arange(M * K) // K
            live = rig.plant.reset_t.cpu().numpy()[plant_of] == 0
            moving = (rig.plant.motion.cpu().numpy()[[F.VTM_VEL_ALONG, F.VTM_VEL_ACROSS]] != 0).any(axis=0)
            assert moving.sum() >= 2 and (live & moving[plant_of]).any()
            compared = rew_differs = reflections = 0
            want = rig.plan_replay("exact")
            for k in range(H):
                assert _same(rig.actions.cpu().numpy(), nominal[plant_of, k])
                rig.model.step_t(rig.actions, sync=False)
                rig.node()
                if tracked:
                    rig.track_node()
                rig.plant_step(nominal[:, k])
                torch.cuda.synchronize()
                cp, cm = rig.plant.step_count, rig.model.step_count
                assert (cp, cm) == (12 + k, 4 + k)
                pst, st = rig.plant.state_t.cpu().numpy(), rig.model.state_t.cpu().numpy()
                same_rew = _bits(rig.model.rew_t.cpu().numpy()) == _bits(rig.plant.rew_t.cpu().numpy()[plant_of])
                if tracked:
                    for f in NOT_RING:
                        if k == H - 1 and f in WRITTEN[rig.mode]:
                            continue
                        assert _same(st[f][live], pst[f][plant_of][live]), (k, f)
                    for w in (0, 1):                                       # ACTION_DELAY 1: one slot, rotated by the step counts
                        assert _same(st[F.VF_FIFO0 + w][live], pst[F.VF_FIFO0 + w][plant_of][live])
                    assert same_rew[live].all(), k
                    assert np.array_equal(rig.model.progress_t.cpu().numpy()[live], rig.plant.progress_t.cpu().numpy()[plant_of][live])
                    assert np.array_equal(rig.model.reset_t.cpu().numpy()[live], rig.plant.reset_t.cpu().numpy()[plant_of][live])
                    reflections += int(want["reflected"][:, k].sum()) if k else 0
                else:
                    rew_differs += int((~same_rew[live]).sum())
                    assert same_rew[live & ~moving[plant_of]].all(), k      # a resting plant needs no node
                compared += int(live.sum())
                live &= (rig.model.reset_t.cpu().numpy() == 0) & (rig.plant.reset_t.cpu().numpy()[plant_of] == 0)
            assert compared >= M * K * H // 2                              # (the comparison did not run empty)
            if tracked:
                assert reflections >= 2                                    # ... and ran through reflections
            differs[tracked] = rew_differs
            assert rig.guards_intact()
        finally:
            rig.close()
    assert differs[True] == 0 and differs[False] >= K * (H - 2), differs


# ------------------------------------------------------------------------------------------------------ the task classes
TARGET = {"VEL_ALONG": {"values": [0.0, 0.4, -0.4]}, "VEL_ACROSS": {"values": [0.0, 0.25, -0.3]}, "SPAN_ALONG": 0.03, "SPAN_ACROSS": [0.02, 0.03]}


def _tasks(M, K, cost=None, **plant_over):
    cfg = _plant_cfg(M, ENV_TARGET=dict(TARGET), **plant_over)
    plant = mpc.make_task(cfg)
    return plant, mpc.make_task(mpc.model_config(cfg, M, K, cost))


def test_held_equals_the_controller_without_tracking():
    """``TrackingController`` with ``PATH: held`` against a plain ``Controller`` on the same moving-target plants, ten control steps
    each: plant state, nominal, plant_actions and cost bit-identical -- the launches alone change nothing."""
    M, K, H = 4, 16, 6
    runs = []
    for held in (True, False):
        plant, model = _tasks(M, K, maxEpisodeLength=7)
        try:
            assert plant.env_target is not None and model.env_target is None
            if held:
                ctl = mpc_track.TrackingController(plant, model, K, {"PATH": "held"}, H, seed=5, graph=False)
            else:
                ctl = mpc.Controller(plant, model, K, H, seed=5, graph=False)
            ctl.run(10)
            torch.cuda.synchronize()
            if held:
                assert ctl.launches["plan"] == 10 and ctl.launches["track"] == 10 * H and not ctl.live.any()
                assert _same(ctl.path[:, 0].cpu().numpy(), np.ascontiguousarray(ctl.path[:, -1].cpu().numpy()))
            runs.append([t.cpu().numpy().copy() for t in (plant.state, ctl.nominal, ctl.plant_actions, ctl.cost, model.state)])
        finally:
            model.close()
            plant.close()
    for a, b in zip(*runs):
        assert _same(a, b)
    assert np.abs(runs[0][1]).max() > 0                                    # (the nominal moved)


def test_captured_control_steps_against_eager_ones():
    """One captured control step replayed ten times against ten eager ones, path kind ``exact``, episodes of seven steps: every
    controller tensor (``path`` and ``live`` among them) and both state blocks bit-identical; the graph holds 1 plan and H track
    launches per control step."""
    M, K, H = 4, 16, 6
    runs = []
    for graph in (True, False):
        plant, model = _tasks(M, K, maxEpisodeLength=7)
        try:
            ctl = mpc_track.TrackingController(plant, model, K, {"PATH": "exact"}, H, seed=5, graph=graph, keep_weights=True)
            assert ctl.use_graph == graph
            ctl.run(10)
            torch.cuda.synchronize()
            if graph:
                assert ctl.graph_launches == {"fork": 1, "step": H, "node": H, "update": 1, "plant_step": 1, "plan": 1, "track": H}
            assert ctl.launches == {"fork": 10, "step": 10 * H, "node": 10 * H, "update": 10, "plant_step": 10, "plan": 10, "track": 10 * H}
            assert plant.step_count == 10 and model.step_count == 10 * H
            assert (plant.num_steps, model.num_steps) == (10, 10 * H)          # replayed or eager: the steps the handles took
            runs.append([t.cpu().numpy().copy() for t in ctl.tensors() + [plant.state, model.state]])
            assert ctl.live.any() and any(t is ctl.path for t in ctl.tensors()) and any(t is ctl.live for t in ctl.tensors())
        finally:
            model.close()
            plant.close()
    for a, b in zip(*runs):
        assert _same(a, b)


def test_play_and_the_command_line(tmp_path):
    """(4, 64, 12) through ``mpc.play`` and through ``mpc.py``'s main with the plant's EPISODE_LOG and ENV_TARGET on: the result
    holds ``track``, the report bins by ``param_TARGET_VEL_ALONG``, and each refused combination raises."""
    spec = importlib.util.spec_from_file_location("mpc_cli_track", os.path.join(REPO, "mpc.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    target = "task.env.ENV_TARGET={VEL_ALONG: {values: [0.0, 0.4, -0.4]}, SPAN_ALONG: 0.03}"
    argv = ["plants=4", "samples=64", "horizon=12", "steps=24", "sigma=[0.5, 0.25]", "lambda=0.1", "out=%s" % tmp_path,
            "task.env.EPISODE_LOG=True", "task.env.maxEpisodeLength=10", "task.env.CREATE_PIPE=False", "task.task.vine_randomize=False",
            "seed=3", target]
    out = cli.main(argv + ["track={PATH: exact}"])
    assert out["track"]["PATH"] == "exact" and 0.0 < out["track"]["live_fraction"] < 1.0
    assert out["graphed"] and out["launches"] == {"fork": 24, "step": 24 * 12, "node": 24 * 12, "update": 24, "plant_step": 24,
                                                  "plan": 24, "track": 24 * 12}
    assert out["report"]["episodes"] >= 4 and "param_TARGET_VEL_ALONG" in out["by_param"]
    edges, rate, count = out["by_param"]["param_TARGET_VEL_ALONG"]
    assert int(np.sum(count)) == out["report"]["episodes"] and edges[0] == f32(-0.4) and edges[-1] == f32(0.4)
    assert os.path.exists(out["path"]) and np.isfinite(out["plant_return"]).all()
    plain = cli.main(argv)                                                 # without the key: nothing of it, as before
    assert "track" not in plain and "plan" not in plain["launches"] and "param_TARGET_VEL_ALONG" not in plain["by_param"]
    cfg = _plant_cfg(4, ENV_TARGET={"VEL_ALONG": 0.4, "SPAN_ALONG": 0.03}, EPISODE_LOG=True, EPISODE_LOG_DIR=str(tmp_path / "play"),
                     maxEpisodeLength=10)
    out = mpc.play(cfg, samples=16, horizon=4, steps=12, track={"PATH": "linear"})
    assert out["track"] == {"PATH": "linear", "live_fraction": out["track"]["live_fraction"]} and out["track"]["live_fraction"] > 0.5
    assert out["by_param"] == {}                                           # a constant velocity is no parameter of the report
    for extra, match in ((["policy=x.pth"], "track= together with policy="),
                         (["adapt={params: {DAMPING: [0.005, 0.1]}}"], "track= together with adapt="),
                         (["observe={DELAY: 1}"], "track= together with observe= or filter="),
                         (["observe={DELAY: 1}", "filter={GAIN_Q: 0.5}"], "track= together with observe= or filter="),
                         (["task.env.ENV_TARGET={}"], "track= needs a plant with task.env.ENV_TARGET")):
        with pytest.raises(ConfigError, match=match):
            cli.main(argv + ["track={PATH: exact}"] + extra)
