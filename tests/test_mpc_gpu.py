"""MPC on the GPU (include/vine_mpc.h, utils/mpc.py): the fork field by field and against the rings the step kernel itself
leaves; fork fidelity (samples fed the plant's actions stay the plant, bit for bit); ``u`` and the cost sums against numpy;
the update against ``mpc_replay``; the captured graph against eager launches; ``play`` and the command line; and the
controller against doing nothing.

Shapes (M plants, K samples, H steps): (5, 14, 12) = 70 model envs, two waves, the second partial, K < 64; (2, 300, 3) = K
above one workgroup of the update and no multiple of 256; (1, 2, 1) the degenerate end; model delays 0..8 inside one wave
through a table.  "Bit-identical" is literal: floats are compared as words."""
import numpy as np
import pytest
import torch

from tests.helpers import base_cfg
from vine_robot_isaacgymenvs_amd import abi, load_task_config, native
from vine_robot_isaacgymenvs_amd.utils import env_params, mpc

pytestmark = pytest.mark.gpu

F = abi
SENTINEL = -7777.0
RING = slice(F.VF_FIFO0, F.VF_FIFO0 + 2 * F.MAX_DELAY)
NOT_RING = [f for f in range(F.VF_COUNT) if not F.VF_FIFO0 <= f < F.VF_FIFO0 + 2 * F.MAX_DELAY]
SHAPES = [(5, 14, 12), (2, 300, 3), (1, 2, 1)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    return np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)))


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _cfg(n, pipe=False, **over):
    cfg = base_cfg(n, 0, False, max_episode_length=100, action_delay=1, **over)
    for f in (abi.FLAG_USE_TARGET_REACHED_RESET, abi.FLAG_USE_TIP_LIMIT_HIT_RESET, abi.FLAG_USE_NONZERO_CONTACT_FORCE_RESET,
              abi.FLAG_CREATE_SHELF, abi.FLAG_CREATE_PIPE):
        cfg.set_flag(f, False)
    cfg.set_flag(abi.FLAG_CREATE_PIPE, pipe)
    return cfg


def _env(cfg, table=None):
    from tests.hip_env import HipEnv
    env = HipEnv(cfg)
    if table is not None:
        env_params.check_table(env.lib, env.cfg, table)
        env.table_t = torch.as_tensor(np.ascontiguousarray(table, np.float32)).to(env.dev).contiguous()
        torch.cuda.synchronize(env.dev)
        native.check(env.lib.vine_bind_env_params(env.h, env.table_t.data_ptr()), env.lib)
    return env


class Rig:
    """A plant and a model handle through the C ABI, and the controller's buffers."""

    def __init__(self, M, K, H, pipe=False, table=None, sigma=(0.5, 0.25), lam=0.05, seed=77, model_cfg=None):
        self.M, self.K, self.H, self.N = M, K, H, M * K
        self.lib = native.load()
        self.plant = _env(_cfg(M, pipe))
        self.model = _env(model_cfg if model_cfg is not None else _cfg(M * K, pipe), table)
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

    def warm_plant(self, steps=10, seed=3, scale=1.3):
        """The plant stepped through `steps` random actions (beyond clipActions too); the last eight go into the history,
        most recent first."""
        rng = np.random.default_rng(seed)
        acts = rng.uniform(-scale, scale, (steps, self.M, 2)).astype(np.float32)
        for a in acts:
            self.plant.step(a, sync=False)
        torch.cuda.synchronize()
        self.history.copy_(torch.as_tensor(np.ascontiguousarray(acts[::-1][:F.MAX_DELAY].transpose(1, 0, 2))))
        return acts

    def fork(self, plant=None, model=None, mcfg=None):
        m = model or self.model
        return self.lib.vine_mpc_fork((plant or self.plant).h, m.h, mcfg or self.mcfg, self.plant.progress_t.data_ptr(),
                                      self.nominal.data_ptr(), self.history.data_ptr(), self.tick.data_ptr(),
                                      self.actions.data_ptr(), m.rew_t.data_ptr(), m.reset_t.data_ptr(), m.progress_t.data_ptr(),
                                      self.cost.data_ptr(), self.alive.data_ptr(), self.window.data_ptr(), _stream(self.dev))

    def node(self):
        m = self.model
        rc = self.lib.vine_mpc_scheduled(m.h, self.mcfg, self.nominal.data_ptr(), self.tick.data_ptr(), self.window.data_ptr(),
                                         self.actions.data_ptr(), m.rew_t.data_ptr(), m.reset_t.data_ptr(), self.cost.data_ptr(),
                                         self.alive.data_ptr(), _stream(self.dev))
        assert rc == abi.OK, self.lib.vine_last_error()

    def update(self):
        rc = self.lib.vine_mpc_update(self.model.h, self.mcfg, self.cost.data_ptr(), self.plant.reset_t.data_ptr(),
                                      self.nominal.data_ptr(), self.history.data_ptr(), self.tick.data_ptr(),
                                      self.plant_actions.data_ptr(), self.weights.data_ptr(), _stream(self.dev))
        assert rc == abi.OK, self.lib.vine_last_error()

    def u(self):
        return mpc.sample_actions(self.nominal.cpu().numpy(), self.sigma, self.seed, self.K, self.tick.cpu().numpy(), self.clip)

    def close(self):
        self.plant.close()
        self.model.close()


def _random_nominal(rig, seed=11, scale=0.7):
    rng = np.random.default_rng(seed)
    rig.nominal.copy_(torch.as_tensor(rng.uniform(-scale, scale, (rig.M, rig.H, 2)).astype(np.float32)))


# -------------------------------------------------------------------------------------------------------------- the fork
def test_fork_field_by_field_and_the_ring_against_the_step_kernels_own():
    """(5, 14, 12); model delays 0..8 inside one wave and a RAIL_VELOCITY_SCALE of its own per sample, through a table; the
    model's block full of a sentinel, its step count at 5 while the plant's is 10.  A reference handle with the same table
    steps through the plant's last eight actions and ends at step count 16: its slot (16 - k) mod d holds the command of the
    action handed k steps ago, and the forked handle must hold the same words in slot (5 - k) mod d."""
    M, K, H = SHAPES[0]
    N = M * K
    lib = native.load()
    table = np.repeat(env_params.config_row(lib, _cfg(N))[:, None], N, axis=1)
    delays = np.arange(N) % 9
    table[abi.VP_ACTION_DELAY] = delays
    table[abi.VP_RAIL_VELOCITY_SCALE] = 0.7 + 0.01 * np.arange(N)
    rig, ref = Rig(M, K, H, table=table), _env(_cfg(N), table)
    try:
        acts = rig.warm_plant(10)
        _random_nominal(rig)
        rig.tick.copy_(torch.as_tensor([0, 3, (1 << 32) + 1, 7, 123456789]))
        ref.step_count = 16 - F.MAX_DELAY
        for a in acts[-F.MAX_DELAY:]:
            ref.step(np.repeat(a, K, axis=0), sync=False)
        torch.cuda.synchronize()
        assert ref.step_count == 16 and rig.plant.step_count == 10
        ref_ring = ref.state_t[RING].cpu().numpy()
        rig.model.state_t.fill_(SENTINEL)
        rig.model.step_count = 5
        rig.model.rew_t.fill_(SENTINEL)
        rig.model.reset_t.fill_(1)
        rig.model.progress_t.fill_(-5)
        assert rig.fork() == abi.OK, lib.vine_last_error()
        torch.cuda.synchronize()
        assert rig.model.step_count == 5 and rig.plant.step_count == 10
        pst, st = rig.plant.state_t.cpu().numpy(), rig.model.state_t.cpu().numpy()
        plant_of = np.arange(N) // K
        for f in NOT_RING:
            assert _same(st[f], pst[f][plant_of]), f
        ring = st[RING]
        for e in range(N):
            d = int(delays[e])
            for k in range(1, d + 1):
                for w in (0, 1):
                    assert _same(ring[2 * ((5 - k) % d) + w, e], ref_ring[2 * ((16 - k) % d) + w, e]), (e, k, w)
            assert np.all(ring[2 * d:, e] == np.float32(SENTINEL)), e
        assert np.array_equal(rig.model.progress_t.cpu().numpy(), rig.plant.progress_t.cpu().numpy()[plant_of])
        assert not rig.model.reset_t.any() and not rig.model.rew_t.any() and not rig.cost.any()
        assert np.all(rig.alive.cpu().numpy() == 1) and int(rig.window[0]) == 5
        assert _same(rig.actions.cpu().numpy().reshape(M, K, 2), rig.u()[:, :, 0])
        assert _same(rig.u()[:, 0], rig.nominal.cpu().numpy())
    finally:
        rig.close()
        ref.close()


def test_fork_refusals_name_the_reason():
    M, K, H = 2, 4, 3
    rig = Rig(M, K, H)
    others = []
    try:
        lib = rig.lib

        def refused(rc_want, word, whole=False, **kw):
            lib.vine_set_step_count(None, -1)
            assert rig.fork(**kw) == rc_want, lib.vine_last_error()
            assert lib.vine_last_error() == word if whole else word in lib.vine_last_error(), lib.vine_last_error()

        def other(cfg):
            others.append(_env(cfg))
            return others[-1]

        rnd = _cfg(M * K)
        rnd.set_flag(abi.FLAG_VINE_RANDOMIZE, True)
        refused(abi.ERR_UNSUPPORTED, b"mpc fork: a model handle with vine_randomize is refused (a sample must be a deterministic plant)",
                whole=True, model=other(rnd))
        differ = b"mpc fork: the model handle's CREATE_SHELF / CREATE_PIPE differ from the plant's"
        refused(abi.ERR_UNSUPPORTED, differ, whole=True, model=other(_cfg(M * K, pipe=True)))
        shelf = _cfg(M * K)
        shelf.set_flag(abi.FLAG_CREATE_SHELF, True)
        refused(abi.ERR_UNSUPPORTED, differ, whole=True, model=other(shelf))
        longer = _cfg(M * K)
        longer.max_episode_length = 101
        refused(abi.ERR_INVALID_ARG, b"mpc fork: the model handle's max_episode_length differs from the plant's", whole=True,
                model=other(longer))
        refused(abi.ERR_INVALID_ARG, b"num_plants * samples", model=other(_cfg(M * K + 1)))
        refused(abi.ERR_INVALID_ARG, b"num_plants envs", plant=other(_cfg(M * K)), mcfg=mpc.mpc_config(M * K // 2, 2, H))
        refused(abi.ERR_INVALID_ARG, b"two handles", plant=rig.model)
        for fn in (rig.node, rig.update):                # the node and the update see the model handle only
            rig.mcfg = mpc.mpc_config(M, K + 1, H)
            with pytest.raises(AssertionError, match="num_plants \\* samples"):
                fn()
        rig.mcfg = mpc.mpc_config(M, K, H)
        assert rig.fork() == abi.OK
        torch.cuda.synchronize()
    finally:
        rig.close()
        for o in others:
            o.close()


@pytest.mark.parametrize("pipe", [False, True], ids=["free", "pipe"])
def test_forked_samples_fed_the_plants_actions_stay_the_plant(pipe):
    """sigma = 0: every sample's action is the nominal's.  The plant is fed the same H actions.  Every sample's state-block
    column (the ring compared slot-rotated: the two handles stand at different step counts), rew and progress equal the
    plant's in every bit until the plant's or the sample's first reset."""
    M, K, H = SHAPES[0]
    rig = Rig(M, K, H, pipe=pipe, sigma=(0.0, 0.0))
    try:
        rig.warm_plant(11, seed=5, scale=0.6)
        _random_nominal(rig, seed=13, scale=0.9)
        rig.model.step_count = 3
        assert rig.fork() == abi.OK, rig.lib.vine_last_error()
        nominal = rig.nominal.cpu().numpy()
        plant_of = np.arange(M * K) // K
        live = rig.plant.reset_t.cpu().numpy()[plant_of] == 0             # (a plant whose next step consumes a reset is not forked)
        compared = 0
        for k in range(H):
            assert _same(rig.actions.cpu().numpy(), nominal[plant_of, k])
            rig.model.step_t(rig.actions, sync=False)
            rig.node()
            rig.plant.step(nominal[:, k], sync=False)
            torch.cuda.synchronize()
            cp, cm = rig.plant.step_count, rig.model.step_count
            assert (cp, cm) == (12 + k, 4 + k)
            pst, st = rig.plant.state_t.cpu().numpy(), rig.model.state_t.cpu().numpy()
            for f in NOT_RING:
                assert _same(st[f][live], pst[f][plant_of][live]), (k, f)
            d = 1                                                          # the configuration's ACTION_DELAY
            for w in (0, 1):
                assert _same(st[F.VF_FIFO0 + 2 * ((cm - 1) % d) + w][live], pst[F.VF_FIFO0 + 2 * ((cp - 1) % d) + w][plant_of][live])
            assert _same(rig.model.rew_t.cpu().numpy()[live], rig.plant.rew_t.cpu().numpy()[plant_of][live]), k
            assert np.array_equal(rig.model.progress_t.cpu().numpy()[live], rig.plant.progress_t.cpu().numpy()[plant_of][live])
            assert np.array_equal(rig.model.reset_t.cpu().numpy()[live], rig.plant.reset_t.cpu().numpy()[plant_of][live])
            compared += int(live.sum())
            live &= (rig.model.reset_t.cpu().numpy() == 0) & (rig.plant.reset_t.cpu().numpy()[plant_of] == 0)
        assert compared >= M * K * H // 2                                  # (the comparison did not run empty)
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------------------- u and the cost
def _rollout(rig, runaway=None, nan_at=None):
    """Fork, then H x (step, node) with snapshots: the actions behind the fork and each node, rew and reset behind each step."""
    rig.model.step_count = 7
    assert rig.fork() == abi.OK, rig.lib.vine_last_error()
    if runaway is not None:                              # past RAIL_SOFT_LIMIT: the next step raises its reset
        y = float(rig.model.cfg.rail_soft_limit) + 0.05
        for f in (F.VF_Q0, F.VF_CART_Y, F.VF_PREV_Q0):
            rig.model.state_t[f, runaway] = y
    acts, rews, resets = [rig.actions.cpu().numpy().copy()], [], []
    for k in range(1, rig.H + 1):
        rig.model.step_t(rig.actions, sync=False)
        if nan_at is not None and k == nan_at[0]:
            rig.model.rew_t[nan_at[1]] = float("nan")
        rews.append(rig.model.rew_t.cpu().numpy().copy())
        resets.append(rig.model.reset_t.cpu().numpy().copy())
        rig.node()
        acts.append(rig.actions.cpu().numpy().copy())
    torch.cuda.synchronize()
    return acts, np.stack(rews), np.stack(resets)


def test_actions_and_costs_against_numpy():
    M, K, H = SHAPES[0]
    RUNAWAY, NAN_ENV = 33, 52
    rig, base = Rig(M, K, H), Rig(M, K, H)
    try:
        for r in (rig, base):
            r.warm_plant(10)
            _random_nominal(r, scale=0.5)
            r.tick.copy_(torch.as_tensor([4, 0, (1 << 33) + 9, 2, 1]))
        acts, rews, resets = _rollout(rig, runaway=RUNAWAY, nan_at=(3, NAN_ENV))
        u = rig.u().reshape(M * K, H, 2)
        for k in range(H):
            assert _same(acts[k], u[:, k]), k                              # behind the fork (k = 0) and behind each node
        assert _same(acts[H], acts[H - 1])                                 # the last node writes no action
        assert np.abs(u).max() <= rig.clip and len(np.unique(u[:, 0, 0])) > M * (K - 1) // 2
        cost, alive = mpc.cost_sums(rews, resets)
        assert _same(rig.cost.cpu().numpy(), cost) and np.array_equal(rig.alive.cpu().numpy(), alive)
        # the runaway: its first step raised the reset, that step counted, nothing after it
        assert resets[0][RUNAWAY] == 1 and alive[RUNAWAY] == 0
        assert _same(cost[RUNAWAY], -np.float64(rews[0][RUNAWAY])) and np.isfinite(cost[RUNAWAY])
        assert np.isposinf(cost[NAN_ENV]) and alive[NAN_ENV] == 0
        # every other sum is what a run without the two gives
        _, rews0, resets0 = _rollout(base)
        others = np.setdiff1d(np.arange(M * K), [RUNAWAY, NAN_ENV])
        assert _same(rig.cost.cpu().numpy()[others], base.cost.cpu().numpy()[others])
        assert np.isfinite(base.cost.cpu().numpy()).all() and not _same(cost[RUNAWAY], base.cost.cpu().numpy()[RUNAWAY])
        # one more node outside the window touches nothing
        rig.model.step_t(rig.actions, sync=False)
        rig.node()
        torch.cuda.synchronize()
        assert _same(rig.cost.cpu().numpy(), cost) and _same(rig.actions.cpu().numpy(), acts[H])
        # ... and the NaN's weight is 0
        rig.update()
        torch.cuda.synchronize()
        w = rig.weights.cpu().numpy()
        assert w[NAN_ENV] == 0.0 and np.isfinite(w).all() and w.reshape(M, K).max(axis=1).min() == 1.0
        assert np.isfinite(rig.nominal.cpu().numpy()).all()
    finally:
        rig.close()
        base.close()


@pytest.mark.parametrize("shape", SHAPES[1:], ids=["2x300x3", "1x2x1"])
def test_fork_and_node_at_the_other_shapes(shape):
    """600 model envs (three workgroups, K no multiple of the wave) and two: the fork's copies, `u` and the sums again."""
    M, K, H = shape
    rig = Rig(M, K, H)
    try:
        rig.warm_plant(9, seed=M + K)
        _random_nominal(rig, seed=K, scale=0.5)
        rig.tick.copy_(torch.as_tensor([(1 << 40) + 5, 2][:M]))
        rig.model.state_t.fill_(SENTINEL)
        acts, rews, resets = _rollout(rig)
        u = rig.u().reshape(M * K, H, 2)
        for k in range(H):
            assert _same(acts[k], u[:, k]), k
        cost, alive = mpc.cost_sums(rews, resets)
        assert _same(rig.cost.cpu().numpy(), cost) and np.array_equal(rig.alive.cpu().numpy(), alive)
        assert np.isfinite(cost).all() and int(rig.window[0]) == 7
        pst, st = rig.plant.state_t.cpu().numpy(), rig.model.state_t.cpu().numpy()
        plant_of = np.arange(M * K) // K
        # what no step writes stays the fork's copy: the target; and ring slots 1 and above keep the sentinel (delay 1)
        for f in (F.VF_TARGET_Y, F.VF_TARGET_Z):
            assert _same(st[f], pst[f][plant_of]), f
        assert np.all(st[F.VF_FIFO0 + 2:F.VF_FIFO0 + 2 * F.MAX_DELAY] == np.float32(SENTINEL))
        assert np.array_equal(rig.model.progress_t.cpu().numpy(), rig.plant.progress_t.cpu().numpy()[plant_of] + H)
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------ the update
@pytest.mark.parametrize("shape", SHAPES, ids=["5x14x12", "2x300x3", "1x2x1"])
def test_update_against_the_replay(shape):
    """Costs made by hand on the device; the replay is fed the device's own costs and nominal.  Weights within 1e-12
    relative (the argument of exp is formed identically in float64, the device's exp is within an ulp, the sums differ in
    order over at most 300 terms); the new nominal and the plant's action within one float32 ulp at clipActions
    (2^-23 * clip: one float32 rounding of two float64 values that agree to 1e-12); history, tick, the reset branch and the
    all-infinite branch exact; two runs the same bits."""
    M, K, H = shape
    rig = Rig(M, K, H, sigma=(0.5, 0.75))
    try:
        rng = np.random.default_rng(M * 1000 + K)
        cost = rng.uniform(0.0, 0.6, (M, K))
        cost[0, rng.integers(0, K)] = np.inf
        reset = np.zeros(M, dtype=np.int64)
        if M >= 2:
            cost[1, :] = np.inf                                           # no finite cost: the nominal stays
        if M >= 3:
            reset[2] = 1                                                   # the plant's next step only consumes its reset
            cost[3, 1:] += 50.0                                            # one sample far below the rest
        nominal = rng.uniform(-0.9, 0.9, (M, H, 2)).astype(np.float32)
        history = rng.uniform(-1, 1, (M, F.MAX_DELAY, 2)).astype(np.float32)
        tick = rng.integers(0, 1 << 34, M)
        outs = []
        for _ in range(2):
            rig.cost.copy_(torch.as_tensor(cost.reshape(-1)))
            rig.nominal.copy_(torch.as_tensor(nominal))
            rig.history.copy_(torch.as_tensor(history))
            rig.tick.copy_(torch.as_tensor(tick))
            rig.plant.reset_t.copy_(torch.as_tensor(reset))
            rig.update()
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy().copy() for t in (rig.nominal, rig.plant_actions, rig.history, rig.tick, rig.weights)])
        for a, b in zip(*outs):
            assert _same(a, b)
        got_nominal, got_act, got_history, got_tick, got_w = outs[0]
        r = mpc.mpc_replay(nominal, cost.reshape(-1), rig.sigma, rig.lam, rig.seed, tick, rig.clip, reset, history)
        w = got_w.reshape(M, K)
        assert np.all(np.abs(w - r["weights"]) <= 1e-12 * r["weights"])
        ulp = 2.0 ** -23 * rig.clip
        assert np.abs(got_nominal.astype(np.float64) - r["nominal"]).max() <= ulp
        assert np.abs(got_act.astype(np.float64) - r["plant_actions"]).max() <= ulp
        assert _same(got_history[:, 1:], history[:, :-1]) and _same(got_history[:, 0], got_act)
        assert np.array_equal(got_tick, tick + 1)
        assert _same(got_nominal[:, -1], got_nominal[:, -2]) if H > 1 else True
        if M >= 2:                                                         # all infinite: exact
            assert not w[1].any() and _same(got_act[1], nominal[1, 0]) and _same(got_nominal[1, :-1], nominal[1, 1:])
            assert _same(got_nominal[1, -1], nominal[1, -1])
        if M >= 3:
            assert _same(got_act[2], np.zeros(2, np.float32)) and _same(got_nominal[2], np.zeros((H, 2), np.float32))
            assert _same(got_act[3], r["u"][3, 0, 0]) and w[3, 0] == 1.0 and not w[3, 1:].any()
        assert w[0].max() == 1.0 and (w[0] == 0.0).sum() == 1
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------ the task classes
def _plant_cfg(M, seed=9, **env_over):
    cfg = load_task_config("Vine5LinkMovingBase", overrides=["num_envs=%d" % M])
    cfg["seed"] = seed
    cfg["task"]["vine_randomize"] = False
    cfg["env"].update(CREATE_PIPE=False, CREATE_SHELF=False)
    cfg["env"].update(env_over)
    return cfg


def _pair(M, K, H, cost=None, plant_over=None, **ctl):
    cfg = _plant_cfg(M, **(plant_over or {}))
    plant = mpc.make_task(cfg)
    model = mpc.make_task(mpc.model_config(cfg, M, K, cost))
    return plant, model, mpc.Controller(plant, model, K, H, **ctl)


def test_captured_control_steps_against_eager_ones(tmp_path):
    """Four captured control steps replayed five times against twenty eager ones: every controller tensor, both state blocks
    and the plant's episode-log rows bit-identical.  Episodes of ten steps, so that rows are written and resets consumed."""
    M, K, H = 4, 16, 6
    runs = []
    for tag, kw in (("graph", dict(graph=True, graph_steps=4)), ("eager", dict(graph=False))):
        over = dict(maxEpisodeLength=10, EPISODE_LOG=True, EPISODE_LOG_CAPACITY=4096, EPISODE_LOG_DIR=str(tmp_path / tag))
        plant, model, ctl = _pair(M, K, H, plant_over=over, seed=5, keep_weights=True, **kw)
        try:
            assert ctl.use_graph == (tag == "graph")
            ctl.run(20)
            torch.cuda.synchronize()
            if tag == "graph":
                assert ctl.graph_launches == {"fork": 4, "step": 4 * H, "node": 4 * H, "update": 4, "plant_step": 4}
            assert ctl.launches == {"fork": 20, "step": 20 * H, "node": 20 * H, "update": 20, "plant_step": 20}
            assert plant.step_count == 20 and model.step_count == 20 * H and int(ctl.tick[0]) == 20
            assert (plant.num_steps, model.num_steps) == (20, 20 * H)          # replayed or eager: the steps the handles took
            plant.episode_log.harvest()
            rows = plant.episode_log.rows()
            runs.append(([t.cpu().numpy().copy() for t in ctl.tensors()], plant.state.cpu().numpy().copy(),
                         model.state.cpu().numpy().copy(), {k: np.asarray(v).copy() for k, v in rows.items()}))
        finally:
            model.close()
            plant.close()
    (ta, pa, ma, ra), (tb, pb, mb, rb) = runs
    for a, b in zip(ta, tb):
        assert _same(a, b)
    assert _same(pa, pb) and _same(ma, mb)
    assert len(ra["env"]) >= M and set(ra) == set(rb)
    for k in ra:
        assert _same(ra[k], rb[k]), k
    assert np.abs(ta[0]).max() > 0                                         # (the nominal moved)


def test_play_and_the_command_line(tmp_path):
    """(4, 64, 12) through ``mpc.py``'s main with the plant's EPISODE_LOG on: the .npz is written and the report is the
    log's; with ``model_params`` the model handle has a table bound and takes the one-lane kernel."""
    import importlib.util
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mpc_cli", os.path.join(repo, "mpc.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    argv = ["plants=4", "samples=64", "horizon=12", "steps=24", "sigma=[0.5, 0.25]", "lambda=0.1", "out=%s" % tmp_path,
            "cost={POSITION_REWARD_WEIGHT: 1.0}", "task.env.EPISODE_LOG=True", "task.env.maxEpisodeLength=10",
            "task.env.CREATE_PIPE=False", "task.task.vine_randomize=False", "seed=3"]
    out = cli.main(argv)
    assert out["path"] and os.path.dirname(out["path"]) == str(tmp_path) and os.path.exists(out["path"])
    assert out["report"]["episodes"] >= 4 and np.isfinite(out["report"]["reached_ever_rate"])
    assert out["graphed"] and out["launches"] == {"fork": 24, "step": 24 * 12, "node": 24 * 12, "update": 24, "plant_step": 24}
    assert not out["model_table_bound"] and out["plant_return"].shape == (4,) and np.isfinite(out["plant_return"]).all()
    with np.load(out["path"], allow_pickle=True) as z:
        assert len(z["env"]) == out["report"]["episodes"]
    out2 = cli.main(argv + ["model_params={DAMPING: [0.01, 0.05], ACTION_DELAY: {values: [1, 2]}}", "steps=6"])
    assert out2["model_table_bound"] and out2["model_step_kernel"] == "vine_step_kernel"
    assert np.isfinite(out2["plant_return"]).all()


def test_set_model_params_repeats_each_plants_value_over_its_samples():
    M, K, H = 3, 5, 2
    cfg = _plant_cfg(M)
    mcfg = mpc.model_config(cfg, M, K)
    mcfg["env"]["ENV_PARAMS"] = {"DAMPING": [0.01, 0.05]}
    plant, model = mpc.make_task(cfg), mpc.make_task(mcfg)
    try:
        ctl = mpc.Controller(plant, model, K, H, graph=False)
        ctl.set_model_params({"DAMPING": np.array([0.01, 0.02, 0.03]), "ACTION_DELAY": 2})
        table = model.env_params.cpu().numpy()
        assert _same(table[abi.VP_DAMPING], np.repeat(np.float32([0.01, 0.02, 0.03]), K))
        assert np.all(table[abi.VP_ACTION_DELAY] == 2)
        with pytest.raises(ValueError, match="DAMPING"):
            ctl.set_model_params({"DAMPING": np.zeros(M * K)})
        ctl.run(2)
        ctl.history.fill_(0.5)
        ctl.reset_plants([1])
        torch.cuda.synchronize()
        assert not ctl.nominal[1].any() and not ctl.history[1].any() and ctl.history[0].all()
        assert int(plant.progress_buf[1]) == 0
    finally:
        model.close()
        plant.close()


def test_it_controls():
    """Free space, the Position and Rail Limit reward weights 1 and every other weight 0 on both handles, no target-reached
    reset, ACTION_DELAY 1; (4, 64, 12), sigma 0.5, lambda 0.05, 60 control steps from one plant step on action zero.  The
    summed plant reward under MPC must exceed that under sigma = 0 (action always zero) on each of the four plants: the
    float64 oracle with numpy normals gave at least 2.3x there."""
    M, K, H = 4, 64, 12
    weights = {k: 0.0 for k in _plant_cfg(M)["env"] if k.endswith("_REWARD_WEIGHT")}
    weights.update(POSITION_REWARD_WEIGHT=1.0, RAIL_LIMIT_REWARD_WEIGHT=1.0)
    over = dict(weights, USE_TARGET_REACHED_RESET=False, ACTION_DELAY=1)
    totals = {}
    for sigma in (0.5, 0.0):
        plant, model, ctl = _pair(M, K, H, cost=weights, plant_over=over, sigma=sigma, lam=0.05, seed=1)
        try:
            plant.step_into(ctl.plant_actions, ctl.plant_obs)              # one plant step on action zero
            total = torch.zeros(M, dtype=torch.float64, device=plant.device)
            for _ in range(60):
                ctl.run(1)
                total += plant.rew_buf
            totals[sigma] = total.cpu().numpy()
            if sigma == 0.0:
                assert not ctl.plant_actions.any() and not ctl.nominal.any()
        finally:
            model.close()
            plant.close()
    print("summed plant reward: MPC %s; action zero %s" % (totals[0.5], totals[0.0]))
    assert np.all(totals[0.5] > totals[0.0]), (totals[0.5], totals[0.0])
