"""ENV_INERTIA on the GPU: vine_step_kernel's third variant (include/vine_env_inertia.h: the parameter table and the inertia
table) against the same kernel without a table, against uniform handles created with the masses in their VineConfig, against
the oracle; set_env_params and a captured graph; the binding rules; SYSID over masses; the entry points.

The shapes are those of tests/test_env_params_gpu.py: 70 envs = two waves, the second partial; mass sets cycling 0..8 inside
one wave; 12-step episodes, so that resets and time-outs occur inside every 40-step run.  "Bit-identical" is literal: float
tensors are compared as 32-bit words."""
import ctypes as C
import glob

import numpy as np
import pytest
import torch

from oracle import vine_oracle as vo
from tests.env_inertia_sets import NUM_SETS, set_cfg, table_of
from tests.helpers import base_cfg, random_state
from tests.step_reference import composite
from tests.test_env_params_gpu import (MAX_LEN, N, T, _make_env, actions_for, assert_bit_equal, bits, case_cfg, own_table, rollout,
                                       saw_resets_and_timeouts)
from tests.test_hip_parity import QPOS, compare_step
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Lane():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    from tests.hip_env import HipEnv as H

    def upload(self, table, rows, check):
        check(self.lib, self.cfg, table)
        t = torch.as_tensor(np.ascontiguousarray(table, np.float32)).to(self.dev).contiguous()
        assert t.shape == (rows, self.n)
        torch.cuda.synchronize(self.dev)
        return t

    def bind(self, table):
        """The parameter table (None unbinds); returns the library's answer."""
        self.table_t = None if table is None else upload(self, table, abi.VP_COUNT, env_params.check_table)
        return self.lib.vine_bind_env_params(self.h, None if table is None else self.table_t.data_ptr())

    def bind_inertia(self, table):
        self.inertia_t = None if table is None else upload(self, table, abi.VI_COUNT, env_params.check_inertia_table)
        return self.lib.vine_bind_env_inertia(self.h, None if table is None else self.inertia_t.data_ptr())

    def bind_both(self, params, inertia):
        assert self.bind(params) == abi.OK and self.bind_inertia(inertia) == abi.OK
        assert self.lib.vine_env_params_bound(self.h) == 1 and self.lib.vine_env_inertia_bound(self.h) == 1

    def kernel_name(self):
        return self.lib.vine_step_kernel_name(self.h).decode()

    return type("HipEnvLane", (H,), {"kernel": "lane", "bind": bind, "bind_inertia": bind_inertia, "bind_both": bind_both,
                                     "kernel_name": kernel_name})


def own_inertia(env):
    return np.repeat(env_params.inertia_config_row(env.lib, env.cfg)[:, None], env.n, axis=1)


def inertia_case_cfg(case):
    if case == "extras":              # joint stiffness and link angular damping on: the substep reads I[] itself
        cfg = base_cfg(N, 0, False, max_episode_length=MAX_LEN, seed=24)
        cfg.stiffness, cfg.link_angular_damping = 0.05, 0.02
        return cfg
    return case_cfg(case)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", ["free-obs0", "free-obs1", "shelf", "pipe", "rand-delay1", "extras"])
def test_own_row_tables_change_nothing(Lane, case):
    """An inertia table filled with the configuration's own row, beside a parameter table filled with the configuration's
    own row, against the unbound one-lane kernel: same seed, same actions, 40 steps; observations, rewards, flags, counters
    and the whole state block after every step, bit for bit."""
    ref_env = Lane(inertia_case_cfg(case))
    assert ref_env.kernel_name() == "vine_step_kernel"
    ref = rollout(ref_env, actions_for(N, T))
    ref_env.close()
    assert saw_resets_and_timeouts(ref), case
    env = Lane(inertia_case_cfg(case))
    if case == "extras":
        assert env.cfg.stiffness != 0.0 and env.cfg.link_angular_damping != 0.0
    env.bind_both(own_table(env), own_inertia(env))
    assert env.kernel_name() == "vine_step_kernel"
    got = rollout(env, actions_for(N, T))
    env.close()
    assert_bit_equal(got, ref, what=case)


def test_extras_path_reads_the_inertias_from_the_table(Lane):
    """With link angular damping on, a table that differs from the configuration's in LINK_INERTIA[2] of env 9 alone (its
    ADIAG[2] follows) moves env 9 and no other: the term cad * I_i * w_i comes from the table."""
    ref_env = Lane(inertia_case_cfg("extras"))
    ref = rollout(ref_env, actions_for(N, 8))
    ref_env.close()
    env = Lane(inertia_case_cfg("extras"))
    table = own_inertia(env)
    table[abi.VI_LINK_INERTIA0 + 2, 9] *= np.float32(40.0)
    table = env_params.derive_inertia(env.lib, env.cfg, table)
    env.bind_both(own_table(env), table)
    got = rollout(env, actions_for(N, 8))
    env.close()
    assert_bit_equal(got, ref, envs=np.array([e for e in range(N) if e != 9]), what="envs other than 9")
    assert not np.array_equal(bits(got["state"][:, abi.VF_Q0:abi.VF_Q0 + 6, 9]), bits(ref["state"][:, abi.VF_Q0:abi.VF_Q0 + 6, 9]))


# ---------------------------------------------------------------------------------------------------------------- 2
def het_cfg():
    cfg = base_cfg(N, 0, True, max_episode_length=MAX_LEN, seed=31)
    cfg.obs_noise_std, cfg.action_noise_std, cfg.dyn_scale_min, cfg.dyn_scale_max = 0.01, 0.02, 0.9, 1.1
    return cfg


def test_nine_plants_in_one_batch_equal_nine_uniform_handles(Lane):
    """Env e of the heterogeneous handle (mass set e % 9: all 31 rows differ inside one wave) against env e of the unbound
    handle created with set e % 9 in its VineConfig, same seed, same actions: bit for bit, every step, 40 steps."""
    env = Lane(het_cfg())
    table = table_of(env.lib, env.cfg, N)
    for r in range(abi.VI_COUNT):
        assert len(set(table[r, :NUM_SETS].tolist())) == NUM_SETS, abi.ENV_INERTIA_ROW_NAMES[r]
    env.bind_both(own_table(env), table)
    het = rollout(env, actions_for(N, T, seed=4))
    env.close()
    assert saw_resets_and_timeouts(het)
    for g in range(NUM_SETS):
        env = Lane(set_cfg(het_cfg(), g))
        assert np.array_equal(bits(own_inertia(env)[:, 0]), bits(table[:, g]))
        uni = rollout(env, actions_for(N, T, seed=4))
        env.close()
        assert_bit_equal(het, uni, envs=np.arange(g, N, NUM_SETS), what="mass set %d" % g)
    assert not np.array_equal(het["state"][-1][abi.VF_Q0:abi.VF_Q0 + 6, 0], het["state"][-1][abi.VF_Q0:abi.VF_Q0 + 6, 1])


# ---------------------------------------------------------------------------------------------------------------- 3
def _composite(oracles):
    """Env e of oracle e % 9, as one oracle-like object for compare_step (tests/step_reference.py)."""
    assert len(oracles) == NUM_SETS
    return composite(oracles, N)


# single_step_case's tolerances for the one-lane kernel (tests/test_hip_parity.py holds them as literals inside the function,
# as tests/test_env_params_gpu.py restates them; compare_step and QPOS are imported)
@pytest.mark.parametrize("precision,tol", [("f32", (2e-5, 2e-3, 2e-3)), ("f64", (1e-4, 1e-2, 1e-2))])
def test_heterogeneous_step_matches_nine_oracles(Lane, precision, tol):
    """One step from a random mid-episode state with resets and time-outs seeded as test_hip_parity's seed_both does,
    randomisation on, against nine OracleEnvs (one per mass set) at single_step_case's tolerances."""
    cfg = het_cfg()
    rng = np.random.default_rng(9)
    hip = Lane(cfg)
    hip.bind_both(own_table(hip), table_of(hip.lib, cfg, N))
    oracles = [vo.OracleEnv(set_cfg(cfg, g), precision) for g in range(NUM_SETS)]
    st = random_state(rng, N, cfg)
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
    hip.bind_both(own_table(hip), table_of(hip.lib, cfg, N))
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
OWN_SPEC = {"LINK_MASS": 1.0}          # binds both tables, every column the configuration's own


def _state_words(env):
    return env.state.clone().view(torch.int32).cpu().numpy()


def test_set_env_params_cart_mass_of_one_env_moves_that_env_only():
    """Env 5's CART_MASS alone is changed through set_env_params: env 5 leaves the unchanged run, every other env stays on it
    bit for bit (a transposed or mis-strided table, or a derived row written to the wrong env, would move others)."""
    acts = actions_for(N, 8, seed=7).cuda()
    runs = []
    for change in (False, True):
        env = _make_env(N, OWN_SPEC)
        try:
            assert env.env_inertia.shape == (abi.VI_COUNT, N) and tuple(env.env_inertia_names) == abi.ENV_INERTIA_ROW_NAMES
            assert np.array_equal(env.env_params.cpu().numpy(), np.repeat(env_params.config_row(env._lib, env._vcfg)[:, None], N, axis=1))
            if change:
                cart = np.full(N, float(env._vcfg.cart_mass))
                cart[5] = 0.7
                before = env.env_inertia.clone()
                env.set_env_params({"CART_MASS": cart})
                after = env.env_inertia.cpu().numpy()
                assert after[abi.VI_CART_MASS, 5] == np.float32(0.7)
                assert after[abi.VI_MTOT, 5] != before[abi.VI_MTOT, 5].item()          # re-derived on the host
                changed = np.argwhere(after != before.cpu().numpy())
                assert sorted(set(changed[:, 1].tolist())) == [5] and sorted(set(changed[:, 0].tolist())) == [abi.VI_CART_MASS, abi.VI_MTOT]
                env_params.check_inertia_table(env._lib, env._vcfg, after)
            obs = torch.zeros(8, N, env.num_obs, device="cuda")
            states = []
            for k in range(8):
                env.step_into(acts[k], obs[k])
                states.append(_state_words(env))
            torch.cuda.synchronize()
            runs.append((obs.view(torch.int32).cpu().numpy(), np.stack(states)))
            if change:
                with pytest.raises(ValueError, match="CART_MASS of env 3 "):
                    bad = cart.copy()
                    bad[3] = -1.0
                    env.set_env_params({"CART_MASS": bad, "DAMPING": 0.5})
                assert np.array_equal(env.env_inertia.cpu().numpy(), after)             # a refusal writes nothing, of either table
                assert torch.all(env.env_params[abi.VP_DAMPING] == float(np.float32(env._vcfg.damping)))
                with pytest.raises(ValueError, match=r"LINK_INERTIA\[1\]"):
                    env.set_env_params({"LINK_INERTIA[1]": -1e-6})
                env.set_env_params({"LINK_MASS[2]": 0.0061})                            # a raw primary row: the value itself
                assert torch.all(env.env_inertia[abi.VI_LINK_MASS0 + 2] == np.float32(0.0061))
        finally:
            env.close()
    (obs_a, st_a), (obs_b, st_b) = runs
    others = np.array([e for e in range(N) if e != 5])
    assert np.array_equal(obs_a[:, others], obs_b[:, others]) and np.array_equal(st_a[:, :, others], st_b[:, :, others])
    assert not np.array_equal(obs_a[:, 5], obs_b[:, 5])
    assert not np.array_equal(st_a[:, abi.VF_Q0:abi.VF_Q0 + 6, 5], st_b[:, abi.VF_Q0:abi.VF_Q0 + 6, 5])


def test_captured_steps_read_the_inertia_table_at_replay():
    """Four steps with both tables bound captured in a graph, replayed twice with LINK_MASS rewritten by set_env_params in
    between (ten primary rows and their derived rows, in place), against the same eight steps issued eagerly: bit for bit."""
    n = N
    acts = actions_for(n, 8, seed=7).cuda()
    new_factor = torch.linspace(0.8, 1.3, n)
    spec = {"CART_MASS": [0.35, 0.7], "LINK_MASS": 1.0}

    def between(env):
        ptr = env.env_inertia.data_ptr()
        env.set_env_params({"LINK_MASS": new_factor})
        assert env.env_inertia.data_ptr() == ptr                                            # rewritten in place
        want = (np.float64(np.float32(env._vcfg.link_mass[4])) * new_factor.numpy().astype(np.float64)).astype(np.float32)
        assert np.array_equal(env.env_inertia[abi.VI_LINK_MASS0 + 4].cpu().numpy(), want)
        env_params.check_inertia_table(env._lib, env._vcfg, env.env_inertia.cpu().numpy())

    eager = _make_env(n, spec)
    obs_e = torch.zeros(8, n, eager.num_obs, device="cuda")
    for k in range(8):
        if k == 4:
            between(eager)
        eager.step_into(acts[k], obs_e[k])
    torch.cuda.synchronize()

    graphed = _make_env(n, spec)
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
    plain = _make_env(n, spec)
    obs_p = torch.zeros(8, n, plain.num_obs, device="cuda")
    for k in range(8):
        plain.step_into(acts[k], obs_p[k])
    torch.cuda.synchronize()
    assert torch.equal(obs_p[:4], obs_e[:4]) and not torch.equal(obs_p[4:], obs_e[4:])
    for e in (eager, graphed, plain):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_binding_rules_and_unbinding_leaves_no_trace(Lane):
    """512 envs on the four-lane kernel.  An inertia table without a parameter table is refused; with both bound the
    one-lane kernel steps the handle, the fused rollout and evaluation steps answer VINE_ERR_UNSUPPORTED, and unbinding the
    parameter table is refused; after unbinding inertia, then parameters, 8 further steps equal those of a handle never bound
    that starts from the same state and step count, bit for bit (randomisation on: the step count keys every draw)."""
    n = 512
    Quad = type("HipEnvQuad", (Lane,), {"kernel": "quad"})
    cfg = base_cfg(n, 0, True, max_episode_length=MAX_LEN, seed=41)
    cfg.obs_noise_std, cfg.action_noise_std, cfg.dyn_scale_min, cfg.dyn_scale_max = 0.01, 0.02, 0.9, 1.1
    lib = native.load()
    acts = actions_for(n, 16, seed=6)
    a = Quad(cfg)
    assert a.kernel_name() == "vine_step_quad_kernel" and lib.vine_step_rollout_blocks(a.h) == 8
    rollout(a, acts[:4])
    plants = table_of(lib, a.cfg, n)
    assert a.bind_inertia(plants) == abi.ERR_UNSUPPORTED and "vine_bind_env_params" in lib.vine_last_error().decode()
    assert lib.vine_env_inertia_bound(a.h) == 0 and a.kernel_name() == "vine_step_quad_kernel"
    a.bind_both(own_table(a), plants)
    assert a.kernel_name() == "vine_step_kernel" and a.step_count == 4
    assert lib.vine_step_rollout_blocks(a.h) == 0 and lib.vine_step_eval_rows(a.h) == 0
    assert lib.vine_bind_env_params(a.h, None) == abi.ERR_UNSUPPORTED and "vine_bind_env_inertia" in lib.vine_last_error().decode()
    assert lib.vine_env_params_bound(a.h) == 1 and lib.vine_env_inertia_bound(a.h) == 1
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
    assert a.bind_inertia(None) == abi.OK and lib.vine_env_inertia_bound(a.h) == 0
    assert a.kernel_name() == "vine_step_kernel" and a.step_count == 8              # the parameter table still routes
    assert a.bind(None) == abi.OK
    assert a.kernel_name() == b.kernel_name() == "vine_step_quad_kernel" and lib.vine_step_rollout_blocks(a.h) == 8
    assert a.step_count == 8
    ra_, rb_ = rollout(a, acts[8:]), rollout(b, acts[8:])
    assert a.step_count == b.step_count == 16
    a.close(); b.close()
    assert_bit_equal(ra_, rb_, what="after unbinding")
    assert saw_resets_and_timeouts(rb_)


# ---------------------------------------------------------------------------------------------------------------- 6
H = 12
TRUTH = {"CART_MASS": 0.55, "LINK_MASS": 1.2, "DAMPING": 0.035}
CART_VALUES = [0.35, 0.4, 0.55, 0.7]
TRUE_ENV, CART_ENV = 17, 18


@pytest.fixture(scope="module")
def recorded():
    """A log from a plant with a cart of 0.55 kg (the configuration's: 0.4) and links 1.2 times the configuration's: 70 envs
    that all carry TRUTH, pinned to test_sysid_gpu's hand-made row 0, 40 steps on its action table, env 3 recorded by
    vine_record behind every step.  Returns the log [41, RECORD_FIELDS] and env 3's columns of both tables."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
    from tests.test_sysid_gpu import _hand_made_log, _stream, _task_cfg
    from vine_robot_isaacgymenvs_amd.utils import sysid
    from vine_robot_isaacgymenvs_amd.utils.trajectory import record_config
    log0 = _hand_made_log()
    A = sysid.candidate_task(_task_cfg(N), TRUTH, N, T)
    try:
        assert A.step_kernel_name == "vine_step_kernel" and A._lib.vine_env_inertia_bound(A._handle) == 1
        ev = sysid.Evaluator(A, log0, T, graph=False)
        rcfg = record_config(A._lib, T, T, 1)
        envs = torch.as_tensor([3], dtype=torch.int32, device=A.device)
        ring = torch.zeros((T, 1, abi.RECORD_FIELDS), device=A.device)
        steps = torch.zeros(T, dtype=torch.int64, device=A.device)
        ev.pin(0)
        for k in range(T):
            A.step_into(ev.actions, ev.obs)
            native.check(A._lib.vine_record(A._handle, rcfg, k, envs.data_ptr(), ev.actions.data_ptr(), A.rew_buf.data_ptr(),
                                            A.reset_buf.data_ptr(), A.progress_buf.data_ptr(), A.timeout_buf.data_ptr(),
                                            ring.data_ptr(), steps.data_ptr(), _stream(A.device)), A._lib)
            ev.node()
        torch.cuda.synchronize()
        rows = ring[:, 0].cpu().numpy()
        truth = A.env_params_of([3])[:, 0].astype(np.float32)
        itruth = A.env_inertia_of([3])[:, 0].astype(np.float32)
        ibase = env_params.inertia_config_row(A._lib, A._vcfg)
    finally:
        A.close()
    log = np.concatenate([log0[:1], rows])
    assert np.array_equal(log[:, abi.VRF_PROGRESS], np.arange(T + 1)) and not log[:, abi.VRF_RESET].any()
    assert sysid.windows(log, H, H) == [0, 12, 24]
    assert itruth[abi.VI_CART_MASS] == np.float32(0.55) != ibase[abi.VI_CART_MASS]
    assert itruth[abi.VI_LINK_MASS0 + 4] == np.float32(np.float64(ibase[abi.VI_LINK_MASS0 + 4]) * 1.2)
    return log, truth, itruth


def test_sysid_true_plant_scores_zero_and_a_cart_mass_error_scores_more(recorded):
    """70 candidates over the windows 0, 12, 24 of the recorded log (H = 12): the true plant at env 17 has error 0.0; env 18
    differs in CART_MASS alone (0.4 kg, a listed value, against the true 0.55 kg) and scores strictly more; every other
    column differs in cart mass and link factor.

    Measured on an MI355X: err[17] = 0.0; err[18] = 1.04e-05 (summed squared joint-position error over 36 compared rows);
    the smallest error among the 68 columns that differ in cart mass and link factor 1.22e-05."""
    from tests.test_sysid_gpu import _task_cfg
    from vine_robot_isaacgymenvs_amd.utils import sysid
    log, truth, itruth = recorded
    B = sysid.candidate_task(_task_cfg(N), TRUTH, N, H)
    try:
        ibase = env_params.inertia_config_row(B._lib, B._vcfg)
        e = np.arange(N)
        table = np.repeat(itruth[:, None], N, axis=1)
        table[abi.VI_CART_MASS] = (0.35 + 0.01 * e).astype(np.float32)
        for i in range(abi.NUM_LINKS):
            for first in (abi.VI_LINK_MASS0, abi.VI_LINK_INERTIA0):
                table[first + i] = (np.float64(ibase[first + i]) * (0.8 + 0.01 * e)).astype(np.float32)
        table[:, TRUE_ENV] = table[:, CART_ENV] = itruth
        table[abi.VI_CART_MASS, CART_ENV] = CART_VALUES[1]
        table = env_params.derive_inertia(B._lib, B._vcfg, table)
        assert sum(np.array_equal(table[:, c], itruth) for c in range(N)) == 1
        B.set_env_params({B.env_inertia_names[r]: table[r] for r in range(abi.VI_PRIMARY_COUNT)})
        assert np.array_equal(bits(B.env_inertia.cpu().numpy()), bits(table))
        assert np.array_equal(B.env_params_of([TRUE_ENV])[:, 0].astype(np.float32), truth)
        ev = sysid.Evaluator(B, log, H, graph=False)
        err = ev.evaluate([0, 12, 24])
        print("\nerr[true] = %r, err[CART_MASS 0.4 for 0.55] = %r, smallest other = %r" % (
            err[TRUE_ENV], err[CART_ENV], np.delete(err, [TRUE_ENV, CART_ENV]).min()))
        assert ev.alive.cpu().numpy().all()
        assert err[TRUE_ENV] == 0.0
        assert err[CART_ENV] > 0.0 and np.isfinite(err[CART_ENV])
        others = np.delete(err, TRUE_ENV)
        assert (others > 0.0).all() and np.isfinite(others).all()
    finally:
        B.close()


def test_sysid_fit_returns_the_true_masses(recorded, tmp_path, capsys):
    """fit over 512 candidates with lists that contain the truth for CART_MASS and LINK_MASS together with DAMPING
    (4 x 4 x 8 = 128 combinations, each four times in the batch): the true values, error 0."""
    from tests.test_sysid_gpu import _task_cfg
    from vine_robot_isaacgymenvs_amd.utils import sysid
    from vine_robot_isaacgymenvs_amd.utils.trajectory import write_trajectory_mat
    log, truth, itruth = recorded
    path = write_trajectory_mat(str(tmp_path / "log.mat"), log, np.arange(len(log)), 0.03332, env=3)
    spec = {"CART_MASS": {"values": CART_VALUES}, "LINK_MASS": {"values": [0.8, 1.0, 1.2, 1.4]},
            "DAMPING": {"values": [0.01, 0.02, 0.03, 0.035, 0.04, 0.05, 0.06, 0.08]}}
    out = sysid.fit(_task_cfg(512), path, spec, num_envs=512, iterations=2, horizon=H, stride=H, seed=42,
                    directory=str(tmp_path), time_str="t")
    assert out["starts"] == [0, 12, 24]
    assert out["best_error"] == 0.0
    assert np.array_equal(out["best"], truth) and np.array_equal(bits(out["inertia_best"]), bits(itruth))
    assert out["best"][abi.VP_DAMPING] == np.float32(0.035) and out["inertia_best"][abi.VI_CART_MASS] == np.float32(0.55)
    assert out["errors"][0] == 0.0 and np.array_equal(bits(out["inertia"][:, 0]), bits(itruth))      # column 0: the best of both
    z = np.load(str(tmp_path / "t_sysid.npz"))
    assert z["table"].shape == (abi.VP_COUNT, 512) and z["inertia"].shape == (abi.VI_COUNT, 512)
    assert np.array_equal(bits(z["inertia_best"]), bits(itruth)) and list(z["env_inertia_names"]) == list(abi.ENV_INERTIA_ROW_NAMES)
    assert np.array_equal(z["best"], truth) and float(z["best_error"]) == 0.0
    text = capsys.readouterr().out
    assert text.count("sysid iteration") == 2 and "CART_MASS" in text and "LINK_MASS[4]" in text and "LINK_INERTIA[0]" in text


# ---------------------------------------------------------------------------------------------------------------- 7
def test_train_and_play_entries_with_masses(tmp_path, monkeypatch, capsys):
    """Two training iterations (horizon 8) at 512 envs through train.py's entry with CART_MASS and LINK_MASS ranges,
    EPISODE_LOG and RECORD_TRAJECTORIES on, then test=True on the checkpoint: the inertia table in the .npz, the recorded
    env's eleven masses in the MAT file, a reached-rate per mass name, the player's stock path."""
    import scipy.io
    from vine_robot_isaacgymenvs_amd.learning.player import PpoPlayerContinuous
    from vine_robot_isaacgymenvs_amd.train import main
    from vine_robot_isaacgymenvs_amd.utils import episodes
    monkeypatch.chdir(tmp_path)
    common = ["task=Vine5LinkMovingBase", "num_envs=512", "headless=True", "experiment=masses", "task.env.CREATE_PIPE=False",
              "task.env.maxEpisodeLength=%d" % MAX_LEN,
              "task.env.ENV_PARAMS={CART_MASS: [0.35, 0.7], LINK_MASS: [0.8, 1.3]}", "task.env.EPISODE_LOG=True",
              "task.env.EPISODE_LOG_CAPACITY=32768", "task.env.EPISODE_LOG_DIR=" + str(tmp_path / "train")]
    main(common + ["minibatch_size=2048", "max_iterations=2", "train.params.config.horizon_length=8",
                   "train.params.config.save_frequency=1", "train.params.config.save_best_after=0",
                   "+train.params.config.print_stats=False", "task.env.RECORD_TRAJECTORIES=True",
                   "task.env.RECORD_TRAJECTORIES_EVERY=8", "task.env.RECORD_TRAJECTORIES_STEPS=8",
                   "task.env.RECORD_TRAJECTORIES_DIR=" + str(tmp_path / "train")])
    torch.cuda.synchronize()
    run = tmp_path / "runs" / "masses"
    (npz,) = glob.glob(str(tmp_path / "train" / "*_episodes.npz"))
    inertia, names = episodes.load_env_inertia(npz)
    table, pnames = episodes.load_env_params(npz)
    assert inertia.shape == (abi.VI_COUNT, 512) and tuple(names) == abi.ENV_INERTIA_ROW_NAMES
    assert table.shape == (abi.VP_COUNT, 512) and tuple(pnames) == abi.ENV_PARAM_ROW_NAMES
    assert np.all(table == table[:, :1])                       # masses only: the parameter table is one row in every column
    cart = inertia[abi.VI_CART_MASS]
    assert np.float32(0.35) <= cart.min() < 0.37 and 0.68 < cart.max() <= np.float32(0.7) and len(np.unique(cart)) > 400
    mats = sorted(glob.glob(str(tmp_path / "train" / "*_trajectory_*_env*.mat")))
    assert mats, "RECORD_TRAJECTORIES wrote nothing"
    mat = scipy.io.loadmat(mats[0])
    e = int(mat["env"][0, 0])
    assert mat["env_inertia"].shape == (abi.VI_PRIMARY_COUNT, 1)
    assert np.array_equal(mat["env_inertia"][:, 0], inertia[:abi.VI_PRIMARY_COUNT, e].astype(np.float64))
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
    assert np.isfinite(reward) and steps > 0 and player.device_path is False          # a bound table: the stock path
    assert "reached_ever_rate by param_CART_MASS:" in out and "reached_ever_rate by param_LINK_MASS:" in out
    assert sorted(player.report["by_param"]) == ["param_CART_MASS", "param_LINK_MASS"]
    for name in ("param_CART_MASS", "param_LINK_MASS"):
        edges, rate, count = player.report["by_param"][name]
        assert len(edges) == len(rate) + 1 and int(count.sum()) == player.report["episodes"]
        ok = count > 0
        assert np.isfinite(rate[ok]).all() and ((0 <= rate[ok]) & (rate[ok] <= 1)).all()
    (play_npz,) = glob.glob(str(tmp_path / "play" / "*_episodes.npz"))
    assert np.array_equal(episodes.load_env_inertia(play_npz)[0], inertia)
