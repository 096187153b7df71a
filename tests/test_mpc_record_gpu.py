"""Whole MPC control steps on the GPU held to a float64 replay of every launch (tests/mpc_reference.py).

A run is S control steps issued eagerly, piece by piece, in ``Controller.control_step``'s own order -- fork, ``after_fork``,
H x (model step, node), update, plant step -- with a host copy of every written tensor behind each launch.  The replay checks,
per control step: (1) the fork (every field outside the ring and ``progress`` the plant's in every bit, the bookkeeping, the
live ring slots in age order against ``fork_reference``'s float64 ring, the sentinel above the delay); (2) every model step,
teacher-forced, flags exact and every group of ``step_reference.GROUP_NAMES`` within ``K_STEP`` / ``K_JOINT`` x max(float32
oracle's error, 2^-24) per class; (3) the node's actions and cost sums bit for bit and the update against ``mpc_replay`` /
``ensemble_replay`` on the run's own data; (4) the plant step, teacher-forced against the plant's own oracles; (5) the decision:
the device's ``plant_actions`` against a float64 planner that rolls the window free-running from the forked state, within
``K_PLAN`` x max(float32 planner's error, 2^-24 x clipActions) per plant in the max and the rms norm.

Cases (M plants, K samples, H steps, S control steps), the smallest shapes that keep a partial wave, several plants per wave, K
no power of two and every delay 0..8 in one wave; the model's env e carries set e % 9 of tests/env_params_sets.py /
tests/env_inertia_sets.py, the plants sets of their own:
    params9            3, 18, 5, 6   free space; the parameter table on the model; plants with sets 2, 5, 7; 7-step episodes
    inertia9           3, 18, 5, 6   configuration rows beside the inertia table; mass sets 1, 4, 8 on the plants; ``stiffness``
    randomized_plant   5, 14, 4, 4   no table on the model (the dispatched route and each route forced); plant randomised
    pipe               2, 27, 3, 4   pipe placed around the tips; parameter table
    ensemble9          2, 18, 4, 4   ``EnsembleRig``'s launches, E = 9, RISK entropic, THETA 0.7; both tables on the model
    controller_masses  2, 18, 3, 3   ``mpc.Controller`` with ``set_model_params`` of LINK_MASS and CART_MASS, and
                                     ``EnsembleController.set_members`` of LINK_MASS; checks 1, 2, 3 and 5
In every case a sample dies inside a window by time-out and one by the rail limit, and a plant's reset is consumed by an update.
The negative controls of ``params9`` (history shifted by one entry, sets rotated by one, ``progress`` not copied, ``cost_sums``
dropping the resetting step, the node's action taken at k + 1) and of ``inertia9`` (the mass sets ignored) must break their
bounds by ``CONTROL_MARGIN``.

Measured on an MI355X: the decision's error / max(float32 planner's error, 2^-24 x clipActions), the worst plant and norm:
    params9                      0.724 (plant 2, max)
    inertia9                     1.034 (plant 2, max)
    randomized_plant             0.376 (plant 3, max)     the dispatched route: vine_step_quad_kernel
    randomized_plant-lane        0.250 (plant 0, max)
    randomized_plant-quad        0.376 (plant 3, max)
    pipe                         1.441 (plant 0, rms)
    ensemble9                    0.203 (plant 1, max)
    controller_masses            0.293 (plant 1, max)
    controller_masses-ensemble   0.559 (plant 1, max)
hence ``K_PLAN`` (tests/mpc_reference.py) = 2.2 (1.5 x 1.441).  Where the float32 planner's error is 0 the weights have
collapsed onto one sample and the decision is that sample's action: the device is then held to the floor alone.  No env-step of any
case was undecided and no plant-window left out.  The teacher-forced steps' worst error / max(float32 oracle's error, 2^-24): 3.02
(``qd``, randomized_plant) on the model, 3.73 (``q``, randomized_plant) on the plants, against ``K_JOINT`` = 8.7; 3.61 (``rew``,
pipe, plants) against ``K_STEP`` = 5.1.  The controls on the device, as error against the wrong reference / bound: 1.8e5 and more
(a wrong input flips a sample's rail or time-out flag, and with it a reward term or a weight); the exact comparisons found 6 of 6
cost tensors and 24 of 24 action tensors differing.  Each run prints its figures;
profiles/mpc_record/ratios.txt has every group of every case, the controls, the caps' counts and this table.
"""
import numpy as np
import pytest
import torch

from tests import env_inertia_sets, env_params_sets
from tests import mpc_reference as mr
from tests.test_mpc_ensemble_gpu import EnsembleRig, _ensemble_pair
from tests.test_mpc_gpu import _plant_cfg
from vine_robot_isaacgymenvs_amd import abi, native
from vine_robot_isaacgymenvs_amd.utils import env_params, mpc, mpc_ensemble

pytestmark = pytest.mark.gpu

F = abi
CONTROLS_OF = {"params9": ("history_shift", "rotated_sets", "progress_zero", "cost_drop", "action_next"),
               "inertia9": ("ignore_inertia",)}
KERNELS = ("vine_step_kernel", "vine_step_quad_kernel")


def _handle(cfg, kind, sets, kernel=None):
    """A handle whose env e carries set ``sets[e]`` of ``kind`` (``params``, ``inertia``: the configuration's parameter rows
    beside the mass sets, ``both``, or None: no table), the route asserted."""
    from tests.hip_env import HipEnv
    dev = type("HipEnv_" + str(kernel), (HipEnv,), {"kernel": kernel})(cfg)
    lib, n = dev.lib, dev.n

    def upload(table, rows, check):
        check(lib, dev.cfg, table)
        t = torch.as_tensor(np.ascontiguousarray(table, np.float32)).to(dev.dev).contiguous()
        assert t.shape == (rows, n)
        torch.cuda.synchronize(dev.dev)
        return t

    if kind is not None:
        params = (env_params_sets.set_rows(lib, dev.cfg)[np.asarray(sets)].T if kind in ("params", "both") else
                  np.repeat(env_params.config_row(lib, dev.cfg)[:, None], n, axis=1))
        dev.params_t = upload(params, abi.VP_COUNT, env_params.check_table)
        assert lib.vine_bind_env_params(dev.h, dev.params_t.data_ptr()) == abi.OK
    if kind in ("inertia", "both"):
        dev.inertia_t = upload(env_inertia_sets.set_rows(lib, dev.cfg)[np.asarray(sets)].T, abi.VI_COUNT, env_params.check_inertia_table)
        assert lib.vine_bind_env_inertia(dev.h, dev.inertia_t.data_ptr()) == abi.OK
    assert lib.vine_env_params_bound(dev.h) == int(kind is not None)
    assert lib.vine_env_inertia_bound(dev.h) == int(kind in ("inertia", "both"))
    name = lib.vine_step_kernel_name(dev.h).decode()
    assert name in KERNELS and (kind is None or name == "vine_step_kernel"), (kind, name)
    return dev


class DeviceController(EnsembleRig):
    """The library's handles and launches behind ``mpc_reference.HostController``'s interface: ``Rig``'s and ``EnsembleRig``'s
    launch methods of tests/test_mpc_gpu.py and tests/test_mpc_ensemble_gpu.py over handles with this case's tables."""

    def __init__(self, case, kernel=None):
        if not torch.cuda.is_available():
            pytest.fail("GPU tests need an MI355X (the product has no CPU fallback)")
        self.case = case
        M, K, H = case.M, case.K, case.H
        self.M, self.K, self.H, self.N, self.E = M, K, H, M * K, case.members
        self.G = K // self.E
        self.lib = native.load()
        self.pcfg = mr.plant_cfg(case)
        self.plant = _handle(self.pcfg, case.model if case.plant_sets else None, case.plant_sets)
        self.model = _handle(mr.model_cfg(case), case.model, np.arange(self.N) % mr.NUM_SETS, kernel)
        self.kernel_name = self.lib.vine_step_kernel_name(self.model.h).decode()
        d = self.dev = self.plant.dev
        self.sigma, self.lam, self.seed = list(mr.SIGMA), mr.LAMBDA, mr.PLANNER_SEED
        self.clip = float(self.model.cfg.clip_actions)
        self.mcfg = mpc.mpc_config(M, K, H, self.lam, self.sigma, self.seed)
        if self.E > 1:
            self.spec = {"params": {"DAMPING": 0.02}, "MEMBERS": self.E, "RISK": case.risk, "THETA": case.theta}
            self.ecfg = mpc_ensemble.ensemble_struct(self.spec, self.mcfg)
        S = mr.SENTINEL
        self.nominal = torch.zeros((M, H, 2), device=d)
        self.history = torch.zeros((M, F.MAX_DELAY, 2), device=d)
        self.tick = torch.zeros(M, dtype=torch.long, device=d)
        self.cost = torch.full((self.N,), S, dtype=torch.float64, device=d)
        self.alive = torch.full((self.N,), 9, dtype=torch.uint8, device=d)
        self.window = torch.full((1,), -99, dtype=torch.long, device=d)
        self.actions = torch.full((self.N, 2), S, device=d)
        self.plant_actions = torch.full((M, 2), S, device=d)
        self.weights = torch.full((self.N,), S, dtype=torch.float64, device=d)
        self.group_cost = torch.full((M * self.G,), S, dtype=torch.float64, device=d)

    def load(self, nominal, history, tick):
        self.nominal.copy_(torch.as_tensor(nominal))
        self.history.copy_(torch.as_tensor(history))
        self.tick.copy_(torch.as_tensor(tick))

    def buffers(self):
        torch.cuda.synchronize(self.dev)
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("nominal", "history", "tick", "cost", "alive", "window",
                                                                    "actions", "plant_actions", "weights", "group_cost")}

    def fork(self):
        assert EnsembleRig.fork(self) == abi.OK, self.lib.vine_last_error()

    def after_fork(self):
        if self.E > 1:
            self.ensemble_node()

    def step_model(self):
        self.model.step_t(self.actions, sync=False)

    def node(self):
        EnsembleRig.node(self)
        if self.E > 1:
            self.ensemble_node()

    def update(self):
        if self.E > 1:
            self.ensemble_update()
        else:
            EnsembleRig.update(self)
            self.group_cost.copy_(self.cost)

    def step_plant(self):
        self.plant.step_t(self.plant_actions, sync=False)


def _show_and_check(case, res, clip, controls=(), title=None):
    print("\n" + "\n".join(mr.lines(case, res, clip)).replace("] %s" % case.name, "] %s" % (title or case.name)), flush=True)
    margins = mr.control_margins(case, res, clip, controls)
    if controls:
        print("[mpc record] %s controls (error against the wrong reference / bound): %s" % (
            case.name, ", ".join("%s %.3g (%s)" % (n, m[1], m[0]) for n, m in margins.items())), flush=True)
    mr.check_caps(case, res)
    mr.check_bounds(case, res, clip)
    weak = {n: m for n, m in margins.items() if not m[1] >= mr.CONTROL_MARGIN}
    assert not weak, ("negative control within the bound", case.name, weak)
    assert len(margins) >= len(controls)


# without a table the library dispatches by size: the route it takes for 70 envs, and each route forced
CASE_KERNELS = [(c, k) for c in mr.CASES for k in ((None, "lane", "quad") if c.name == "randomized_plant" else (None,))]


@pytest.mark.parametrize("case,kernel", CASE_KERNELS, ids=["%s%s" % (c.name, "-" + k if k else "") for c, k in CASE_KERNELS])
def test_control_steps_against_the_float64_replay(case, kernel):
    """Checks 1 - 5 of a case; the negative controls on ``params9`` and ``inertia9``."""
    controls = CONTROLS_OF.get(case.name, ())
    seen = {}

    def make(c):
        seen["ctl"] = DeviceController(c, kernel)
        return seen["ctl"]

    res, clip = mr.run_case(case, make, controls)
    name = seen["ctl"].kernel_name
    print("\n[mpc record] %s: model step kernel %s" % (case.name, name))
    if kernel:                                       # default physics, no table: ``use_quad_kernel`` covers it
        assert name == {"lane": "vine_step_kernel", "quad": "vine_step_quad_kernel"}[kernel]
    _show_and_check(case, res, clip, controls, title=case.name + ("-" + kernel if kernel else ""))


# ------------------------------------------------------------------------------------------------------ the task classes
MASSES = mr.Case("controller_masses", 2, 18, 3, 3, "default", False, None, "masses", None, 1, None, None, 4, 56)
MASSES_ENSEMBLE = MASSES._replace(name="controller_masses-ensemble", members=3, risk="mean")
PLANT_OVER = dict(maxEpisodeLength=MASSES.episode, ACTION_DELAY=2)


def _with_masses(vcfg, n, link=None, cart=None):
    """A copy of a task's configuration with ``n`` envs, LINK_MASS (a factor on the link masses and inertias, formed in float64
    and rounded once: utils/env_params.py ``set_inertia_rows``) and CART_MASS (kg) applied."""
    c = type(vcfg).from_buffer_copy(vcfg)
    c.num_envs = n
    if link is not None:
        for i in range(abi.NUM_LINKS):
            c.link_mass[i] = float(np.float32(np.float64(vcfg.link_mass[i]) * link))
            c.link_inertia[i] = float(np.float32(np.float64(vcfg.link_inertia[i]) * link))
    if cart is not None:
        c.cart_mass = float(np.float32(cart))
    return c


class TaskController:
    """``mpc.Controller`` / ``EnsembleController`` over task classes behind ``mpc_reference.HostController``'s interface."""

    def __init__(self, case, plant, model, ctl, model_cfgs, which):
        self.case, self.plant, self.model, self.ctl = case, plant, model, ctl
        self.M, self.K, self.H, self.N, self.E = ctl.M, ctl.K, ctl.H, ctl.M * ctl.K, case.members
        self.sigma, self.lam, self.seed = list(mr.SIGMA), mr.LAMBDA, mr.PLANNER_SEED
        self.clip = float(model._vcfg.clip_actions)
        self.pcfg = plant._vcfg
        self._sets = mr.types.SimpleNamespace(model=(model_cfgs, which), plant=([plant._vcfg], np.zeros(self.M, np.int64)))

    def sets(self):
        return self._sets

    def buffers(self):
        c = self.ctl
        torch.cuda.synchronize(c.device)
        out = {k: getattr(c, k).cpu().numpy().copy() for k in ("nominal", "history", "tick", "cost", "alive", "window", "actions",
                                                               "plant_actions", "weights")}
        out["group_cost"] = (c.group_cost if self.E > 1 else c.cost).cpu().numpy().copy()
        return out

    def fork(self):
        self.ctl.fork()

    def after_fork(self):
        self.ctl.after_fork()

    def step_model(self):
        self.ctl.model.step_into(self.ctl.actions, self.ctl.model_obs)

    def node(self):
        mpc.Controller.node(self.ctl)
        if self.E > 1:
            self.ctl.ensemble_node()

    def update(self):
        self.ctl.update()

    def step_plant(self):
        self.ctl.plant.step_into(self.ctl.plant_actions, self.ctl.plant_obs)


def _seed_tasks(tc):
    """Two plant steps on action zero (the first consumes the initial reset), plant 0's cart moved to the rail limit on its way
    out and plant 1 one step younger, so that the plants' samples do not all time out at the same step; the model's ring full of
    the sentinel; the reward matrices bound (which arms introspection: the oracles read the tip in
    front of a step from the state block)."""
    plant, model, ctl = tc.plant, tc.model, tc.ctl
    plant.bind_reward_matrix()
    model.bind_reward_matrix()
    zero = torch.zeros_like(ctl.plant_actions)
    for _ in range(2):
        plant.step_into(zero, ctl.plant_obs)
    torch.cuda.synchronize(ctl.device)
    shift = (float(plant._vcfg.rail_soft_limit) - 0.012) - float(plant.state[F.VF_Q0, 0])
    for f in (F.VF_Q0, F.VF_CART_Y, F.VF_TIP_Y, F.VF_PREV_TIP_Y, F.VF_TARGET_Y, F.VF_PREV_Q0):
        plant.state[f, 0] += shift
    for f in (F.VF_QD0, F.VF_CART_VY, F.VF_PREV_CART_VEL):
        plant.state[f, 0] = 0.25
    plant.progress_buf[1] = 0
    model.state[mr.RING0:mr.RING1] = mr.SENTINEL
    model.step_count = mr.MODEL_COUNT
    rng = np.random.default_rng(MASSES.seed)
    ctl.nominal.copy_(torch.as_tensor(rng.uniform(-0.5, 0.5, (tc.M, tc.H, 2)).astype(np.float32)))
    ctl.history.copy_(torch.as_tensor(rng.uniform(-1.3, 1.3, (tc.M, F.MAX_DELAY, 2)).astype(np.float32)))
    ctl.tick.copy_(torch.as_tensor([(1 << 33) + 9, 4][:tc.M]))
    torch.cuda.synchronize(ctl.device)


def _task_run(tc, case):
    _seed_tasks(tc)
    res = mr.replay(tc, case, mr.record(tc, case.S), plant_step=False)
    _show_and_check(case, res, tc.clip)


def _inertia_words(task):
    return task.env_inertia.cpu().numpy()


def test_controller_with_model_masses_against_the_float64_replay():
    """``mpc.Controller(graph=False)`` over ``mpc.make_task`` tasks whose model binds LINK_MASS and CART_MASS, set per plant by
    ``set_model_params``: the model's inertia table, read back from the device, is ``derive_inertia`` of the repeated values bit
    for bit, and the oracles are built from the tasks' ``_vcfg`` with those masses applied.  Checks 1, 2, 3 and 5."""
    case = MASSES
    M, K, H = case.M, case.K, case.H
    link, cart = np.array([0.8, 1.3]), np.array([0.5, 0.36])
    cfg = _plant_cfg(M, **PLANT_OVER)
    mcfg = mpc.model_config(cfg, M, K)
    mcfg["env"]["ENV_PARAMS"] = {"LINK_MASS": [0.7, 1.4], "CART_MASS": [0.3, 0.6]}       # binds the tables; set per plant below
    plant, model = mpc.make_task(cfg), mpc.make_task(mcfg)
    try:
        ctl = mpc.Controller(plant, model, K, H, sigma=list(mr.SIGMA), lam=mr.LAMBDA, seed=mr.PLANNER_SEED, graph=False,
                             keep_weights=True)
        ctl.set_model_params({"LINK_MASS": link, "CART_MASS": cart})
        lib, v = model._lib, model._vcfg
        table = np.repeat(env_params.inertia_config_row(lib, v)[:, None], M * K, axis=1)
        env_params.set_inertia_rows(table, env_params.inertia_config_row(lib, v),
                                    {"LINK_MASS": np.repeat(link, K), "CART_MASS": np.repeat(cart, K)})
        assert mr.same(_inertia_words(model), env_params.derive_inertia(lib, v, table))
        assert lib.vine_env_inertia_bound(model._handle) == 1 and model.step_kernel_name == "vine_step_kernel"
        cfgs = [_with_masses(v, M * K, link[p], cart[p]) for p in range(M)]
        _task_run(TaskController(case, plant, model, ctl, cfgs, np.arange(M * K) // K), case)
    finally:
        model.close()
        plant.close()


def test_ensemble_controller_with_mass_members_against_the_float64_replay():
    """``EnsembleController.set_members`` with LINK_MASS members: sample j of plant p is member j mod E."""
    case = MASSES_ENSEMBLE
    M, K, H, E = case.M, case.K, case.H, case.members
    members = np.array([[0.75, 1.0, 1.35], [1.2, 0.9, 0.7]])
    spec = {"params": {"LINK_MASS": [0.7, 1.4]}, "MEMBERS": E, "RISK": case.risk}
    plant, model, ctl = _ensemble_pair(M, K, H, spec, members={"LINK_MASS": members}, plant_over=PLANT_OVER, sigma=list(mr.SIGMA),
                                       lam=mr.LAMBDA, seed=mr.PLANNER_SEED, graph=False, keep_weights=True)
    try:
        lib, v = model._lib, model._vcfg
        tiled = mpc_ensemble.tile_members({"LINK_MASS": members}, K // E)["LINK_MASS"]
        table = np.repeat(env_params.inertia_config_row(lib, v)[:, None], M * K, axis=1)
        env_params.set_inertia_rows(table, env_params.inertia_config_row(lib, v), {"LINK_MASS": tiled})
        assert mr.same(_inertia_words(model), env_params.derive_inertia(lib, v, table))
        assert lib.vine_env_inertia_bound(model._handle) == 1
        cfgs = [_with_masses(v, M * K, members[p, m]) for p in range(M) for m in range(E)]
        which = (np.arange(M * K) // K) * E + (np.arange(M * K) % K) % E
        _task_run(TaskController(case, plant, model, ctl, cfgs, which), case)
    finally:
        model.close()
        plant.close()
