"""MPC_POLICY on the host side: the sampling planner of ``utils/mpc.py`` samples around the trained policy.

The semantics are stated once, in include/vine_mpc_policy.h.  Every sample rolls the policy closed-loop on its own model
state, the controller's ``nominal`` is a residual on the policy's mean, and the critic may close the horizon
(``terminal_value``).  What is left for the host: the configuration (``policy_config``), the numpy statements every GPU test
and the float64 oracle compare against (``head``, ``act``, ``keep``, ``terminal``, ``compose``), the network for N rows on the
trainer's own inference kernels (``PolicyProposal``) and the controller around the four launches (``PolicyController``);
``mpc.play(policy=...)`` and ``mpc.py policy=<checkpoint>`` run it."""
import numpy as np

from .. import abi
from ..learning.fast_inference import FastInferenceMixin
from .config import ConfigError
from .mpc import DEFAULTS as MPC_DEFAULTS
from .mpc import Controller, PlayVariant

DEFAULTS = {"ln_eps": 1e-5, "value_eps": 1e-5, "terminal_value": 0.0}
UNITS = abi.MPC_POLICY_UNITS


# ---------------------------------------------------------------------------------------------------------- configuration
def check_eps(key, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
        raise ConfigError("mpc policy: %s must be a finite number that is not negative, not %r" % (key, v))
    return float(v)


def policy_config(obs_width, ln_eps=DEFAULTS["ln_eps"], value_eps=DEFAULTS["value_eps"],
                  terminal_value=DEFAULTS["terminal_value"]):
    """The checked ``abi.VineMpcPolicyConfig``: what include/vine_mpc_policy.h refuses of it is refused here with a
    ``ConfigError`` naming the key (``obs_width``, ``ln_eps``, ``value_eps``, ``terminal_value``)."""
    c = abi.VineMpcPolicyConfig()
    c.abi_version = abi.MPC_POLICY_ABI_VERSION
    if isinstance(obs_width, bool) or not isinstance(obs_width, (int, np.integer)) or not 1 <= obs_width <= abi.MAX_OBS:
        raise ConfigError("mpc policy: obs_width must be an integer in 1 .. %d, not %r" % (abi.MAX_OBS, obs_width))
    c.obs_width = int(obs_width)
    c.ln_eps = check_eps("ln_eps", ln_eps)
    c.value_eps = check_eps("value_eps", value_eps)
    c.terminal_value = check_eps("terminal_value", terminal_value)
    return c


def check_shape(num_plants, samples):
    """N = M * K must be a multiple of 512, the shape of the inference kernels."""
    n = int(num_plants) * int(samples)
    if n % abi.MPC_POLICY_ROWS:
        raise ConfigError("mpc policy: plants * samples = %d * %d = %d must be a multiple of %d (the inference kernels' shape)"
                          % (int(num_plants), int(samples), n, abi.MPC_POLICY_ROWS))
    return n


# ---------------------------------------------------------------------------------------------------- the launches, in numpy
def head(y, hw, hc, ln_eps=DEFAULTS["ln_eps"]):
    """float64 [N, 3]: the LayerNorm folded into the rows mu_0, mu_1, value (``vine_rollout_head_prep``'s ``hw`` [3, 256] and
    ``hc`` [3]) applied to the LSTM output rows ``y`` [N, 256]: ``rstd * (hw[r] . (y - mean)) + hc[r]``."""
    y = np.asarray(y, dtype=np.float64).reshape(-1, UNITS)
    hw = np.asarray(hw, dtype=np.float64).reshape(3, UNITS)
    hc = np.asarray(hc, dtype=np.float64).reshape(3)
    centred = y - y.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt((centred * centred).mean(axis=1) + np.float64(ln_eps))
    return rstd[:, None] * (centred @ hw.T) + hc


def unnormalize_value(v, mean, var, eps=DEFAULTS["value_eps"]):
    """float32: ``clamp(v, +-5) * sqrt(float32(var) + eps) + float32(mean)``, the value normaliser inverted in float32."""
    v = np.asarray(v, dtype=np.float32)
    std = np.sqrt(np.float32(np.float64(var)) + np.float32(eps), dtype=np.float32)
    return (np.clip(v, np.float32(-5.0), np.float32(5.0)) * std + np.float32(np.float64(mean))).astype(np.float32)


def act(mu, d, clip):
    """float32 [N, 2]: ``clamp(mu + d, +-clip)`` -- one float32 add, the step's clamp."""
    x = np.asarray(mu, dtype=np.float32) + np.asarray(d, dtype=np.float32)
    clip = np.float32(clip)
    return np.minimum(np.maximum(x, -clip), clip)


def keep(mu, h, c, samples, plant_reset=None):
    """``(mu0 [M, 2], plant_h [M, 256], plant_c [M, 256])``: sample 0's rows of ``mu`` [N, 2], ``h`` and ``c`` [N, 256]; zeros
    for a plant whose reset is raised."""
    K = int(samples)
    mu0 = np.array(np.asarray(mu, dtype=np.float32)[::K])
    ph = np.array(np.asarray(h, dtype=np.float32).reshape(-1, UNITS)[::K])
    pc = np.array(np.asarray(c, dtype=np.float32).reshape(-1, UNITS)[::K])
    if plant_reset is not None:
        consumed = np.asarray(plant_reset).reshape(-1) != 0
        mu0[consumed], ph[consumed], pc[consumed] = 0.0, 0.0, 0.0
    return mu0, ph, pc


def terminal(cost, alive, value, terminal_value):
    """``(cost float64 [N], alive uint8 [N])`` behind the terminal launch: an alive sample's cost minus
    ``terminal_value * float64(V)`` (one multiply, one subtract); a non-finite V gives +inf and clears ``alive``; a sample
    that is not alive is not touched."""
    cost = np.array(cost, dtype=np.float64)
    alive = np.array(alive).astype(bool)
    v = np.asarray(value, dtype=np.float32)
    bad = alive & ~np.isfinite(v)
    good = alive & np.isfinite(v)
    with np.errstate(invalid="ignore"):
        wv = np.float64(terminal_value) * v.astype(np.float64)
        cost[good] = cost[good] - wv[good]
    cost[bad] = np.inf
    return cost, (alive & ~bad).astype(np.uint8)


def compose(mu0, plant_actions, history, clip, plant_reset=None):
    """``(plant_actions [M, 2], history [M, MAX_DELAY, 2])`` behind the composition: ``clamp(mu0 + residual, +-clip)`` to the
    plant's action and to the history's front; a plant whose reset is raised keeps both."""
    residual = np.array(plant_actions, dtype=np.float32)
    history = np.array(history, dtype=np.float32).reshape(residual.shape[0], abi.MAX_DELAY, 2)
    a = act(mu0, residual, clip)
    if plant_reset is not None:
        consumed = np.asarray(plant_reset).reshape(-1) != 0
        a[consumed] = residual[consumed]
        front = history[:, 0].copy()
        front[~consumed] = a[~consumed]
        history[:, 0] = front
    else:
        history[:, 0] = a
    return a, history


# ------------------------------------------------------------------------------------------------------------ the network
class PolicyProposal(FastInferenceMixin):
    """The policy network for N rows on the trainer's inference kernels (``FastInferenceMixin._infer``: the split-fp32 MLP
    and LSTM step), with the head's operands ``hw`` / ``hc`` of ``vine_rollout_head_prep``.

    ``params``: the ``train.params`` block of the composed configuration, as ``train.py test=True`` hands it to the player.
    Only the default network is served (256-128-64 ELU MLP, LSTM 256 with LayerNorm, concatenated input, normalised input) at
    N a multiple of 512 in the split-fp32 mode: anything else is refused by name, never run on another path."""

    def __init__(self, params, num_rows, obs_width, device="cuda:0"):
        import torch
        from ..learning import fused
        from ..learning.network import ModelA2CContinuousLogStd
        config = params["config"]
        self.device = torch.device(device)
        self.obs_shape = (int(obs_width),)
        self.normalize_input = bool(config.get("normalize_input", False))
        self.normalize_value = bool(config.get("normalize_value", False))
        self.model = ModelA2CContinuousLogStd(params["network"], abi.NUM_ACTIONS, self.obs_shape, self.normalize_value,
                                              self.normalize_input).to(self.device)
        self.model.eval()
        self.num_actors = int(num_rows)
        self.fused_rollout, self.rollout_lp16, self._pending_fin = True, False, None
        self.rollout_f32_terms = int(config.get("rollout_f32_terms", fused.ROLLOUT_F32_SPLIT))
        if self.num_actors % abi.MPC_POLICY_ROWS:
            raise ConfigError("mpc policy: %d rows must be a multiple of %d (the inference kernels' shape)"
                              % (self.num_actors, abi.MPC_POLICY_ROWS))
        self.rnn_states = [s.contiguous() for s in self.model.get_default_rnn_state(self.num_actors, self.device)]
        self._setup_fast_inference()
        f = self._fast
        if f is None:
            raise ConfigError("mpc policy: the network is not served by the inference kernels (they need normalize_input, ELU "
                              "activations, an LSTM of 256, 512 or 1024 units with LayerNorm and MLP widths that are multiples of 4)")
        for key, why in (("f32_mfma", "the fp32 matrix-core kernels serve the 256-128-64 MLP with concatenated input, an LSTM of 256 "
                                      "units and at most 32 observation columns"),
                         ("mlp_wt_split", "the split MLP needs rollout_f32_terms of 6 or 9"),
                         ("ln_in_head", "the head applies the LayerNorm of a 256-unit LSTM itself")):
            if f.get(key) is None or f.get(key) is False:
                raise ConfigError("mpc policy: %s does not hold for this network or shape (%s)" % (key, why))
        self.hw = torch.empty(3 * UNITS, device=self.device)
        self.hc = torch.empty(3, device=self.device)
        self.prepare()

    def restore(self, fn):
        """The weights and normalisers of a checkpoint of ``train.py``; the operand copies follow."""
        import torch
        ckpt = torch.load(fn, map_location=self.device, weights_only=False)
        self.model.load_state_dict(ckpt["model"])
        self.prepare()

    def prepare(self):
        """The operand copies of the weights and the head's products, once per set of weights; outside any capture."""
        import torch
        with torch.no_grad():
            self._infer_begin()
            self._head_prep(self.hw, self.hc)

    @property
    def ln_eps(self):
        return float(self.model.a2c_network.layer_norm.eps)

    def value_statistics(self):
        """``(mean, var, eps)``: the value normaliser's float64 statistics, or ``(None, None, default)`` without one."""
        if not self.normalize_value:
            return None, None, DEFAULTS["value_eps"]
        rms = self.model.value_mean_std
        return rms.running_mean, rms.running_var, float(rms.epsilon)

    def h_op(self):
        """Address and row stride (in floats) of the operand copy of h that the next ``_infer`` READS."""
        f = self._fast
        xh = f["xh2"][f["cur"]]
        return xh.data_ptr() + xh.element_size() * f["XW"], f["XW"] + f["H"]

    def tensors(self):
        """What a control step writes of the network's buffers."""
        return [self.rnn_states[0], self.rnn_states[1], self._fast["xh2"][0], self._fast["xh2"][1]]


# ------------------------------------------------------------------------------------------------------------ the device
class PolicyController(Controller):
    """A ``Controller`` whose samples roll the policy: the extra state of include/vine_mpc_policy.h and the four launches.

    ``control_step()`` = ``fork()``, ``policy_fork()``, H x (``_infer`` + ``policy_act()`` + ``model.step_into`` + ``node()``),
    [``terminal_value`` != 0: ``_infer(commit=False)`` + ``policy_terminal()``], ``update()``, ``policy_compose()``,
    ``plant.step_into``.  ``keep_mu``: every act also stores mu of every sample in ``mu`` [N, 2], and the terminal launch V in
    ``value`` [N] -- diagnostics, nothing reads them back."""

    def __init__(self, plant_task, model_task, samples, proposal, horizon=MPC_DEFAULTS["horizon"], lam=MPC_DEFAULTS["lambda"],
                 sigma=MPC_DEFAULTS["sigma"], seed=MPC_DEFAULTS["seed"], graph=True, graph_steps=1, keep_weights=False,
                 terminal_value=DEFAULTS["terminal_value"], keep_mu=False):
        import torch
        super().__init__(plant_task, model_task, samples, horizon, lam, sigma, seed, graph=graph, graph_steps=graph_steps,
                         keep_weights=keep_weights)
        N = check_shape(self.M, self.K)
        if int(plant_task.num_obs) != int(model_task.num_obs):
            raise ConfigError("mpc policy: the plant has %d observation columns, the model %d" % (
                int(plant_task.num_obs), int(model_task.num_obs)))
        if int(proposal.num_actors) != N or int(proposal.obs_shape[0]) != int(plant_task.num_obs):
            raise ConfigError("mpc policy: the network was set up for %d rows of %d columns, not %d of %d" % (
                int(proposal.num_actors), int(proposal.obs_shape[0]), N, int(plant_task.num_obs)))
        if torch.device(proposal.device) != torch.device(self.device):
            raise ConfigError("mpc policy: the network sits on %s, the plant on %s" % (proposal.device, self.device))
        self.proposal = proposal
        vmean, vvar, veps = proposal.value_statistics()
        self.value_mean, self.value_var = vmean, vvar
        self.pcfg = policy_config(int(plant_task.num_obs), proposal.ln_eps, veps, terminal_value)
        self.terminal_value = float(terminal_value)
        dev, f32 = self.device, torch.float32
        self.plant_h = torch.zeros((self.M, UNITS), dtype=f32, device=dev)
        self.plant_c = torch.zeros((self.M, UNITS), dtype=f32, device=dev)
        self.mu0 = torch.zeros((self.M, 2), dtype=f32, device=dev)
        self.mu = torch.zeros((N, 2), dtype=f32, device=dev) if keep_mu else None
        self.value = torch.zeros(N, dtype=f32, device=dev) if keep_mu else None
        self.plant_obs.copy_(plant_task.reset()["obs"])      # what the policy sees first: the plant's reset observation
        self.launches.update({"policy_fork": 0, "infer": 0, "policy_act": 0, "policy_terminal": 0, "policy_compose": 0})

    def tensors(self):
        extra = [self.plant_h, self.plant_c, self.mu0] + [t for t in (self.mu, self.value) if t is not None]
        return super().tensors() + extra + self.proposal.tensors()

    # -- the four launches, and the trunk ----------------------------------------------------------------------------------
    def policy_fork(self):
        from .. import native
        p, m, q = self.plant, self.model, self.proposal
        q._fast["cur"] = 0             # every control step issues the same addresses, whatever the parity of H
        h_op, stride = q.h_op()
        native.check(self.lib.vine_mpc_policy_fork(
            p._handle, m._handle, self.mcfg, self.pcfg, self.plant_obs.data_ptr(), int(self.plant_obs.shape[1]),
            self.model_obs.data_ptr(), int(self.model_obs.shape[1]), self.plant_h.data_ptr(), self.plant_c.data_ptr(),
            q.rnn_states[0].data_ptr(), q.rnn_states[1].data_ptr(), h_op, stride, self._stream()), self.lib)
        self.launches["policy_fork"] += 1

    def infer(self, commit=True):
        """The policy's trunk on the model's observation buffer; returns the LSTM output rows the head reads."""
        y = self.proposal._infer(self.model_obs, commit=commit)
        self.launches["infer"] += 1
        return y

    def policy_act(self, y):
        from .. import native
        q = self.proposal
        native.check(self.lib.vine_mpc_policy_act(
            self.model._handle, self.mcfg, self.pcfg, y.data_ptr(), q.hw.data_ptr(), q.hc.data_ptr(), self.window.data_ptr(),
            self.plant.reset_buf.data_ptr(), q.rnn_states[0].data_ptr(), q.rnn_states[1].data_ptr(), self.actions.data_ptr(),
            self.mu0.data_ptr(), self.plant_h.data_ptr(), self.plant_c.data_ptr(),
            self.mu.data_ptr() if self.mu is not None else None, self._stream()), self.lib)
        self.launches["policy_act"] += 1

    def policy_terminal(self, y):
        from .. import native
        q = self.proposal
        native.check(self.lib.vine_mpc_policy_terminal(
            self.model._handle, self.mcfg, self.pcfg, y.data_ptr(), q.hw.data_ptr(), q.hc.data_ptr(),
            self.value_mean.data_ptr() if self.value_mean is not None else None,
            self.value_var.data_ptr() if self.value_var is not None else None, self.window.data_ptr(), self.cost.data_ptr(),
            self.alive.data_ptr(), self.value.data_ptr() if self.value is not None else None, self._stream()), self.lib)
        self.launches["policy_terminal"] += 1

    def policy_compose(self):
        from .. import native
        native.check(self.lib.vine_mpc_policy_compose(
            self.model._handle, self.mcfg, self.pcfg, self.mu0.data_ptr(), self.plant.reset_buf.data_ptr(),
            self.plant_actions.data_ptr(), self.history.data_ptr(), self._stream()), self.lib)
        self.launches["policy_compose"] += 1

    def model_step(self):
        """The policy on the sample's observation, its mean added to the perturbation the fork or the node left, one model
        step, and the node behind it."""
        self.policy_act(self.infer())
        super().model_step()

    def after_fork(self):
        self.policy_fork()

    def before_update(self):
        if self.terminal_value != 0.0:
            self.policy_terminal(self.infer(commit=False))

    def after_update(self):
        self.policy_compose()

    def control_step(self):
        import torch
        with torch.no_grad():
            super().control_step()

    def clear_rows(self, ids):
        """The policy's LSTM state of those plants starts anew too."""
        super().clear_rows(ids)
        self.plant_h[ids] = 0.0
        self.plant_c[ids] = 0.0


# ------------------------------------------------------------------------------------------------------------------ a run
class Play(PlayVariant):
    """``policy=`` of ``mpc.play``, with its ``policy_params`` and ``terminal_value``."""

    def check(self, run):
        if run.args["policy_params"] is None:
            raise ConfigError("mpc: policy= needs policy_params, the train.params block the network is built from")
        check_shape(run.M, run.samples)
        check_eps("terminal_value", run.args["terminal_value"])

    def controller(self, run):
        proposal = PolicyProposal(run.args["policy_params"], run.M * int(run.samples), int(run.plant.num_obs), run.plant.device)
        proposal.restore(self.spec)
        return PolicyController(run.plant, run.model, run.samples, proposal, *run.planner, graph=run.graph,
                                terminal_value=run.args["terminal_value"])

    def banner(self, run):
        print("mpc: the samples roll the policy of %s; terminal_value %g" % (self.spec, float(run.args["terminal_value"])), flush=True)

    def result(self, run, out):
        out["policy"] = self.spec
