"""Reference of the rollout record: what ``A2CAgent.play_steps_rnn`` leaves behind, restated step by step.

Nothing here comes from ``learning/fused.py``, ``learning/fast_inference.py`` or the HIP library.  The network is written
out from the model's parameters in plain torch as tests/update_reference.py writes the training forward (normalise with the
float64 statistics, clamp at +-5, MLP + ELU, concatenated observation, one LSTM cell, LayerNorm, the two heads, the value
un-normalised as ``RunningMeanStd(unnorm=True)`` does: clamp at +-5, times sqrt(var + eps), plus mean) and runs in float64,
or in float32 as the yardstick of what fp32 arithmetic costs.  The env side is the CPU oracle re-seeded from the device's
own state before every step; the bookkeeping, GAE and the value normaliser's updates are float64 numpy / torch loops.

``replay`` is teacher-forced: the LSTM state starts from the record's stored state wherever the record has one (the
``mb_rnn_states`` slots every ``seq_len`` steps, ``rnn_states`` behind the last step) and is the reference's own in between,
zeroed wherever the done flag of the previous step is set.  Its ``control`` argument recomputes the reference from subtly
wrong inputs (the negative controls of tests/test_rollout_record.py)."""
import copy
import math

import numpy as np
import torch
import torch.nn.functional as F

from vine_robot_isaacgymenvs_amd import abi

CONTROLS = ("state not zeroed", "dones shifted", "h two steps back", "snapshot one step late", "last values one step on",
            "normaliser at 0 / 1")
NEAR = 1e-5          # a reset criterion this close to its threshold (float64 oracle) may go either way in float32


def model_copy(model, dtype, device):
    """A deep copy of ``model`` in eval mode with its parameters in ``dtype`` (the normalisers' statistics stay float64, as
    in the product)."""
    net = model.a2c_network
    lookup, net.op_weight_lookup = net.op_weight_lookup, None         # (a bound method of the optimiser: not copied)
    try:
        m = copy.deepcopy(model)
    finally:
        net.op_weight_lookup = lookup
    m = m.to(device).eval()
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
        p.data = p.data.to(dtype)
    return m


def policy_step(m, obs, h, c, unit_normaliser=False):
    """One inference step of ``ModelA2CContinuousLogStd`` in the dtype of ``h``
    -> mu [N, A], un-normalised value [N, 1], h' [N, H], c' [N, H]."""
    net, dt = m.a2c_network, h.dtype
    x0 = obs.to(dt)
    if m.normalize_input:
        rms = m.running_mean_std
        mean, var = rms.running_mean.to(dt), rms.running_var.to(dt)
        if unit_normaliser:
            mean, var = torch.zeros_like(mean), torch.ones_like(var)
        x0 = ((x0 - mean) / torch.sqrt(var + rms.epsilon)).clamp(-5.0, 5.0)
    x = x0
    for mod in net.actor_mlp:
        x = F.linear(x, mod.weight, mod.bias) if isinstance(mod, torch.nn.Linear) else F.elu(x)
    if net.rnn_concat_input:
        x = torch.cat([x, x0], dim=1)
    r = net.rnn.rnn
    h, c = torch._VF.lstm_cell(x, (h, c), r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0)
    y = h
    if net.rnn_ln:
        y = F.layer_norm(y, (y.shape[1],), net.layer_norm.weight, net.layer_norm.bias, net.layer_norm.eps)
    mu = F.linear(y, net.mu.weight, net.mu.bias)
    value = F.linear(y, net.value.weight, net.value.bias)
    if m.normalize_value:
        vms = m.value_mean_std
        value = value.clamp(-5.0, 5.0) * torch.sqrt(vms.running_var.to(dt) + vms.epsilon) + vms.running_mean.to(dt)
    return mu, value, h, c


def record(agent, snaps, batch, start):
    """Everything one ``play_steps_rnn()`` left behind, as clones: every ``agent.buf`` tensor, the stored and the live LSTM
    state (``start``: the live state in front of the call), last values, done flags, observation, episode accumulators,
    meters and rollout counter, the batch's tensors, and the env snapshots ``snaps`` on the host."""
    rec = {k: v.clone() for k, v in agent.buf.items()}
    rec.update(mb_h=agent.mb_rnn_states[0][0].clone(), mb_c=agent.mb_rnn_states[1][0].clone(),
               h_end=agent.rnn_states[0][0].clone(), c_end=agent.rnn_states[1][0].clone(), h_start=start[0], c_start=start[1],
               last_values=agent.last_values.clone(), dones_end=agent.dones.clone(), obs_end=agent.obs.clone(),
               cur_r=agent.current_rewards.clone(), cur_l=agent.current_lengths.clone())
    f = getattr(agent, "_fast", None)
    if f is not None:                     # the hand-written inference: its operand copy of h, the device meters and counter
        rec.update(h_operand=f["xh2"][f["cur"]][:, f["XW"]:].clone(), meter=agent.meter.clone(),
                   counter=int(agent.roll_counter))
    else:
        rec["meter"] = torch.stack([agent.game_rewards.mean[0], agent.game_rewards.current_size,
                                    agent.game_lengths.mean[0], agent.game_lengths.current_size]).clone()
    rec["assembled"] = bool(batch.get("assembled", False))
    for k in ("returns", "old_values", "values", "advantages", "obs", "obses", "actions", "dones", "mu", "mus", "sigma",
              "sigmas", "old_logp_actions", "neglogpacs"):
        if k in batch:
            rec["batch_" + k] = batch[k].clone()
    rec["batch_rnn_states"] = [s.clone() for s in batch["rnn_states"]]
    if "vms_pending" in batch:
        rec["vms_pending"] = batch["vms_pending"].clone()
    rec["snaps"] = [{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in s.items()} for s in snaps]
    return rec


def neglogp(actions, mu, sigma):
    """-log N(actions; mu, sigma), summed over the action components."""
    A = actions.shape[-1]
    return (0.5 * (((actions - mu) / sigma) ** 2).sum(-1) + 0.5 * math.log(2.0 * math.pi) * A + torch.log(sigma).sum(-1))


def replay(m, rec, h0, c0, seq_len, control=None):
    """The network side of one rollout ``rec`` (see tests/test_rollout_record.py ``_record``) in the dtype of ``m``'s
    parameters.  ``h0`` / ``c0`` [N, H]: the reference's own state behind the previous rollout (zeros before the first).
    -> dict of mus [T, N, A], sigmas [A], values [T, N, 1], neglogpacs [T, N], snap_h / snap_c [N, T / seq_len, H] (the
    reference's own state carried over ``seq_len`` steps from the previous stored snapshot), h_end / c_end [N, H] (carried
    from the last snapshot to behind the last step), last_values [N, 1] (from the record's final observation and state)."""
    assert control is None or control in CONTROLS, control
    dt = h0.dtype
    T = rec["obses"].shape[0]
    flags = torch.cat([rec["dones"], rec["dones_end"][None]]).to(dt)          # [T + 1, N]: flags[n + 1] = done in step n
    unit = control == "normaliser at 0 / 1"
    h, c = h0, c0
    h_before = None                                 # h in front of the previous step (what the other operand copy holds)
    mus, values, snap_h, snap_c = [], [], [], []
    for n in range(T):
        if n % seq_len == 0:
            k = n // seq_len
            snap_h.append(h); snap_c.append(c)
            h, c = rec["mb_h"][:, k].to(dt), rec["mb_c"][:, k].to(dt)
        h_in = h_before if (control == "h two steps back" and h_before is not None) else h
        h_before = h
        mu, value, h, c = policy_step(m, rec["obses"][n], h_in, c, unit)
        mus.append(mu); values.append(value)
        if control != "state not zeroed":
            keep = (1.0 - flags[n if control == "dones shifted" else n + 1]).unsqueeze(-1)
            h, c = h * keep, c * keep
        if control == "snapshot one step late" and n % seq_len == 0:
            snap_h[-1], snap_c[-1] = h, c
    h_last, c_last = rec["h_end"].to(dt), rec["c_end"].to(dt)
    if control == "last values one step on":
        _, _, h_last, c_last = policy_step(m, rec["obs_end"], h_last, c_last, unit)
    last_values = policy_step(m, rec["obs_end"], h_last, c_last, unit)[1]
    mus = torch.stack(mus)
    sigmas = torch.exp(m.a2c_network.sigma)
    return {"mus": mus, "sigmas": sigmas, "values": torch.stack(values),
            "neglogpacs": neglogp(rec["actions"].to(dt), mus, sigmas),
            "snap_h": torch.stack(snap_h, 1), "snap_c": torch.stack(snap_c, 1), "h_end": h, "c_end": c,
            "last_values": last_values}


# --------------------------------------------------------------------------- sampling
def noise_statistics(eps):
    """``eps`` [S, N, A] (S consecutive steps): mean, standard deviation, lag-1 correlation across steps and across
    neighbouring envs, and the number of draws that repeat another one (to 3e-6: ``eps`` is recomputed from rounded
    actions, which moves it by up to ~1e-6)."""
    e = eps.double()
    mean, std = float(e.mean()), float(e.std())
    z = (e - e.mean()) / e.std()
    steps = float((z[1:] * z[:-1]).mean())
    envs = float((z[:, 1:] * z[:, :-1]).mean())
    flat = e.reshape(-1, e.shape[-1])
    flat = flat[torch.argsort(flat[:, 0])]
    repeats = 0
    for lag in (1, 2, 3):
        repeats += int(((flat[lag:] - flat[:-lag]).abs().max(dim=1).values < 3e-6).sum())
    return {"mean": mean, "std": std, "lag1_steps": steps, "lag1_envs": envs, "repeats": repeats}


# --------------------------------------------------------------------------- env
def reset_margins(cfg, state):
    """Distance of every reset criterion of compute_reset from its threshold, from the float64 oracle's state behind a step
    -> [4, N]: tip distance - SUCCESS_DIST, |cart_y| - soft limit, tip_y - target_y, mean contact force (0: no contact)."""
    s = np.asarray(state, np.float64)
    dist = np.hypot(s[abi.VF_TIP_Y] - s[abi.VF_TARGET_Y], s[abi.VF_TIP_Z] - s[abi.VF_TARGET_Z])
    return np.stack([dist - float(cfg.success_dist), np.abs(s[abi.VF_CART_Y]) - float(cfg.rail_soft_limit),
                     s[abi.VF_TIP_Y] - s[abi.VF_TARGET_Y], s[abi.VF_CONTACT_MEAN]])


def undecided(cfg, f32, f64):
    """Env-steps [T, N] whose flags float32 round-off may decide: the two oracles, stepped from the same snapshot, disagree
    on a flag, or the float64 oracle puts a criterion within ``NEAR`` of its threshold."""
    differ = (f32["reset"] != f64["reset"]) | (f32["timeouts"] != f64["timeouts"])
    mg = f64["margins"]
    near = (np.abs(mg[:, :3]) < NEAR).any(1) | ((mg[:, 3] != 0.0) & (np.abs(mg[:, 3]) < NEAR))
    return differ | near


def oracle_steps(cfg, precision, snaps, actions):
    """One oracle step from each device snapshot (``state`` [VF_COUNT, N], ``reset``, ``progress``, ``step_count``: what
    the env held in front of the step) with that step's stored actions -> dict of obs [T, N, F], rew [T, N], reset [T, N],
    timeouts [T, N], progress [T, N], the state block behind the step [T, VF_COUNT, N] (float64) and, float64 only, margins
    [T, 4, N]."""
    from oracle import vine_oracle as vo
    orc = vo.OracleEnv(cfg, precision)
    out = {"obs": [], "rew": [], "reset": [], "timeouts": [], "progress": [], "state": [], "margins": []}
    for snap, a in zip(snaps, actions):
        orc.state[:] = snap["state"].astype(orc.real)
        orc.reset_buf[:] = snap["reset"]
        orc.progress[:] = snap["progress"]
        orc.step_count = snap["step_count"]
        orc.step(a)
        out["obs"].append(orc.obs.copy()); out["rew"].append(orc.rew.copy())
        out["reset"].append(orc.reset_buf.copy()); out["timeouts"].append(orc.timeouts.copy())
        out["progress"].append(orc.progress.copy()); out["state"].append(np.array(orc.state, np.float64))
        if precision == "f64":
            out["margins"].append(reset_margins(cfg, orc.state))
    orc.close()
    return {k: np.stack(v) for k, v in out.items() if v}


# --------------------------------------------------------------------------- bookkeeping, GAE, value normaliser
class Books:
    """The episode accumulators and the two windowed meters of ``play_steps`` (rl_games ``AverageMeter.update`` with the
    step's finished episodes as one batch) in float64."""

    def __init__(self, n, max_size):
        self.cur_r, self.cur_l = np.zeros(n), np.zeros(n)
        self.mean, self.size, self.max_size = [0.0, 0.0], [0.0, 0.0], float(max_size)
        self.last, self.last_abs = (0.0, 0.0, 0.0), 0.0
        self.steps = 0
        self.scale = 1.0             # largest |partial sum| seen: what float32 round-off of the accumulators scales with

    def step(self, rew, done):
        fin_r, fin_l = self.cur_r + rew, self.cur_l + 1.0
        self.scale = max(self.scale, float(np.abs(fin_r).max()))
        d = done != 0
        count = float(d.sum())
        self.last = (float(fin_r[d].sum()), float(fin_l[d].sum()), count)
        self.last_abs = float(np.abs(fin_r[d]).sum())
        if count > 0:
            sc = min(count, self.max_size)
            for i, total in enumerate(self.last[:2]):
                old = min(self.max_size - sc, self.size[i])
                self.mean[i] = (self.mean[i] * old + total / count * sc) / (old + sc)
                self.size[i] = old + sc
        self.cur_r, self.cur_l = np.where(d, 0.0, fin_r), np.where(d, 0.0, fin_l)
        self.steps += 1

    def meter(self):
        return np.array([self.mean[0], self.size[0], self.mean[1], self.size[1], *self.last])


def gae(rewards, values, dones, last_values, dones_end, gamma, tau):
    """rl_games ``discount_values`` in float64 -> advantages, returns [T, N, 1]."""
    r, v = rewards.double(), values.double()
    d = torch.cat([dones, dones_end[None]]).double().unsqueeze(-1)
    nxt_v = torch.cat([v[1:], last_values.double()[None]])
    lam = torch.zeros_like(v[0])
    advs = torch.zeros_like(v)
    for t in reversed(range(r.shape[0])):
        nonterminal = 1.0 - d[t + 1]
        delta = r[t] + gamma * nxt_v[t] * nonterminal - v[t]
        lam = delta + gamma * tau * nonterminal * lam
        advs[t] = lam
    return advs, advs + v


def rms_update(mean, var, count, x):
    """``RunningMeanStd.update`` (the parallel-variance merge) of scalar statistics with the batch ``x``, in float64."""
    x = x.double().reshape(-1)
    n = float(x.numel())
    delta = float(x.mean()) - mean
    tot = count + n
    m2 = var * count + float(x.var(unbiased=True)) * n + delta * delta * count * n / tot
    return mean + delta * n / tot, m2 / tot, tot
