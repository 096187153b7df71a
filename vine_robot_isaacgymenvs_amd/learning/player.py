"""Inference player (``test=True`` of train.py:166-171; deployment consumer
isaacgymenvs/vine_robot_test_model.py:143-177): loads a checkpoint and runs the deterministic policy.

Two paths.  The stock path evaluates the stock model through PyTorch and steps through ``VecTask.step``; it serves every
configuration.  The device path (the default network on the four-lanes-per-env step kernel, see ``_device_eligible``) is
three hand-written launches per step -- the trainer's split MLP and LSTM step (``FastInferenceMixin``) and
``vine_step_eval`` (include/vine_ppo.h), which applies the policy head, steps the env and accounts for episodes --
replayed as one hipGraph of ``player.graph_steps`` steps.  It reports per-episode task statistics (``eval_report``)."""
import math

import numpy as np
import torch

from .. import abi
from . import graph_capture
from .fast_inference import FastInferenceMixin
from .network import ModelA2CContinuousLogStd

REPORT_KEYS = ("episodes", "return_mean", "length_mean", "reached_ever_rate", "reached_at_end_rate", "steps_to_reach_mean",
               "final_dist_mean", "min_dist_mean", "end_timeout_rate", "end_rail_limit_rate", "end_tip_limit_rate",
               "end_contact_rate")


def eval_report(totals_rows):
    """The evaluation report from ``vine_step_eval``'s per-workgroup totals ([rows, abi.EVAL_NUM_TOTALS]): the rows are
    folded in float64; a mean over zero episodes (or zero reaching episodes) is ``nan``."""
    t = np.asarray(totals_rows, dtype=np.float64).reshape(-1, abi.EVAL_NUM_TOTALS).sum(axis=0)
    games, reached = t[abi.EVAL_EPISODES], t[abi.EVAL_REACHED_EVER]

    def per(x, n):
        return float(x) / float(n) if n > 0 else math.nan

    return {"episodes": int(round(games)),
            "return_mean": per(t[abi.EVAL_RETURN_SUM], games),
            "length_mean": per(t[abi.EVAL_LENGTH_SUM], games),
            "reached_ever_rate": per(reached, games),
            "reached_at_end_rate": per(t[abi.EVAL_REACHED_AT_END], games),
            "steps_to_reach_mean": per(t[abi.EVAL_FIRST_REACH_SUM], reached),
            "final_dist_mean": per(t[abi.EVAL_FINAL_DIST_SUM], games),
            "min_dist_mean": per(t[abi.EVAL_MIN_DIST_SUM], games),
            "end_timeout_rate": per(t[abi.EVAL_END_TIMEOUT], games),
            "end_rail_limit_rate": per(t[abi.EVAL_END_RAIL_LIMIT], games),
            "end_tip_limit_rate": per(t[abi.EVAL_END_TIP_LIMIT], games),
            "end_contact_rate": per(t[abi.EVAL_END_CONTACT], games)}


def format_report(report):
    """One line per quantity of ``eval_report`` (the stock path's report holds the first three only)."""
    lines = ["episodes: %d" % report["episodes"]]
    for k in REPORT_KEYS[1:]:
        if k in report:
            lines.append("%s: %.6g" % (k, report[k]))
    return "\n".join("  " + line for line in lines)


DRAW_OBSERVERS = ("env_sensor", "env_push", "env_target")      # whose named draws the episode log joins to its rows


def _has_any(env, *names):
    """Is one of the env's properties ``names`` there and not ``None``?"""
    return any(getattr(env, name, None) is not None for name in names)


class PpoPlayerContinuous(FastInferenceMixin):
    def __init__(self, params, vec_env=None):
        self.config = config = params["config"]
        self.vec_env = vec_env
        from ..utils.rlgames_utils import RLGPUEnv
        if self.vec_env is None:
            self.vec_env = RLGPUEnv(config["env_name"], config["num_actors"])
        elif not hasattr(self.vec_env, "get_env_info"):
            self.vec_env = RLGPUEnv.wrap(self.vec_env)
        info = self.vec_env.get_env_info()
        self.device = torch.device(config.get("device", "cuda:0"))
        self.actions_num = info["action_space"].shape[0]
        self.obs_shape = tuple(info["observation_space"].shape)
        self.normalize_input = config["normalize_input"]
        self.model = ModelA2CContinuousLogStd(params["network"], self.actions_num, self.obs_shape,
                                              config.get("normalize_value", False), self.normalize_input).to(self.device)
        self.model.eval()
        pcfg = config.get("player", None) or {}
        self.is_deterministic = pcfg.get("deterministic", True)
        self.max_steps = pcfg.get("max_steps", 27000)
        self.device_rollout = pcfg.get("device_rollout", True) is not False
        self.graph_steps = int(pcfg.get("graph_steps", 16))      # steps per captured graph (0: eager)
        if self.graph_steps < 0 or self.graph_steps % 2:
            # the observation and the LSTM operand each alternate between two buffers: a graph must end where it began
            raise ValueError("player.graph_steps must be 0 or a positive even number")
        seed = config.get("seed", None)
        self.eval_seed = int(seed) if seed is not None and int(seed) >= 0 else 0    # Philox key of sampled actions
        self.states = None
        self.report = None           # filled by run()
        self.device_path = None      # which path the last run() took
        self._fast = None
        self._dev = None
        self._eval_graph = None

    def restore(self, fn):
        ckpt = torch.load(fn, map_location=self.device, weights_only=False)
        self.model.load_state_dict(ckpt["model"])

    def init_rnn(self, batch):
        self.states = [s.clone() for s in self.model.get_default_rnn_state(batch, self.device)]

    @torch.no_grad()
    def get_action(self, obs, is_deterministic=True):
        if self.states is None:
            self.init_rnn(obs.shape[0])
        res = self.model({"is_train": False, "prev_actions": None, "obs": obs, "rnn_states": self.states})
        self.states = list(res["rnn_states"])
        action = res["mus"] if is_deterministic else res["actions"]
        return torch.clamp(action, -1.0, 1.0)

    def run(self, n_steps=None):
        """Plays ``n_steps`` env steps (default: max_steps); returns mean episode return and length and leaves the
        report in ``self.report``."""
        n_steps = n_steps or self.max_steps
        self.device_path = self._device_eligible()
        if self.device_path:
            return self._run_device(n_steps)
        return self._run_stock(n_steps)

    def _finish(self, mean_r, mean_l, games):
        env = getattr(self.vec_env, "env", self.vec_env)
        for side in (getattr(env, "video", None), getattr(env, "trajectory", None), getattr(env, "episode_log", None)):
            if side is not None:                 # CAPTURE_VIDEO / RECORD_TRAJECTORIES / EPISODE_LOG: what was harvested is on
                torch.cuda.synchronize(self.device)                                      # disk when run() returns
                side.drain()
        print("reward:", mean_r, "steps:", mean_l, "games:", games)
        print(format_report(self.report))
        if getattr(env, "episode_log", None) is not None and env.episode_log.table is not None:
            print(self._binned_report(env))
            # ENV_PARAMS: the same rate against every varying parameter; ENV_SENSOR: and against the sensor's values; ENV_PUSH:
            # and against the push's (by impulse: how large a kick the checkpoint survives); ENV_TARGET: and against the target's (by
            # velocity: how fast a target the checkpoint still reaches)
            if _has_any(env, "env_params", *DRAW_OBSERVERS):
                print(self._param_report(env))
        return mean_r, mean_l

    # ------------------------------------------------------------------ EPISODE_LOG
    def _episodes_begin(self, env):
        """The log's totals and the env's step count when a run starts: the run reports the episodes finished since."""
        log = getattr(env, "episode_log", None)
        if log is not None:
            log.harvest()
            self._episodes_start = (log.folded_totals(), int(env.step_count))

    def _binned_report(self, env, bins=5):
        """``reached_ever_rate`` of this run's episodes by obstacle depth when an obstacle is configured, else by target z."""
        from ..utils import episodes
        rows = env.episode_log.rows()
        keep = rows["end_step"] >= self._episodes_start[1]
        rows = {k: v[keep] for k, v in rows.items()}
        obstacle = bool(env.cfg["env"].get("CREATE_SHELF", False) or env.cfg["env"].get("CREATE_PIPE", False))
        column = "obj_depth" if obstacle else "target_z"
        if not len(rows["env"]):
            return "  reached_ever_rate by %s: no episode finished" % column
        rate, count, edges = episodes.binned_rate(rows, column, bins)
        lines = ["  reached_ever_rate by %s:" % column]
        lines += ["    [%.4g, %.4g%s  %.4g  (%d episodes)" % (edges[i], edges[i + 1], "]" if i == len(rate) - 1 else ")", rate[i],
                                                            count[i]) for i in range(len(rate))]
        return "\n".join(lines)

    def _param_report(self, env, bins=5, exact=16):
        """``reached_ever_rate`` of this run's episodes by every parameter of the bound per-env table that varies across
        the envs: by exact value where the envs hold at most ``exact`` distinct ones (a ``values`` entry of ``ENV_PARAMS``),
        else by bin.  Also kept in ``self.report["by_param"]``: name -> (values or bin edges, rate, episode count)."""
        from ..utils import episodes
        # ENV_PARAMS_PER_EPISODE: the plant of every row's own episode; ENV_SENSOR / ENV_PUSH / ENV_TARGET: the log joins their values
        # to its rows
        if _has_any(env, "env_redraw", *DRAW_OBSERVERS):
            rows = env.episode_log.rows_with_params()
            keep = rows["end_step"] >= self._episodes_start[1]
            rows = {k: v[keep] for k, v in rows.items()}
            per_env = {k[6:]: v for k, v in rows.items() if k.startswith("param_")}
        else:
            rows = env.episode_log.rows()
            keep = rows["end_step"] >= self._episodes_start[1]
            rows = {k: v[keep] for k, v in rows.items()}
            table = env.env_params_of(range(int(env.num_envs)))
            inertia = env.env_inertia_of(range(int(env.num_envs))) if getattr(env, "env_inertia", None) is not None else None
            per_env = episodes.varying_params(table, env.env_param_names, inertia)
            rows = episodes.with_env_params(rows, table, env.env_param_names, inertia)
        by_param, lines = {}, []
        for column in [k for k in rows if k.startswith("param_")]:
            lines.append("  reached_ever_rate by %s:" % column)
            if not len(rows["env"]):
                lines[-1] += " no episode finished"
                continue
            if len(np.unique(per_env[column[6:]])) <= exact:
                values, rate, count = episodes.value_rate(rows, column)
                by_param[column] = (values, rate, count)
                lines += ["    %.6g  %.4g  (%d episodes)" % (values[i], rate[i], count[i]) for i in range(len(values))]
            else:
                rate, count, edges = episodes.binned_rate(rows, column, bins)
                by_param[column] = (edges, rate, count)
                lines += ["    [%.4g, %.4g%s  %.4g  (%d episodes)" % (edges[i], edges[i + 1], "]" if i == len(rate) - 1 else ")",
                                                                    rate[i], count[i]) for i in range(len(rate))]
        self.report["by_param"] = by_param
        return "\n".join(lines)

    # ------------------------------------------------------------------ stock path
    def _run_stock(self, n_steps):
        env = getattr(self.vec_env, "env", self.vec_env)
        self._episodes_begin(env)
        obs = self.vec_env.reset()["obs"].to(self.device)
        n = obs.shape[0]
        cur_r = torch.zeros(n, device=self.device)
        cur_l = torch.zeros(n, device=self.device)
        sum_r = torch.zeros((), device=self.device)
        sum_l = torch.zeros((), device=self.device)
        games = torch.zeros((), device=self.device)
        for _ in range(n_steps):
            action = self.get_action(obs, self.is_deterministic)
            o, r, d, _ = self.vec_env.step(action)
            obs = o["obs"].to(self.device)
            d = d.to(self.device).float()
            cur_r += r.to(self.device)
            cur_l += 1
            sum_r += (cur_r * d).sum()
            sum_l += (cur_l * d).sum()
            games += d.sum()
            keep = 1.0 - d
            self.states = [s * keep.view(1, -1, 1) for s in self.states]
            cur_r *= keep
            cur_l *= keep
        g = max(float(games), 1.0)
        mean_r, mean_l = float(sum_r) / g, float(sum_l) / g
        played = int(games) > 0
        self.report = {"episodes": int(games), "return_mean": mean_r if played else math.nan,
                       "length_mean": mean_l if played else math.nan}
        log = getattr(env, "episode_log", None)
        if log is not None:                      # EPISODE_LOG: the task figures of the episodes the log saw finish in this run
            full = eval_report(log.folded_totals() - self._episodes_start[0])
            self.report.update({k: full[k] for k in REPORT_KEYS[3:]})
        return self._finish(mean_r, mean_l, int(games))

    # ------------------------------------------------------------------ device path
    def _device_eligible(self):
        """The device path serves the default network (256-128-64 MLP, LSTM 256 with LayerNorm, 2 actions) at a multiple
        of 512 envs on the four-lanes-per-env step kernel; everything else stays on the stock path."""
        env = getattr(self.vec_env, "env", self.vec_env)
        if not (self.device_rollout and self.device.type == "cuda" and hasattr(env, "eval_step_rows")
                and hasattr(env, "timeout_buf") and env.rew_buf.is_cuda and env.rew_buf.device == self.device
                and self.actions_num == 2 and float(getattr(env, "clip_actions", 1.0)) <= 1.0
                and int(env.num_envs) % 512 == 0 and self.normalize_input):
            return False
        if env.eval_step_rows() <= 0:            # (0 with a MAT_FILE too)
            return False
        if self._fast is None:
            from . import fused
            self.num_actors = int(env.num_envs)
            self.fused_rollout, self.rollout_lp16, self._pending_fin = True, False, None
            self.rollout_f32_terms = int(self.config.get("rollout_f32_terms", fused.ROLLOUT_F32_SPLIT))
            self.rnn_states = [s.contiguous() for s in self.model.get_default_rnn_state(self.num_actors, self.device)]
            self._setup_fast_inference()
        f = self._fast
        return bool(f is not None and f["f32_mfma"] and f.get("mlp_wt_split") is not None and f["ln_in_head"])

    def _device_buffers(self, env):
        if self._dev is None:
            N, dev = self.num_actors, self.device
            rows = env.eval_step_rows()
            self._dev = {"obs_ring": [torch.zeros((N,) + self.obs_shape, device=dev) for _ in range(2)], "slot": 0,
                         "episode": torch.zeros((abi.EVAL_EPISODE_FIELDS, N), device=dev),
                         "totals": torch.zeros((rows, abi.EVAL_NUM_TOTALS), device=dev, dtype=torch.float64),
                         "mu": torch.zeros((N, 2), device=dev), "action": torch.zeros((N, 2), device=dev),
                         "dones": torch.zeros(N, device=dev, dtype=torch.uint8),
                         "hw": torch.empty(3 * 256, device=dev), "hc": torch.empty(3, device=dev)}
        return self._dev

    def _device_step(self):
        """One step: the split MLP, the split LSTM step, ``vine_step_eval``."""
        env = getattr(self.vec_env, "env", self.vec_env)
        d = self._dev
        y = self._infer(d["obs_ring"][d["slot"]])
        a = abi.EvalArgs()
        self._fill_head_args(a, y, d["hw"], d["hc"])
        a.deterministic, a.seed = int(bool(self.is_deterministic)), self.eval_seed
        a.mu_out, a.action_out, a.dones_out = d["mu"].data_ptr(), d["action"].data_ptr(), d["dones"].data_ptr()
        a.episode, a.totals = d["episode"].data_ptr(), d["totals"].data_ptr()
        d["slot"] ^= 1
        env.step_eval_into(a, d["obs_ring"][d["slot"]])

    def _capture(self, env):
        """``graph_steps`` steps as one graph, as the trainer captures its rollout: a warm-up pass on a side stream whose
        effects are rolled back (env state, step count -- the key of sampled actions --, LSTM state, accounting), then the
        capture pass, which executes nothing (``graph_capture.capture_rolled_back``)."""
        d, f = self._dev, self._fast
        live = [self.rnn_states[0], self.rnn_states[1], f["xh2"][0], f["xh2"][1], d["obs_ring"][0], d["obs_ring"][1],
                d["episode"], d["totals"], d["mu"], d["action"], d["dones"]]
        num_steps = env.num_steps

        def body():
            for _ in range(self.graph_steps):
                self._device_step()

        graph = graph_capture.capture_rolled_back(self.device, body, live + env.live_tensors(), env)
        env.num_steps = num_steps
        return graph

    @torch.no_grad()
    def _run_device(self, n_steps):
        env = getattr(self.vec_env, "env", self.vec_env)
        self._episodes_begin(env)
        d = self._device_buffers(env)
        obs = self.vec_env.reset()["obs"]
        d["slot"] = 0
        d["obs_ring"][0].copy_(obs)
        for s in self.rnn_states:
            s.zero_()
        d["episode"].zero_()
        d["episode"][abi.EVAL_EP_MIN_DIST].fill_(math.inf)
        d["totals"].zero_()
        # operand copies of the weights (restore() may have changed them since the last run) and of h
        self._infer_begin()
        self._head_prep(d["hw"], d["hc"])
        # CAPTURE_VIDEO: eager throughout (the capture schedule is not wired into this graph).  RECORD_TRAJECTORIES and
        # EPISODE_LOG are: their launches are captured with the steps, and the host is told of every replay.
        graphed = self.graph_steps > 0 and n_steps >= self.graph_steps and getattr(env, "video", None) is None
        done = 0
        if graphed:
            if self._eval_graph is None:
                self._eval_graph = self._capture(env)
            for _ in range(n_steps // self.graph_steps):
                graph_capture.replay_observed(self._eval_graph, env, self.graph_steps)
                env.num_steps += self.graph_steps
            done = n_steps // self.graph_steps * self.graph_steps
        for _ in range(n_steps - done):
            self._device_step()
        totals = d["totals"].cpu().numpy()           # the only device -> host copy; synchronises
        self.report = eval_report(totals)
        return self._finish(self.report["return_mean"], self.report["length_mean"], self.report["episodes"])
