"""``Vine5LinkMovingBase`` task: host-side mirror of the reference task class
(isaacgymenvs/tasks/Vine5LinkMovingBase.py:90-1455) on top of the fused HIP step.

The per-step work of the reference's hooks -- ``pre_physics_step`` (V5:922), the 4x
``compute_and_set_dof_actuation_force_tensor`` + ``gym.simulate`` loop (V5:1028; vec_task.py:338-356),
``post_physics_step`` (V5:1110) with ``reset_idx`` (V5:774), ``compute_observations`` (V5:1339) and
``compute_reward`` (V5:1218) -- is one kernel launch behind ``vine_step`` (include/vine.h).
This class keeps the constructor signature, the buffers and the attributes callers read.
"""
import contextlib
import ctypes as C
import logging
import os
from enum import Enum

import torch

from .. import abi, native
from .base.vec_task import VecTask

# Same constants as V5:48-88
NUM_XYZ = 3
NUM_OBJECT_INFO = 2
N_REVOLUTE_DOFS = 5
N_PRISMATIC_DOFS = 1
N_PRESSURE_ACTIONS = 1
INIT_X, INIT_Y, INIT_Z = 0.0, 0.0, 1.0
CART_Z = 0.975  # 1.0 - 0.025 (URDF slider_to_cart origin)

REWARD_NAMES = ["Position", "Const Negative", "Position Success",
                "Velocity Success", "Velocity", "Rail Velocity Control",
                "FPAM Control", "Rail Velocity Change", "FPAM Change", "Rail Limit",
                "Cart Y", "Tip Y", "Contact Force"]
_REWARD_KEYS = ["POSITION", "CONST_NEGATIVE", "POSITION_SUCCESS", "VELOCITY_SUCCESS", "VELOCITY",
                "U_RAIL_VELOCITY_CONTROL", "U_FPAM_CONTROL", "RAIL_VELOCITY_CHANGE", "U_FPAM_CHANGE",
                "RAIL_LIMIT", "CART_Y", "TIP_Y", "CONTACT_FORCE"]


class ObservationType(Enum):
    POS_ONLY = "POS_ONLY"
    POS_AND_VEL = "POS_AND_VEL"
    POS_AND_FD_VEL = "POS_AND_FD_VEL"
    POS_AND_PREV_POS = "POS_AND_PREV_POS"
    POS_AND_FD_VEL_AND_OBJ_INFO = "POS_AND_FD_VEL_AND_OBJ_INFO"
    TIP_AND_CART_AND_OBJ_INFO = "TIP_AND_CART_AND_OBJ_INFO"


def num_observations(observation_type: ObservationType) -> int:
    """V5:152-170."""
    if observation_type == ObservationType.POS_ONLY:
        return N_REVOLUTE_DOFS + N_PRISMATIC_DOFS + NUM_XYZ + NUM_XYZ + N_PRESSURE_ACTIONS + N_PRISMATIC_DOFS
    if observation_type == ObservationType.TIP_AND_CART_AND_OBJ_INFO:
        return 2 * (N_PRISMATIC_DOFS + NUM_XYZ + NUM_XYZ) + N_PRESSURE_ACTIONS + N_PRISMATIC_DOFS + NUM_OBJECT_INFO
    n = 2 * (N_REVOLUTE_DOFS + N_PRISMATIC_DOFS + NUM_XYZ + NUM_XYZ) + N_PRESSURE_ACTIONS + N_PRISMATIC_DOFS
    if observation_type == ObservationType.POS_AND_FD_VEL_AND_OBJ_INFO:
        n += NUM_OBJECT_INFO
    return n


def vine_config_from_cfg(cfg, lib, seed=None):
    """Freeze the task config dict (reference YAML keys, cfg/task/Vine5LinkMovingBase.yaml) into the flat
    ``VineConfig`` handed to the C ABI.  Raises like the reference for what it cannot do."""
    env, sim, task = cfg["env"], cfg["sim"], cfg["task"]
    c = abi.VineConfig()
    native.check(lib.vine_config_default(C.byref(c)), lib)
    observation_type = ObservationType[env["OBSERVATION_TYPE"]]
    scale_observations = bool(env.get("SCALE_OBSERVATIONS", True))
    if scale_observations and abi.OBS_TYPE_BY_NAME[observation_type.value] not in abi.SCALABLE_OBS_TYPES:
        # the reference raises the same for these types whenever SCALE_OBSERVATIONS is on (V5:267-268)
        raise NotImplementedError(f"Observation scaling not implemented for {observation_type}")
    native.check(lib.vine_config_set_obs_type(C.byref(c), abi.OBS_TYPE_BY_NAME[observation_type.value],
                                              int(scale_observations)), lib)
    if not env.get("USE_MOVING_BASE", True):
        raise NotImplementedError("Not implemented for non-moving base")   # V5:898
    c.num_envs = int(env["numEnvs"])
    c.control_freq_inv = int(env.get("controlFrequencyInv", 1))
    c.max_episode_length = int(env["maxEpisodeLength"])
    c.action_delay = int(env.get("ACTION_DELAY", 0))
    c.clip_observations = float(env.get("clipObservations", float("inf")))
    c.clip_actions = float(env.get("clipActions", float("inf")))
    c.dt = float(sim["dt"])
    c.substeps = int(sim.get("substeps", 2))
    gravity = sim.get("gravity", [0.0, 0.0, -9.81])
    if sim.get("up_axis", "z") != "z" or float(gravity[0]) != 0.0 or float(gravity[1]) != 0.0:
        raise ValueError("Vine5LinkMovingBase requires up_axis 'z' and gravity along -z (V5:441)")
    c.gravity = -float(gravity[2])
    for key, field in [("FPAM_MIN", "fpam_min"), ("FPAM_MAX", "fpam_max"), ("RAIL_VELOCITY_SCALE", "rail_velocity_scale"),
                       ("DAMPING", "damping"), ("STIFFNESS", "stiffness"), ("RAIL_SOFT_LIMIT", "rail_soft_limit"),
                       ("RAIL_P_GAIN", "rail_p_gain"), ("RAIL_D_GAIN", "rail_d_gain"),
                       ("RAIL_ACCELERATION", "rail_acceleration"),
                       ("SMOOTHING_ALPHA_INFLATE", "smoothing_alpha_inflate"),
                       ("SMOOTHING_ALPHA_DEFLATE", "smoothing_alpha_deflate"),
                       ("RANDOM_INIT_CART_MIN_Y", "random_init_cart_min_y"),
                       ("RANDOM_INIT_CART_MAX_Y", "random_init_cart_max_y"), ("SUCCESS_DIST", "success_dist"),
                       ("MIN_TARGET_DEPTH_IN_OBSTACLE", "min_target_depth"),
                       ("MAX_TARGET_DEPTH_IN_OBSTACLE", "max_target_depth"),
                       ("MIN_TARGET_Y", "min_target_y"), ("MAX_TARGET_Y", "max_target_y"),
                       ("MIN_TARGET_Z", "min_target_z"), ("MAX_TARGET_Z", "max_target_z")]:
        setattr(c, field, float(env[key]))
    for i, key in enumerate(_REWARD_KEYS):
        c.reward_weights[i] = float(env[key + "_REWARD_WEIGHT"])
    rp = task.get("randomization_parameters", {})
    c.dyn_scale_min = float(rp.get("DYNAMICS_SCALING_MIN", 1.0))
    c.dyn_scale_max = float(rp.get("DYNAMICS_SCALING_MAX", 1.0))
    c.obs_noise_std = float(rp.get("OBSERVATION_NOISE_STD", 0.0))
    c.action_noise_std = float(rp.get("ACTION_NOISE_STD", 0.0))
    for flag, on in [(abi.FLAG_USE_SMOOTHED_FPAM, env.get("USE_SMOOTHED_FPAM", True)),
                     (abi.FLAG_FORCE_U_FPAM, env.get("FORCE_U_FPAM", False)),
                     (abi.FLAG_FORCE_U_RAIL_VELOCITY, env.get("FORCE_U_RAIL_VELOCITY", False)),
                     (abi.FLAG_CREATE_SHELF, env.get("CREATE_SHELF", False)),
                     (abi.FLAG_CREATE_PIPE, env.get("CREATE_PIPE", False)),
                     (abi.FLAG_RANDOMIZE_DOF_INIT, env.get("RANDOMIZE_DOF_INIT", True)),
                     (abi.FLAG_RANDOMIZE_TARGETS, env.get("RANDOMIZE_TARGETS", True)),
                     (abi.FLAG_USE_TARGET_REACHED_RESET, env.get("USE_TARGET_REACHED_RESET", True)),
                     (abi.FLAG_USE_TIP_LIMIT_HIT_RESET, env.get("USE_TIP_LIMIT_HIT_RESET", False)),
                     (abi.FLAG_USE_NONZERO_CONTACT_FORCE_RESET, env.get("USE_NONZERO_CONTACT_FORCE_RESET", False)),
                     (abi.FLAG_VINE_RANDOMIZE, task.get("vine_randomize", False))]:
        c.set_flag(flag, bool(on))
    # physics-model switches of this build (not reference keys; see DESIGN.md "assumptions")
    model = env.get("physicsModel", {})
    c.set_flag(abi.FLAG_STALE_BODY_STATE_AFTER_RESET, bool(model.get("staleBodyStateAfterReset", True)))
    c.set_flag(abi.FLAG_IMPLICIT_JOINT_DAMPING, bool(model.get("implicitJointDamping", True)))
    c.set_flag(abi.FLAG_FPAM_DAMPING_HELD, bool(model.get("fpamDampingHeld", False)))
    c.link_angular_damping = float(model.get("linkAngularDamping", 0.0))
    c.effort_limit = float(model.get("effortLimit", 0.0))
    c.set_flag(abi.FLAG_INTROSPECT, bool(env.get("introspection", False)))
    c.env_id_offset = int(env.get("envIdOffset", 0))
    if seed is not None:
        c.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return c


class Vine5LinkMovingBase(VecTask):
    """Drop-in for ``isaacgym_task_map["Vine5LinkMovingBase"]`` (rlgames_utils.py:78-86)."""

    def __init__(self, cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture=False,
                 force_render=False):
        self.cfg = cfg
        self.logger = logging.getLogger(__name__)
        self.max_episode_length = self.cfg["env"]["maxEpisodeLength"]
        self.vine_randomize = self.cfg["task"]["vine_randomize"]

        observation_type = ObservationType[self.cfg["env"]["OBSERVATION_TYPE"]]
        self.cfg["env"]["numObservations"] = num_observations(observation_type)
        self.cfg["env"]["numActions"] = N_PRESSURE_ACTIONS + N_PRISMATIC_DOFS
        if self.cfg["env"].get("CREATE_PIPE", False):
            self.logger.info("CREATE_PIPE: the pipe mesh is simulated as its planar cross-section (two walls)")
        self._video = None
        self._trajectory = None
        self._episode_log = None
        self._env_redraw = None
        self._env_sensor = None
        self._env_push = None
        self._env_target = None
        self._env_draw_adr = None
        self._observers = []       # what rides behind every step: the video capture, the trajectory recorder, the episode log,
                                   # the per-episode redraw of the plants (last: it replaces what the others read)

        self._lib = None
        self._handle = None
        from ..utils import env_params
        self._per_episode = env_params.per_episode(self.cfg["env"])      # (refused here, before anything is created)
        self._adr = env_params.adr_config(self.cfg["env"], multi_gpu=int(os.getenv("WORLD_SIZE", "1")) > 1)
        from ..utils import env_sensor
        self._sensor_cfg = env_sensor.sensor_config(self.cfg["env"], self.cfg["env"]["numObservations"])
        from ..utils import env_push
        self._push_cfg = env_push.push_config(self.cfg["env"])
        from ..utils import env_target
        self._target_cfg = env_target.target_config(self.cfg["env"], env_target.control_period(
            self.cfg["sim"]["dt"], self.cfg["env"].get("controlFrequencyInv", 1)))
        from ..utils import env_draw_adr
        self._draw_adr_cfg = env_draw_adr.draw_adr_config(self.cfg["env"], self._sensor_cfg, self._push_cfg, self._target_cfg,
                                                          multi_gpu=int(os.getenv("WORLD_SIZE", "1")) > 1)
        super().__init__(config=self.cfg, rl_device=rl_device, sim_device=sim_device,
                         graphics_device_id=graphics_device_id, headless=headless,
                         virtual_screen_capture=virtual_screen_capture, force_render=force_render)

        self.num_dof = N_REVOLUTE_DOFS + N_PRISMATIC_DOFS
        self.reward_weights = torch.tensor([[self.cfg["env"][k + "_REWARD_WEIGHT"] for k in _REWARD_KEYS]],
                                           device=self.device, dtype=torch.float)
        self.index_to_view = int(0.1 * self.num_envs)
        self.num_steps = 0
        self.dt = self.cfg["sim"]["dt"]
        self.control_dt = self.dt * self.control_freq_inv
        self.obs_scaling = torch.tensor(list(self._vcfg.obs_scaling[:self.num_obs]), device=self.device)
        self.wandb_dict = {}
        self._reward_matrix = None
        self._stats_out = None
        self._introspection = bool(self._vcfg.flags & abi.FLAG_INTROSPECT)
        self.mat = self.read_mat_file(self.cfg["env"]["MAT_FILE"]) if len(self.cfg["env"].get("MAT_FILE", "")) > 0 else None
        # host-indexed state overwrite every step: cannot live inside a captured hipGraph
        self.graph_capturable = self.mat is None
        if self.mat is not None:
            # replay overwrites the DOF state before every step without moving the bodies: the step kernel must keep
            # reading the tip / cart rigid-body states from memory, which it does with introspection on
            self.set_introspection(True)
        if self._on_rank0("CAPTURE_VIDEO", "recorded"):
            self._setup_video()
        if self._on_rank0("RECORD_TRAJECTORIES", "recorded"):
            self._setup_trajectory()
        if self._on_rank0("EPISODE_LOG", "logged"):
            self._setup_episode_log()
        if self._target_cfg is not None:         # every rank, by the global env id; behind the observers that account for the
            self._setup_env_target()             # step as the plant left it, in front of the sensor, which senses its velocity
        if self._sensor_cfg is not None:         # every rank: each senses its own shard, by the global env id; in front of
            self._setup_env_sensor()             # the redraw, which stays last
        if self._push_cfg is not None:           # every rank, by the global env id; behind the sensor (which has then sensed
            self._setup_env_push()               # what the step wrote), in front of the redraw
        if self._draw_adr_cfg is not None:       # ENV_DRAW_ADR: behind the three whose freshly drawn rows it replaces
            self._setup_env_draw_adr()
        if self._adr is not None:                # ENV_PARAMS_ADR: the redraw's place, with ranges that move
            self._setup_env_adr()
        elif self._per_episode:                  # every rank: each redraws its own shard, by the global env id
            self._setup_env_redraw()

    # ------------------------------------------------------------------ step observers (utils/observers.py)
    def _on_rank0(self, key, done):
        """Is ``env.<key>`` on, and is this the rank that does it?  Every rank would write the same file names: rank 0
        records its env, the others launch nothing."""
        if not self.cfg["env"].get(key, False):
            return False
        if int(os.getenv("LOCAL_RANK", "0")) == 0:
            return True
        self.logger.info(f"{key}: {done} by rank 0 only")
        return False

    def _stamp(self):
        """``time_str`` (V5:145), made once: every observer's files carry the same stamp."""
        if not hasattr(self, "time_str"):
            import datetime
            self.time_str = datetime.datetime.now().strftime("%Y-%m-%d_%H-%M-%S")
        return self.time_str

    def _out_dir(self, key):
        return self.cfg["env"].get(key + "_DIR") or os.path.join("runs", self.cfg["name"])     # V5:140

    def _add_observer(self, observer):
        if self.env_params is not None and hasattr(observer, "env_params_of"):
            # ENV_PARAMS: a recording says which plant produced it, the episode file holds the table its env column indexes
            observer.env_params_of, observer.env_param_names = self.env_params_of, self.env_param_names
            if self.env_inertia is not None:     # ENV_INERTIA: and its masses, beside it
                observer.env_inertia_of, observer.env_inertia_names = self.env_inertia_of, self.env_inertia_names
        self._observers.append(observer)
        return observer

    @property
    def observers(self):
        """What rides behind every step, in launch order (the protocol: utils/observers.py)."""
        return list(self._observers)

    def live_tensors(self):
        """What a caller that rolls steps back (the warm-up pass in front of a graph capture) must save and restore of
        the env and of its observers (in their order: the episode log harvests here)."""
        live = [self._state, self.reset_buf, self.progress_buf, self.rew_buf, self.timeout_buf]
        for o in self._observers:
            live += o.live_tensors()
        return live

    @contextlib.contextmanager
    def observers_paused(self):
        """Steps enqueued inside are not counted by any observer (the warm-up and capture passes of a hipGraph, whose
        effects are rolled back or not executed at all)."""
        held = list(self._observers)
        for o in held:
            # such a pass still launches the draw / record kernels, which write the rings from the device's counter:
            # a harvest copy still in flight on an observer's side stream must have read its ring first
            if o.copy_done is not None and not torch.cuda.is_current_stream_capturing():
                torch.cuda.current_stream(self.device).wait_event(o.copy_done)
                o.copy_done = None
            o.paused += 1
        try:
            yield
        finally:
            for o in held:
                o.paused -= 1

    def observers_replayed(self, n_steps, before=False):
        """A captured graph holding ``n_steps`` steps (and their observers' launches) is about to be / has been
        replayed."""
        for o in self._observers:
            (o.before if before else o.advance)(n_steps)

    def _observe(self, actions, obs_out=None):
        """Behind a step launch: every observer's launch on the same stream, then its host-side count.  ``actions``:
        device address of the action buffer the step consumed; ``obs_out``: the observation tensor it wrote, handed to
        the observers that ask for it (``wants_obs``)."""
        for o in self._observers:
            if getattr(o, "wants_obs", False):
                o.enqueue(self._stream(), actions, obs=obs_out.data_ptr())
            else:
                o.enqueue(self._stream(), actions)
            o.advance(1)

    # ------------------------------------------------------------------ CAPTURE_VIDEO (V5:205-221, 1169-1207)
    def _setup_video(self):
        """The camera of V5:206-221 as a ``VineRenderConfig`` (include/vine_render.h), the device frame ring and the
        writer.  Frames are drawn by a launch behind every step."""
        from ..utils import video
        env = self.cfg["env"]
        torch.cuda.synchronize(self.device)
        tip_y = float(self._state[abi.VF_TIP_Y, self.index_to_view])         # cam_target, V5:206-207
        rcfg = video.render_config(self._lib, env, tip_y, INIT_Z)
        views = [(self.index_to_view + v) % self.num_envs for v in range(rcfg.num_views)]
        self.log_dir = self._out_dir("CAPTURE_VIDEO")
        self._video = self._add_observer(video.VideoCapture(
            self._lib, self._handle, rcfg, views, self.progress_buf, self.device, self.log_dir, self._stamp(),
            self.control_dt, self.logger))
        self.logger.info(f"CAPTURE_VIDEO: {rcfg.num_frames} frames of {rcfg.num_views} view(s) at "
                         f"{rcfg.width} x {rcfg.height} every {rcfg.capture_every} steps -> "
                         f"{self.log_dir}/{self.time_str}_video_<num_steps>.png")

    @property
    def video(self):
        """The ``VideoCapture`` of this env (``None`` unless ``CAPTURE_VIDEO``)."""
        return self._video

    # ------------------------------------------------------------------ RECORD_TRAJECTORIES (include/vine_record.h)
    def _setup_trajectory(self):
        """The recorded envs, the device row ring and the writer; rows are written by a launch behind every step, see
        utils/trajectory.py for the MAT files."""
        from ..utils import trajectory
        env = self.cfg["env"]
        every = int(env.get("RECORD_TRAJECTORIES_EVERY", 1000))
        steps = min(int(env.get("RECORD_TRAJECTORIES_STEPS", 0) or self.max_episode_length), every)
        which = env.get("RECORD_TRAJECTORIES_ENVS", 1)
        if isinstance(which, (int, float, str)):
            envs = [(self.index_to_view + k) % self.num_envs for k in range(int(which))]
        else:
            envs = [int(e) for e in which]
        if not 1 <= len(envs) <= abi.RECORD_MAX_ENVS:
            raise ValueError(f"RECORD_TRAJECTORIES_ENVS: 1 .. {abi.RECORD_MAX_ENVS} envs can be recorded, not {len(envs)}")
        if any(e < 0 or e >= self.num_envs for e in envs):
            raise ValueError(f"RECORD_TRAJECTORIES_ENVS: env indices must lie in [0, {self.num_envs}): {envs}")
        rcfg = trajectory.record_config(self._lib, every, steps, len(envs))
        directory = self._out_dir("RECORD_TRAJECTORIES")
        self._trajectory = self._add_observer(trajectory.TrajectoryRecorder(
            self._lib, self._handle, rcfg, envs, (self.rew_buf, self.reset_buf, self.progress_buf, self.timeout_buf),
            self.device, directory, self._stamp(), self.control_dt, self.logger))
        self.logger.info(f"RECORD_TRAJECTORIES: {steps} steps of env(s) {envs} every {every} steps -> "
                         f"{directory}/{self.time_str}_trajectory_<num_steps>_env<e>.mat")

    @property
    def trajectory(self):
        """The ``TrajectoryRecorder`` of this env (``None`` unless ``RECORD_TRAJECTORIES``)."""
        return self._trajectory

    # ------------------------------------------------------------------ EPISODE_LOG (include/vine_episodes.h)
    def _setup_episode_log(self):
        """The accumulators, totals and row ring of the per-episode task log; a launch behind every step keeps them, see
        utils/episodes.py for the harvest and the file.  The log reads the step's reward-matrix row, so a matrix is bound
        here (arming introspection) before anything is captured; one bound for a dashboard already is shared."""
        from ..utils import episodes
        env = self.cfg["env"]
        if self._reward_matrix is None:
            self.bind_reward_matrix()
        capacity = int(env.get("EPISODE_LOG_CAPACITY", 1048576))
        task = {k: env[k] for k in episodes.TASK_KEYS if k in env}
        self._episode_log = self._add_observer(episodes.EpisodeLog(
            self._lib, self._handle, self.num_envs, capacity, bool(env.get("EPISODE_LOG_TABLE", True)),
            (self.rew_buf, self.reset_buf, self.progress_buf, self.timeout_buf), self.device,
            self._out_dir("EPISODE_LOG"), self._stamp(), task, self.logger))
        self.logger.info(f"EPISODE_LOG: one row per finished episode (ring of {capacity}) -> {self._episode_log.path}")

    @property
    def episode_log(self):
        """The ``EpisodeLog`` of this env (``None`` unless ``EPISODE_LOG``)."""
        return self._episode_log

    # ------------------------------------------------------------------ the three observers with a table of named draws
    def _add_table_observer(self, key, observer, what):
        """What ENV_SENSOR, ENV_PUSH and ENV_TARGET do alike with their observer: into the launch order, onto the episode log
        (whose attribute ``key.lower()`` it becomes), and one log line: ``what``, then which names vary."""
        from ..utils import named_draw
        self._add_observer(observer)
        if self._episode_log is not None:
            setattr(self._episode_log, key.lower(), observer)
        varying = ", ".join(named_draw.varying(observer.NAMES, observer.spec))
        self.logger.info(f"ENV_{key}: {what}; {varying or 'nothing'} varies"
                         f"{', redrawn at every reset' if observer.spec['PER_EPISODE'] else ''}")
        return observer

    # ------------------------------------------------------------------ ENV_SENSOR (include/vine_env_sensor.h)
    def _setup_env_sensor(self):
        """A launch behind every step rewrites the observation that step wrote: per-env delay, dropped frames and noise
        (utils/env_sensor.py).  The step kernels are not touched: the four-lane kernel and the fused rollout step stay."""
        from ..utils import env_sensor
        self._env_sensor = self._add_table_observer("SENSOR", env_sensor.EnvSensor(
            self._lib, self._handle, self._vcfg, self._sensor_cfg, self.reset_buf, self.progress_buf, self.num_envs, self.num_obs,
            self.device), f"delay, dropped frames and noise on {len(self._sensor_cfg['COLUMNS'])} of {self.num_obs} observation columns")

    @property
    def env_sensor(self):
        """The ``EnvSensor`` of this env (``None`` unless ``ENV_SENSOR``)."""
        return self._env_sensor

    # ------------------------------------------------------------------ ENV_PUSH (include/vine_env_push.h)
    def _setup_env_push(self):
        """A launch behind every step adds, for the envs its draw selects, what a random impulse at a point of the chain does
        to the six generalised velocities (utils/env_push.py).  The step kernels are not touched: the four-lane kernel and
        the fused rollout step stay."""
        from ..utils import env_push
        self._env_push = self._add_table_observer("PUSH", env_push.EnvPush(
            self._lib, self._handle, self._vcfg, self._push_cfg, self.reset_buf, self.num_envs, self.device),
            f"impulses at point(s) {self._push_cfg['POINTS']}")

    @property
    def env_push(self):
        """The ``EnvPush`` of this env (``None`` unless ``ENV_PUSH``)."""
        return self._env_push

    # ------------------------------------------------------------------ ENV_TARGET (include/vine_env_target.h)
    def _setup_env_target(self):
        """A launch behind every step carries each env's target one control step along its bounded path in the state block
        the next step reads, and adds the target's velocity to the observation the step wrote (utils/env_target.py).  The
        step kernels are not touched: the four-lane kernel and the fused rollout step stay."""
        from ..utils import env_target
        if self.mat is not None:
            raise NotImplementedError("ENV_TARGET with MAT_FILE: the replay overwrites the target before every step")
        self._env_target = self._add_table_observer("TARGET", env_target.EnvTarget(
            self._lib, self._handle, self._vcfg, self._target_cfg, self.reset_buf, self.progress_buf, self.num_envs, self.num_obs,
            self.device), f"targets move in {env_target.MODES[self._target_cfg['MODE']]} mode")

    @property
    def env_target(self):
        """The ``EnvTarget`` of this env (``None`` unless ``ENV_TARGET``)."""
        return self._env_target

    # ------------------------------------------------------------------ ENV_DRAW_ADR (include/vine_env_draw_adr.h)
    def _setup_env_draw_adr(self):
        """Two launches behind every step, behind the target's, the sensor's and the push's, move the ranges of the names
        under ``ENV_DRAW_ADR.NAMES`` and replace the rows those three have just drawn for a flagged env: the ranges begin at
        START (the rows of episode 0 are overwritten here), the ``[lo, hi]`` of the three observers' mappings are their
        limits.  The launches read the step's reward matrix, so one is bound here (arming introspection) before anything is
        captured; one bound already is shared."""
        from ..utils import env_draw_adr
        if self._reward_matrix is None:
            self.bind_reward_matrix()
        self._env_draw_adr = self._add_observer(env_draw_adr.EnvDrawAdr(
            self._lib, self._handle, self._vcfg, self._draw_adr_cfg, self.reset_buf, self._env_sensor, self._env_push,
            self._env_target, self.device, self.logger))
        if self._episode_log is not None:
            self._episode_log.draw_adr = self._env_draw_adr
        self.logger.info(f"ENV_DRAW_ADR: the ranges of {', '.join(self._draw_adr_cfg['NAMES'])} start at START and move on the "
                         f"device by the reach rate of the episodes probing their boundaries")

    @property
    def env_draw_adr(self):
        """The ``EnvDrawAdr`` of this env (``None`` unless ``ENV_DRAW_ADR``)."""
        return self._env_draw_adr

    # ------------------------------------------------------------------ ENV_PARAMS_PER_EPISODE (include/vine_env_redraw.h)
    def _setup_env_redraw(self):
        """A launch behind every step redraws, on the device, the plant of every env that step flagged for a reset: episode
        ``k`` of global env ``g`` runs with ``env_params.draw_columns`` of ``(g, k)``.  From here on the SPEC owns the tables:
        ``env_params`` / ``env_inertia`` stay the device tensors, ``env_params_of`` / ``env_inertia_of`` read them, and
        ``set_env_params`` raises.  Envs reset from outside the step (``reset_idx``) keep their plant."""
        from ..utils import env_redraw
        spec = self.cfg["env"].get("ENV_PARAMS") or {}
        self._env_redraw = env_redraw.EnvRedraw(self._lib, self._handle, self._vcfg, spec, self.reset_buf, self.env_params,
                                                self.env_inertia, self.device)
        self._attach_env_redraw()
        self.logger.info(f"ENV_PARAMS_PER_EPISODE: the plants of {len(self._env_redraw.spec)} names are redrawn on the device "
                         f"whenever an env's episode ends")

    def _attach_env_redraw(self):
        self._env_params_host = self._env_inertia_host = None        # no host mirror: the device redraws
        for o in self._observers:
            if hasattr(o, "redraw"):
                o.redraw = self._env_redraw
            if hasattr(o, "env_episode_of"):
                o.env_episode_of = lambda envs: self._env_redraw.episodes_now()[list(envs)]
        self._add_observer(self._env_redraw)

    @property
    def env_redraw(self):
        """The ``EnvRedraw`` of this env (``None`` unless ``ENV_PARAMS_PER_EPISODE``; under ``ENV_PARAMS_ADR`` its ``EnvAdr``)."""
        return self._env_redraw

    # ------------------------------------------------------------------ ENV_PARAMS_ADR (include/vine_env_adr.h)
    def _setup_env_adr(self):
        """The redraw's place is taken by two launches behind every step that also move the ranges of the names under
        ``ENV_PARAMS_ADR.NAMES``: they begin at START (the tables bound in ``create_sim`` are START's), the ``[lo, hi]`` of
        ``ENV_PARAMS`` are their limits.  The launches read the step's reward matrix, so one is bound here (arming
        introspection) before anything is captured; one bound already is shared."""
        from ..utils import env_adr
        if self._reward_matrix is None:
            self.bind_reward_matrix()
        spec = self.cfg["env"].get("ENV_PARAMS") or {}
        self._env_redraw = env_adr.EnvAdr(self._lib, self._handle, self._vcfg, spec, self._adr, self.reset_buf, self.env_params,
                                          self.env_inertia, self.device, self.logger)
        self._attach_env_redraw()
        self.logger.info(f"ENV_PARAMS_ADR: the ranges of {', '.join(self._adr['NAMES'])} start at START and move on the device "
                         f"by the reach rate of the episodes probing their boundaries")

    @property
    def env_adr(self):
        """The ``EnvAdr`` of this env (``None`` unless ``ENV_PARAMS_ADR``)."""
        return self._env_redraw if self._adr is not None else None

    # ------------------------------------------------------------------ MAT_FILE replay (V5:281-297, 947-982)
    def read_mat_file(self, filename):
        """Recorded trajectory: cart_pos (1,T), Q (5,T), moving_target_pos (3,T), target_vel, tip_pos (3,T),
        tip_vel (3,T) -> one [T, 12] device table (q(6), target y/z, tip y/z, tip vy/vz)."""
        import numpy as np
        import scipy.io
        mat = scipy.io.loadmat(filename)
        cart, Q = np.asarray(mat["cart_pos"], np.float64), np.asarray(mat["Q"], np.float64)
        T = cart.shape[1]
        assert cart.shape == (1, T) and Q.shape == (N_REVOLUTE_DOFS, T)
        if np.any(np.asarray(mat["target_vel"], np.float64) != 0.0):
            raise NotImplementedError("MAT_FILE with a moving target: target velocities are identically zero in the "
                                      "step kernel (V5:916-918)")
        rows = np.concatenate([cart, Q, np.asarray(mat["moving_target_pos"], np.float64)[1:3],
                               np.asarray(mat["tip_pos"], np.float64)[1:3],
                               np.asarray(mat["tip_vel"], np.float64)[1:3]], 0).T
        self._mat_table = torch.as_tensor(rows, dtype=torch.float32, device=self.device).contiguous()
        return mat

    def overwrite_with_mat(self):
        """V5:947-982: every env is put on sample ``num_steps % T`` of the recording before the step."""
        T = self._mat_table.shape[0]
        index = self.num_steps % T
        self.logger.info(f"Currently at {index} / {T}")
        row = self._mat_table[index]
        st, f = self._state, abi
        st[f.VF_Q0:f.VF_Q0 + 6] = row[0:6].unsqueeze(-1)
        st[f.VF_QD0:f.VF_QD0 + 6] = 0.0
        st[f.VF_TARGET_Y], st[f.VF_TARGET_Z] = row[6], row[7]
        st[f.VF_TIP_Y], st[f.VF_TIP_Z], st[f.VF_TIP_VY], st[f.VF_TIP_VZ] = row[8], row[9], row[10], row[11]

    # ------------------------------------------------------------------ native handle
    def create_sim(self):
        """Replaces create_sim/_create_envs/prepare_sim (V5:364-556): one ``vine_create``."""
        self._lib = native.load()
        seed = self.cfg.get("seed", None)
        self._vcfg = vine_config_from_cfg(self.cfg, self._lib, seed=seed)
        if not torch.cuda.is_available():
            raise RuntimeError("no MI355X visible to PyTorch-ROCm; vine_robot_isaacgymenvs_amd has no CPU path")
        # torch owns the SoA state block so that the reference's state views are zero-copy tensors
        self._state = torch.zeros((abi.VF_COUNT, self.num_envs), device=self.device, dtype=torch.float32)
        h = C.c_void_p()
        native.check(self._lib.vine_create(C.byref(self._vcfg), self.device_id, self._state.data_ptr(), C.byref(h)),
                     self._lib)
        self._handle = h
        self.env_params = None                   # ENV_PARAMS: the bound device table [VP_COUNT, N], else None
        self.env_param_names = abi.ENV_PARAM_ROW_NAMES
        self._env_params_host = None             # its host mirror (numpy), what the checks run on
        self.env_inertia = None                  # ENV_INERTIA: the bound device table [VI_COUNT, N] of masses, else None
        self.env_inertia_names = abi.ENV_INERTIA_ROW_NAMES
        self._env_inertia_host = None
        self._env_inertia_draws = {}             # LINK_MASS / TIP_LINK_MASS: the per-env factors the link rows were formed from
        spec = self.cfg["env"].get("ENV_PARAMS") or {}
        if len(spec):
            if getattr(self, "_adr", None) is not None:      # ENV_PARAMS_ADR: episode 0 is drawn from START
                from ..utils import env_params
                spec = env_params.adr_start_spec(spec, self._adr)
            self._setup_env_params(spec)
            self._setup_env_inertia(spec)

    # ------------------------------------------------------------------ ENV_PARAMS (include/vine_env_params.h)
    def _setup_env_params(self, spec):
        """The per-env parameter table of the spec (utils/env_params.py), checked on the host, uploaded and bound: from
        here on every env steps with its own column, on the one-lane-per-env kernel."""
        from ..utils import env_params
        before = self.step_kernel_name
        table = env_params.build_table(spec, self._vcfg, int(self._vcfg.seed), self.num_envs, int(self._vcfg.env_id_offset),
                                       lib=self._lib)
        self._env_params_host = table
        self.env_params = torch.as_tensor(table, device=self.device).contiguous()
        torch.cuda.synchronize(self.device)
        native.check(self._lib.vine_bind_env_params(self._handle, self.env_params.data_ptr()), self._lib)
        varying = [self.env_param_names[p] for p in env_params.varying_rows(table)]
        self.logger.info(f"ENV_PARAMS: {len(varying)} of {abi.VP_COUNT} table rows vary across the {self.num_envs} envs "
                         f"({', '.join(varying) or 'none'}); step kernel {before} -> {self.step_kernel_name}")

    def _setup_env_inertia(self, spec):
        """The per-env inertia table of the spec's CART_MASS / LINK_MASS / TIP_LINK_MASS (utils/env_params.py), derived and
        checked through the library, uploaded and bound beside the parameter table (which a spec of masses alone leaves at
        the configuration's row in every column).  Nothing happens for a spec without the three names."""
        from ..utils import env_params
        draws = {}
        table = env_params.draw_inertia_table(
            spec, env_params.inertia_config_row(self._lib, self._vcfg), int(self._vcfg.seed), self.num_envs,
            lambda t: env_params.derive_inertia(self._lib, self._vcfg, t), int(self._vcfg.env_id_offset),
            check=lambda t: env_params.check_inertia_table(self._lib, self._vcfg, t), draws=draws)
        if table is None:
            return
        self._bind_env_inertia(table, draws)
        varying = [self.env_inertia_names[r] for r in env_params.varying_rows(table[:abi.VI_PRIMARY_COUNT])]
        self.logger.info(f"ENV_PARAMS: {len(varying)} of {abi.VI_PRIMARY_COUNT} masses and inertias vary across the "
                         f"{self.num_envs} envs ({', '.join(varying) or 'none'})")

    def _bind_env_inertia(self, table, draws):
        self._env_inertia_host = table
        self._env_inertia_draws = {k: draws[k] for k in ("LINK_MASS", "TIP_LINK_MASS") if k in draws}
        self.env_inertia = torch.as_tensor(table, device=self.device).contiguous()
        torch.cuda.synchronize(self.device)
        native.check(self._lib.vine_bind_env_inertia(self._handle, self.env_inertia.data_ptr()), self._lib)

    def _set_env_inertia(self, values):
        """The inertia-table half of ``set_env_params``: the new primary rows, re-derived and checked on the host, then
        every changed row rewritten in place on the device.  A table is built and bound on first use."""
        import numpy as np
        from ..utils import env_params
        base = env_params.inertia_config_row(self._lib, self._vcfg)
        table = (self._env_inertia_host.copy() if self._env_inertia_host is not None
                 else np.repeat(base[:, None], self.num_envs, axis=1))
        draws = dict(self._env_inertia_draws)
        full = lambda v: np.broadcast_to(v, (self.num_envs,)).astype(np.float64)      # noqa: E731
        factors = {k: full(v) for k, v in values.items() if k in ("LINK_MASS", "TIP_LINK_MASS")}
        if factors:                              # the link rows anew from the configuration's and the two factors
            draws.update(factors)
            cart = table[abi.VI_CART_MASS].copy()
            env_params.set_inertia_rows(table, base, draws)
            table[abi.VI_CART_MASS] = cart
        for name, v in values.items():           # then the rows stated themselves
            if name == "CART_MASS":
                table[abi.VI_CART_MASS] = full(v).astype(np.float32)
            elif name not in factors:
                table[self.env_inertia_names.index(name)] = full(v).astype(np.float32)
        table = env_params.derive_inertia(self._lib, self._vcfg, table)
        env_params.check_inertia_table(self._lib, self._vcfg, table)
        if self.env_inertia is None:
            self._bind_env_inertia(table, draws)
            return
        for r in range(abi.VI_COUNT):
            if not np.array_equal(table[r].view(np.uint32), self._env_inertia_host[r].view(np.uint32)):
                self.env_inertia[r].copy_(torch.from_numpy(table[r]))
        self._env_inertia_host, self._env_inertia_draws = table, draws

    def set_env_params(self, values):
        """Rewrite rows of the bound table in place: ``values`` maps a name to a scalar or an array [N].  Names are
        ``abi.ENV_PARAM_NAMES`` -- an FPAM vector's value is a factor on the configuration's five constants, as in the
        ``ENV_PARAMS`` spec -- or a single row of ``env_param_names`` (``"FPAM_K[2]"``: the constant itself).  The new table
        is checked on the host first; a captured hipGraph reads the new contents at its next replay.  Not inside a graph
        capture.

        The names of the inertia table go the same way (include/vine_env_inertia.h): ``CART_MASS`` in kg, ``LINK_MASS`` and
        ``TIP_LINK_MASS`` as factors on the configuration's link masses and inertias (either one re-forms all ten link
        rows from the configuration's and the two factors in force), or a primary row of ``env_inertia_names``
        (``"LINK_MASS[2]"``, ``"LINK_INERTIA[4]"``: the value itself).  The derived rows are formed anew on the host.  The
        first such call binds an inertia table if none is bound yet: call it before a step is captured."""
        import numpy as np
        from ..utils import env_params
        if self.env_params is None:
            raise RuntimeError("set_env_params(): no per-env parameter table is bound (task.env.ENV_PARAMS is empty)")
        if self._env_redraw is not None:
            raise RuntimeError("set_env_params(): task.env.ENV_PARAMS_PER_EPISODE is on, the spec owns the tables: the device "
                               "redraws an env's column at its next reset and would overwrite what is set here")
        primary = self.env_inertia_names[:abi.VI_PRIMARY_COUNT]
        inertia = {}
        for name in [k for k in values if k in abi.ENV_INERTIA_NAMES or k in primary]:
            v = values[name]
            v = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
            if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != self.num_envs):
                raise ValueError(f"set_env_params: {name} takes a scalar or an array [{self.num_envs}], not {v.shape}")
            inertia[name] = v
        values = {k: v for k, v in values.items() if k not in inertia}
        table = self._env_params_host.copy()
        base = env_params.config_row(self._lib, self._vcfg)
        rows = []
        for name, v in values.items():
            v = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
            if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != self.num_envs):
                raise ValueError(f"set_env_params: {name} takes a scalar or an array [{self.num_envs}], not {v.shape}")
            if name in abi.ENV_PARAM_ROWS:
                first, count = abi.ENV_PARAM_ROWS[name]
                for p in range(first, first + count):
                    table[p] = (v if count == 1 else base[p].astype(np.float64) * v).astype(np.float32)
                    rows.append(p)
            elif name in self.env_param_names:
                p = self.env_param_names.index(name)
                table[p] = v.astype(np.float32)
                rows.append(p)
            else:
                raise ValueError(f"set_env_params: unknown parameter {name!r}")
        env_params.check_table(self._lib, self._vcfg, table)
        if inertia:                              # (checked before anything is written: a refusal leaves both tables as they were)
            self._set_env_inertia(inertia)
        for p in rows:
            self.env_params[p].copy_(torch.from_numpy(table[p]))
        self._env_params_host = table

    def env_params_of(self, envs):
        """The host mirror's columns of ``envs`` as float64 [VP_COUNT, len(envs)] (``None`` without a bound table)."""
        import numpy as np
        if self._env_redraw is not None:         # ENV_PARAMS_PER_EPISODE: the device's table, as of now (synchronises)
            return self.env_params[:, list(envs)].cpu().numpy().astype(np.float64)
        if self._env_params_host is None:
            return None
        return self._env_params_host[:, list(envs)].astype(np.float64)

    def env_inertia_of(self, envs):
        """The inertia table's host mirror, columns ``envs``, as float64 [VI_COUNT, len(envs)] (``None`` without one)."""
        import numpy as np
        if self._env_redraw is not None and self.env_inertia is not None:
            return self.env_inertia[:, list(envs)].cpu().numpy().astype(np.float64)
        if self._env_inertia_host is None:
            return None
        return self._env_inertia_host[:, list(envs)].astype(np.float64)

    def close(self):
        if self._observers:
            torch.cuda.synchronize(self.device)
            for o in self._observers:
                o.drain()
                o.close()
            self._observers, self._video, self._trajectory, self._episode_log, self._env_redraw = [], None, None, None, None
            self._env_sensor = self._env_push = self._env_target = self._env_draw_adr = None
        if self._handle is not None and self._lib is not None:
            torch.cuda.synchronize(self.device)
            self._lib.vine_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _launch_step(self, fn, first_arg, actions_ptr, obs_out):
        """One step launch (``vine_step``, ``vine_step_rollout`` or ``vine_step_eval``: ``first_arg`` is the action buffer
        or the address of the argument block) with the observers around it."""
        for o in self._observers:
            o.before(1)
        native.check(fn(self._handle, first_arg, obs_out.data_ptr(), self.rew_buf.data_ptr(), self.reset_buf.data_ptr(),
                        self.progress_buf.data_ptr(), self.timeout_buf.data_ptr(), self._stream()), self._lib)
        self._observe(actions_ptr, obs_out)
        self.num_steps += 1

    def _rebind(self, obs_out):
        """The buffers re-bound exactly as ``step_into`` does."""
        self.obs_buf = obs_out
        self.obs_dict["obs"] = obs_out.to(self.rl_device)
        self.extras["time_outs"] = self.timeout_buf.to(self.rl_device)
        return obs_out

    def _native_step(self, actions, obs_out):
        if self.mat is not None:
            self.overwrite_with_mat()
        self._launch_step(self._lib.vine_step, actions.data_ptr(), actions.data_ptr(), obs_out)

    def rollout_step_blocks(self):
        """Rows of the per-workgroup episode sums ``step_rollout_into`` writes (0: this configuration does not run the
        four-lanes-per-env kernel, the fused rollout step is not available)."""
        return 0 if self.mat is not None else int(self._lib.vine_step_rollout_blocks(self._handle))

    def step_rollout_into(self, args, obs_out):
        """One ROLLOUT step in one launch (``vine_step_rollout``, include/vine_ppo.h): the policy head on the LSTM output
        rows in front of the step, the rollout bookkeeping behind it -- an extension for the PPO loop (the trainer's
        ``_rollout_body_fused``); ``VecTask.step`` / ``step_into`` are untouched.  ``args``: abi.RolloutArgs; the
        observation goes to ``obs_out`` and the buffers are re-bound exactly as ``step_into`` does."""
        self._launch_step(self._lib.vine_step_rollout, C.addressof(args), args.action_out, obs_out)
        return self._rebind(obs_out)

    def eval_step_rows(self):
        """Rows of the per-workgroup float64 totals ``step_eval_into`` adds to (0: this configuration does not run the
        four-lanes-per-env kernel, the evaluation step is not available)."""
        return 0 if self.mat is not None else int(self._lib.vine_step_eval_rows(self._handle))

    def step_eval_into(self, args, obs_out):
        """One EVALUATION step in one launch (``vine_step_eval``, include/vine_ppo.h): the policy head's mean on the LSTM
        output rows in front of the step, per-episode task statistics behind it -- an extension for the player's device
        path; ``VecTask.step`` / ``step_into`` are untouched.  ``args``: abi.EvalArgs; the observation goes to ``obs_out``
        and the buffers are re-bound exactly as ``step_into`` does."""
        self._launch_step(self._lib.vine_step_eval, C.addressof(args), args.action_out, obs_out)
        return self._rebind(obs_out)

    def reset_idx(self, env_ids):
        """V5:774-839 for callers outside the step (reset_done, V5:715-718)."""
        ids = torch.as_tensor(env_ids, device=self.device).to(torch.long).contiguous()
        if ids.numel() == 0:
            return
        native.check(self._lib.vine_reset_idx(self._handle, ids.data_ptr(), ids.numel(), self.rew_buf.data_ptr(),
                                              self.reset_buf.data_ptr(), self.progress_buf.data_ptr(), self._stream()),
                     self._lib)
        if self._episode_log is not None:        # EPISODE_LOG: their running episode is discarded without a row
            self._episode_log.reset_envs(ids)
        if self.env_adr is not None:             # ENV_PARAMS_ADR: ... and is not counted at its boundary
            self.env_adr.reset_envs(ids)
        if self._env_sensor is not None:         # ENV_SENSOR: their next frame is an episode's first
            self._env_sensor.reset_envs(ids)
        if self._env_target is not None:         # ENV_TARGET: ... and their target starts from where this reset put it
            self._env_target.reset_envs(ids)
        if self._env_draw_adr is not None:       # ENV_DRAW_ADR: ... and is not counted at a boundary of the draws' ranges
            self._env_draw_adr.reset_envs(ids)

    # ------------------------------------------------------------------ metrics side channel (V5:1250-1322)
    def collect_stats(self):
        """The ~120 scalars the reference puts into ``wandb_dict`` EVERY step with one ``.item()`` sync each
        (V5:1250-1322): here ONE two-stage reduction on the device (``vine_stats``, include/vine.h) and ONE
        device->host copy, on demand.  Same key names, so dashboards carry over.  The fields the step only stores on
        request (VINE_FLAG_INTROSPECT) must have been armed before the step being summarised:
        ``bind_reward_matrix()`` (also needed for the per-term entries) or ``set_introspection(True)``."""
        if not self._introspection:
            raise RuntimeError("collect_stats(): call bind_reward_matrix() or set_introspection(True) before the step "
                               "whose state is to be summarised (the step stores the dashboard-only fields on request)")
        f = abi
        if self._stats_out is None:
            self._stats_out = torch.zeros(f.NUM_STATS, device=self.device, dtype=torch.float32)
        native.check(self._lib.vine_stats(self._handle, self.rew_buf.data_ptr(), self.progress_buf.data_ptr(),
                                          int(self.index_to_view), self._stats_out.data_ptr(), self._stream()), self._lib)
        v = self._stats_out.cpu().tolist()           # the only synchronisation
        d = {}
        for name, k in (("dist_tip_to_target", f.VS_DIST_MEAN), ("target_reached", f.VS_TARGET_REACHED),
                        ("limit_hit", f.VS_LIMIT_HIT), ("tip_limit_hit", f.VS_TIP_LIMIT_HIT), ("abs_tip_y", f.VS_ABS_TIP_Y),
                        ("tip_z", f.VS_TIP_Z), ("max_abs_tip_y", f.VS_MAX_ABS_TIP_Y), ("max_tip_z", f.VS_MAX_TIP_Z),
                        ("tip_velocities", f.VS_TIP_VEL_MEAN), ("tip_velocities_max", f.VS_TIP_VEL_MAX),
                        ("u_rail_velocity", f.VS_U_RAIL_ABS), ("prev_u_rail_velocity", f.VS_PREV_U_RAIL_ABS),
                        ("rail_force", f.VS_RAIL_FORCE_ABS), ("u_fpam", f.VS_U_FPAM_ABS),
                        ("smoothed_u_fpam", f.VS_SMOOTHED_ABS),
                        ("tip_target_velocity_difference", f.VS_TIP_VEL_MEAN),      # target velocities are zero (V5:916-918)
                        ("progress_buf", f.VS_PROGRESS_MEAN), ("contact_forces", f.VS_CONTACT_MEAN),
                        ("nonzero_contact_force", f.VS_CONTACT_NONZERO), ("Aggregated Reward", f.VS_AGG_MEAN)):
            d[name] = v[k]
        d["Aggregated Reward 1 Std Up"] = v[f.VS_AGG_MEAN] + v[f.VS_AGG_STD]
        d["Aggregated Reward 1 Std Down"] = v[f.VS_AGG_MEAN] - v[f.VS_AGG_STD]
        w0 = f.VS_VIEW0
        q, qd, pq = v[w0:w0 + 6], v[w0 + 6:w0 + 12], v[w0 + 12:w0 + 18]
        tip_y, tip_z, tip_vy, tip_vz, ptip_y, ptip_z, cart_y, cart_vy, tgt_y, tgt_z = v[w0 + 18:w0 + 28]
        u_fpam, smoothed, u_rail, rail_force, contact = v[f.VS_VIEW_U:f.VS_VIEW_U + 5]
        fd = [(a - b) / self.control_dt for a, b in zip(q, pq)]
        d["prismatic_q0 at self.index_to_view"] = q[0]
        d["prismatic_qd0 at self.index_to_view"] = qd[0]
        d["prismatic_finite_diff_qd0 at self.index_to_view"] = fd[0]
        for j in range(N_REVOLUTE_DOFS):
            d[f"q{j} at self.index_to_view"] = q[1 + j]
            d[f"qd{j} at self.index_to_view"] = qd[1 + j]
            d[f"finite_diff_qd{j} at self.index_to_view"] = fd[1 + j]
        per_dir = {"x": (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                   "y": (tip_vy, cart_vy, 0.0, (tip_y - ptip_y) / self.control_dt, tip_y, cart_y, tgt_y),
                   "z": (tip_vz, 0.0, 0.0, (tip_z - ptip_z) / self.control_dt, tip_z, CART_Z, tgt_z)}
        for dr, (tv, cv, gv, ftv, tp, cp, gp) in per_dir.items():
            d[f"tip_vel_{dr} at self.index_to_view"] = tv
            d[f"cart_vel_{dr} at self.index_to_view"] = cv
            d[f"target_vel_{dr} at self.index_to_view"] = gv
            d[f"finite_diff_tip_vel_{dr} at self.index_to_view"] = ftv
            d[f"tip_pos_{dr} at self.index_to_view"] = tp
            d[f"cart_pos_{dr} at self.index_to_view"] = cp
            d[f"target_pos_{dr} at self.index_to_view"] = gp
        d["u_fpam at self.index_to_view"] = u_fpam
        d["smoothed u_fpam at self.index_to_view"] = smoothed
        d["u_rail_velocity at self.index_to_view"] = u_rail
        d["rail_force at self.index_to_view"] = rail_force
        d["contact_force at self.index_to_view"] = contact
        d["nonzero_contact_force at self.index_to_view"] = float(contact > 0)
        if self._reward_matrix is not None:
            for k, name in enumerate(REWARD_NAMES):
                mean, mx, mn = v[f.VS_TERM0 + 3 * k:f.VS_TERM0 + 3 * k + 3]
                w = float(self.cfg["env"][_REWARD_KEYS[k] + "_REWARD_WEIGHT"])
                d[f"Mean {name} Reward"] = mean
                d[f"Max {name} Reward"] = mx
                d[f"Weighted Mean {name} Reward"] = w * mean
                d[f"Weighted Max {name} Reward"] = w * mx if w >= 0 else w * mn
        d["Mean Total Reward"] = v[f.VS_REW_MEAN]
        d["Max Total Reward"] = v[f.VS_REW_MAX]
        self.wandb_dict = d
        return d

    @property
    def step_kernel_name(self):
        """Device kernel ``vine_step`` launches for this configuration (one lane per env, or four lanes per env)."""
        return self._lib.vine_step_kernel_name(self._handle).decode()

    def set_introspection(self, on=True):
        """Arm / disarm the stores of the fields nothing in the step reads back (``prev_dof_pos``, ``prev_tip_positions``,
        ``tip_velocities``, ``u_fpam``, ``u_rail_velocity``, ``prev_u_rail_velocity``, ``rail_force``, the mean contact
        force): the reference exposes them as attributes and dashboard inputs; they are ~70 B of the step's HBM traffic
        per env, so the step only stores them on request.  Takes effect with the next step launched outside a captured
        hipGraph (a captured rollout keeps the setting it was captured with)."""
        native.check(self._lib.vine_set_introspection(self._handle, int(bool(on))), self._lib)
        self._introspection = bool(on)

    def observation_names(self):
        """Column names of the default observation layout (V5:1430-1437); generic names for the other layouts."""
        xyz = ("x", "y", "z")
        names = ([f"joint_pos_{i}" for i in range(self.num_dof)] + [f"joint_vel_{i}" for i in range(self.num_dof)]
                 + [f"tip_pos_{i}" for i in xyz] + [f"tip_vel_{i}" for i in xyz] + [f"target_pos_{i}" for i in xyz]
                 + [f"target_vel_{i}" for i in xyz] + ["smoothed_u_fpam", "prev_u_rail_vel", "target_depth", "target_angle"])
        return names if len(names) == self.num_obs else [f"obs_{i}" for i in range(self.num_obs)]

    def write_histograms(self, rows, directory, bins=20):
        """CREATE_HISTOGRAMS_PERIODICALLY (V5:1392-1452) without wandb: one ``.npz`` per histogram set holding the raw
        rows, and per observation column the counts and bin edges a ``wandb.plot.histogram`` would draw."""
        import numpy as np
        os.makedirs(directory, exist_ok=True)
        data = np.asarray(rows, dtype=np.float32)
        out = {"rows": data, "names": np.array(self.observation_names())}
        for j, name in enumerate(self.observation_names()):
            counts, edges = np.histogram(data[:, j], bins=bins)
            out[name + "_counts"], out[name + "_edges"] = counts, edges
        path = os.path.join(directory, f"observation_histograms_{self.num_steps}.npz")
        np.savez_compressed(path, **out)
        self.logger.info(f"Creating histogram at self.num_steps {self.num_steps}: {path}")
        return path

    # ------------------------------------------------------------------ test / tooling hooks
    def bind_reward_matrix(self):
        """Ask the kernel to also write the [N,13] unweighted reward matrix (V5:1272) each step."""
        if self._episode_log is not None or self.env_adr is not None or self._env_draw_adr is not None:
            return self._reward_matrix      # EPISODE_LOG, ENV_PARAMS_ADR and ENV_DRAW_ADR read the matrix bound at set-up: that one is shared
        self._reward_matrix = torch.zeros((self.num_envs, abi.NUM_REWARDS), device=self.device)
        native.check(self._lib.vine_bind_reward_matrix(self._handle, self._reward_matrix.data_ptr()), self._lib)
        self._introspection = True           # the library arms VINE_FLAG_INTROSPECT together with the matrix
        return self._reward_matrix

    def bind_reset_values(self, values):
        """Deterministic reset draws ([N,10], see include/vine.h); ``None`` restores the counter RNG."""
        if values is None:
            self._reset_values = None
            native.check(self._lib.vine_bind_reset_values(self._handle, None), self._lib)
        else:
            self._reset_values = torch.as_tensor(values, dtype=torch.float32, device=self.device).contiguous()
            assert self._reset_values.shape == (self.num_envs, 10)
            native.check(self._lib.vine_bind_reset_values(self._handle, self._reset_values.data_ptr()), self._lib)

    @property
    def step_count(self):
        return self._lib.vine_get_step_count(self._handle)

    @step_count.setter
    def step_count(self, v):
        native.check(self._lib.vine_set_step_count(self._handle, int(v)), self._lib)
        for o in self._observers:
            o.set_steps(int(v))

    @property
    def state(self):
        """The [VF_COUNT, N] SoA block (fields: include/vine.h VineField)."""
        return self._state

    # ------------------------------------------------------------------ reference attribute names (views)
    def _col(self, f):
        return self._state[f].unsqueeze(-1)

    def _xyz(self, fy, fz, x=0.0):
        return torch.stack([torch.full_like(self._state[fy], x), self._state[fy], self._state[fz]], dim=-1)

    @property
    def dof_pos(self):            # V5:303
        return self._state[abi.VF_Q0:abi.VF_Q0 + 6].t()

    @property
    def dof_vel(self):            # V5:304
        return self._state[abi.VF_QD0:abi.VF_QD0 + 6].t()

    @property
    def prev_dof_pos(self):       # V5:231
        return self._state[abi.VF_PREV_Q0:abi.VF_PREV_Q0 + 6].t()

    @property
    def tip_positions(self):      # V5:357
        return self._xyz(abi.VF_TIP_Y, abi.VF_TIP_Z)

    @property
    def tip_velocities(self):     # V5:361
        return self._xyz(abi.VF_TIP_VY, abi.VF_TIP_VZ)

    @property
    def prev_tip_positions(self):  # V5:232
        return self._xyz(abi.VF_PREV_TIP_Y, abi.VF_PREV_TIP_Z)

    @property
    def cart_positions(self):     # V5:358
        z = torch.full_like(self._state[abi.VF_CART_Y], CART_Z)
        return torch.stack([torch.zeros_like(z), self._state[abi.VF_CART_Y], z], dim=-1)

    @property
    def cart_velocities(self):    # V5:362
        z = torch.zeros_like(self._state[abi.VF_CART_VY])
        return torch.stack([z, self._state[abi.VF_CART_VY], z], dim=-1)

    @property
    def target_positions(self):   # V5:179
        return self._xyz(abi.VF_TARGET_Y, abi.VF_TARGET_Z)

    @property
    def target_velocities(self):  # V5:180 (always zero, V5:916-918)
        return torch.zeros(self.num_envs, NUM_XYZ, device=self.device)

    @property
    def smoothed_u_fpam(self):    # V5:224
        return self._col(abi.VF_SMOOTHED_U)

    @property
    def u_fpam(self):             # V5:937
        return self._col(abi.VF_U_FPAM)

    @property
    def u_rail_velocity(self):    # V5:937
        return self._col(abi.VF_U_RAIL)

    @property
    def prev_u_rail_velocity(self):  # V5:233
        return self._col(abi.VF_PREV_U_RAIL)

    @property
    def prev_cart_vel(self):      # V5:235
        return self._col(abi.VF_PREV_CART_VEL)

    @property
    def prev_cart_vel_error(self):  # V5:234
        return self._col(abi.VF_PREV_CART_VEL_ERR)

    @property
    def rail_force(self):         # V5:1094
        return self._col(abi.VF_RAIL_FORCE)

    @property
    def object_info(self):        # V5:238
        return self._state[abi.VF_OBJ_DEPTH:abi.VF_OBJ_DEPTH + 2].t()

    @property
    def aggregated_rew_buf(self):  # V5:183
        return self._state[abi.VF_AGG_REW]
