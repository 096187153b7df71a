"""Packaged default configuration of the Vine5LinkMovingBase path, as Python literals.

Same key names, nesting and interpolation grammar as the Hydra config directory of the reference
(``isaacgymenvs/cfg/config.yaml``, ``cfg/task/Vine5LinkMovingBase.yaml``, ``cfg/train/Vine5LinkMovingBasePPO.yaml``):
values written as ``${...}`` are resolved by ``utils/config.py`` exactly like OmegaConf would.  A user who prefers
editable YAML files can write them with ``python -m vine_robot_isaacgymenvs_amd.utils.config --dump-yaml DIR`` and
pass ``config_dir=DIR`` (the reference's own cfg directory loads through the same code path).

The pipe obstacle (CREATE_PIPE, the reference's default) is simulated as the planar cross-section of its mesh.

Deviations from the reference's defaults (each documented in DESIGN.md / INTEGRATION.md):
  task.env.CAPTURE_VIDEO False (the reference: True; set it to draw and save rollout videos);
    task.env.CAPTURE_VIDEO_EVERY / _FRAMES / _VIEWS / _WIDTH / _HEIGHT: the reference's camera constants (V5:213-219) as keys,
  task.env.RECORD_TRAJECTORIES False (not a reference key; set it to log chosen envs on the device and save them as MAT
    files in the layout MAT_FILE reads); task.env.RECORD_TRAJECTORIES_EVERY / _STEPS (0: maxEpisodeLength,
    at most _EVERY) / _ENVS (a count from index_to_view on, or a list of env indices) / _DIR ('': runs/<name>),
  task.env.EPISODE_LOG False (not a reference key; set it to log one row per finished episode of every env on the device:
    reached or not, when, final and smallest distance, why it ended, target and obstacle);
    task.env.EPISODE_LOG_TABLE (False: totals only) / _CAPACITY (rows of the device ring) / _DIR ('': runs/<name>),
  task.env.ENV_PARAMS {} (not a reference key; name -> number, [lo, hi] or {values: [...]} gives every env its own joint
    damping, FPAM constants (as a factor), smoothing constants, rail gains and action delay, held for the whole run, on the
    one-lane-per-env step kernel; utils/env_params.py; CART_MASS (kg), LINK_MASS and TIP_LINK_MASS
    (factors on the link masses and inertias) likewise, through a second table: DESIGN.md section 19),
  task.env.ENV_PARAMS_PER_EPISODE False (not a reference key; set it to redraw an env's ENV_PARAMS plant on the device
    whenever its episode ends, instead of holding it for the whole run: DESIGN.md section 20),
  task.env.ENV_PARAMS_ADR {} (not a reference key; with ENV_PARAMS_PER_EPISODE, NAMES: {NAME: {START: [lo, hi], STEP: s}} makes
    the ranges of those names begin at START and widen on the device towards their ENV_PARAMS limits while the episodes pinned
    to a boundary still reach the target; BOUNDARY_FRACTION, QUEUE, WIDEN_AT, NARROW_AT: DESIGN.md section 21),
  task.env.ENV_SENSOR {} (not a reference key; DELAY, HOLD, NOISE_STD -- each a number, [lo, hi] or {values: [...]} -- give every
    env its own sensing latency in control steps, probability of a dropped frame and per-frame observation noise, applied on
    the device behind the step to COLUMNS (all, or a list of column indices); PER_EPISODE redraws them at every reset; the
    step kernels are untouched; utils/env_sensor.py),
  task.env.ENV_PUSH {} (not a reference key; RATE, IMPULSE -- each a number, [lo, hi] or {values: [...]} -- give every env its own
    probability per control step of being pushed and its own largest impulse component in N s; a push is an instantaneous
    impulse at one of POINTS (0 the cart, m the distal end of link m - 1, 5 the tip; default [5]), applied on the device
    behind the step to the six generalised velocities through the step's own mass matrix; PER_EPISODE redraws the two values
    at every reset; the step kernels are untouched; utils/env_push.py),
  task.env.ENV_TARGET {} (not a reference key; VEL_ALONG, VEL_ACROSS, SPAN_ALONG, SPAN_ACROSS -- each a number, [lo, hi] or
    {values: [...]} -- give every env a target that moves during the episode: at VEL m/s along +y / +z in free space, or along
    the depth axis of the shelf or the pipe, turning round SPAN m either side of where the reset put it; advanced on the device
    behind the step, which also puts the target's velocity into the observation; PER_EPISODE redraws the four values at every
    reset; the step kernels are untouched; utils/env_target.py),
  task.env.ENV_DRAW_ADR {} (not a reference key; NAMES: {DRAW NAME: {START: [lo, hi], STEP: s}} over the PER_EPISODE [lo, hi] draws
    of ENV_SENSOR, ENV_PUSH and ENV_TARGET (SENSOR_DELAY .. TARGET_SPAN_ACROSS) makes those ranges begin at START and widen on the
    device towards their limits as ENV_PARAMS_ADR's do; utils/env_draw_adr.py),
  train.params.config.mixed_precision_dtype (not an rl_games key): fp16 (the reference's autocast dtype) = the hand-written
    mixed-precision update with device-side loss scaling; train.params.config.rollout_precision: fp32 (the reference's),
  task.env.physicsModel.* (switches of the built-in articulation solver; not reference keys),
  train.params.config.use_graphs / use_fused_ops (execution switches of this build; not rl_games keys),
  defaults list: task = Vine5LinkMovingBase (reference: Ant, which this build does not contain).
"""

# Root config (CLI shims, devices, seeds).  '' means "keep the value of the task/train config" (resolve_default).
ROOT = {'defaults': ['_self_', {'task': 'Vine5LinkMovingBase'}, {'train': '${task}PPO'}],
 'task_name': '${task.name}',
 'experiment': '',
 'num_envs': '',
 'horizon_length': '',
 'minibatch_size': '',
 'control_frequency_inv': '',
 'vine_randomize': '',
 'CAPTURE_VIDEO': '',
 'RAIL_VELOCITY_SCALE': '',
 'RAIL_SOFT_LIMIT': '',
 'RAIL_P_GAIN': '',
 'OBSERVATION_TYPE': '',
 'RAIL_ACCELERATION': '',
 'max_iterations': '',
 'seed': 42,
 'torch_deterministic': False,
 'physics_engine': 'physx',
 'pipeline': 'gpu',
 'sim_device': 'cuda:0',
 'rl_device': 'cuda:0',
 'graphics_device_id': 0,
 'num_threads': 4,
 'solver_type': 1,
 'num_subscenes': 4,
 'test': False,
 'checkpoint': '',
 'multi_gpu': False,
 'wandb_activate': False,
 'wandb_group': '',
 'wandb_name': '${train.params.config.name}',
 'wandb_entity': '',
 'wandb_project': 'isaacgymenvs',
 'capture_video': False,
 'capture_video_freq': 1464,
 'capture_video_len': 100,
 'force_render': True,
 'enable_viewer_sync_at_start': True,
 'headless': False}

# Task configs by name: env.* (task parameters), sim.* (time step, substeps, gravity; the physx block is accepted
# for compatibility and ignored by the built-in solver), task.* (randomisation).
TASK = {
    "Vine5LinkMovingBase": {'name': 'Vine5LinkMovingBase',
 'physics_engine': '${..physics_engine}',
 'env': {'numEnvs': '${resolve_default:4096,${...num_envs}}',
         'envSpacing': 6.0,
         'clipObservations': 5.0,
         'clipActions': 1.0,
         'maxEpisodeLength': 500,
         'controlFrequencyInv': '${resolve_default:4,${...control_frequency_inv}}',
         'enableCameraSensors': False,
         'USE_MOVING_BASE': True,
         'USE_SMOOTHED_FPAM': True,
         'FORCE_U_FPAM': False,
         'FORCE_U_RAIL_VELOCITY': False,
         'SMOOTHING_ALPHA_INFLATE': 0.81,
         'SMOOTHING_ALPHA_DEFLATE': 0.86,
         'CAPTURE_VIDEO': '${resolve_default:False,${...CAPTURE_VIDEO}}',
         'CAPTURE_VIDEO_EVERY': 1000,
         'CAPTURE_VIDEO_FRAMES': 100,
         'CAPTURE_VIDEO_VIEWS': 1,
         'CAPTURE_VIDEO_WIDTH': 400,
         'CAPTURE_VIDEO_HEIGHT': 225,
         'RECORD_TRAJECTORIES': False,
         'RECORD_TRAJECTORIES_EVERY': 1000,
         'RECORD_TRAJECTORIES_STEPS': 0,
         'RECORD_TRAJECTORIES_ENVS': 1,
         'RECORD_TRAJECTORIES_DIR': '',
         'EPISODE_LOG': False,
         'EPISODE_LOG_TABLE': True,
         'EPISODE_LOG_CAPACITY': 1048576,
         'EPISODE_LOG_DIR': '',
         'ENV_PARAMS': {},
         'ENV_PARAMS_PER_EPISODE': False,
         'ENV_PARAMS_ADR': {},
         'ENV_SENSOR': {},
         'ENV_PUSH': {},
         'ENV_TARGET': {},
         'ENV_DRAW_ADR': {},
         'CREATE_SHELF': False,
         'CREATE_PIPE': True,
         'CREATE_HISTOGRAMS_PERIODICALLY': False,
         'MAT_FILE': '',
         'FPAM_MIN': -0.1,
         'FPAM_MAX': 3.0,
         'RAIL_VELOCITY_SCALE': '${resolve_default:1.0,${...RAIL_VELOCITY_SCALE}}',
         'DAMPING': 0.02,
         'STIFFNESS': 0.0,
         'RAIL_SOFT_LIMIT': '${resolve_default:0.3,${...RAIL_SOFT_LIMIT}}',
         'RAIL_P_GAIN': '${resolve_default:10.0,${...RAIL_P_GAIN}}',
         'RAIL_D_GAIN': 0.0,
         'RAIL_ACCELERATION': '${resolve_default:8.0,${...RAIL_ACCELERATION}}',
         'OBSERVATION_TYPE': '${resolve_default:POS_AND_FD_VEL_AND_OBJ_INFO,${...OBSERVATION_TYPE}}',
         'RANDOMIZE_DOF_INIT': True,
         'RANDOM_INIT_CART_MIN_Y': "${eval:'-0.1 * ${.RAIL_SOFT_LIMIT}'}",
         'RANDOM_INIT_CART_MAX_Y': '${.RAIL_SOFT_LIMIT}',
         'RANDOMIZE_TARGETS': True,
         'SUCCESS_DIST': 0.08,
         'MIN_TARGET_DEPTH_IN_OBSTACLE': -0.05,
         'MAX_TARGET_DEPTH_IN_OBSTACLE': 0.2,
         'MIN_TARGET_Y': -0.48,
         'MAX_TARGET_Y': -0.4,
         'MIN_TARGET_Z': 0.58,
         'MAX_TARGET_Z': 0.67,
         'POSITION_REWARD_WEIGHT': 0.0,
         'CONST_NEGATIVE_REWARD_WEIGHT': 0.0,
         'POSITION_SUCCESS_REWARD_WEIGHT': 1.0,
         'VELOCITY_SUCCESS_REWARD_WEIGHT': 0,
         'VELOCITY_REWARD_WEIGHT': 0.1,
         'U_RAIL_VELOCITY_CONTROL_REWARD_WEIGHT': 0.0,
         'U_FPAM_CONTROL_REWARD_WEIGHT': 0.0,
         'RAIL_VELOCITY_CHANGE_REWARD_WEIGHT': 0.0,
         'U_FPAM_CHANGE_REWARD_WEIGHT': 0.0,
         'RAIL_LIMIT_REWARD_WEIGHT': 1.0,
         'CART_Y_REWARD_WEIGHT': 0.0,
         'TIP_Y_REWARD_WEIGHT': 0.0,
         'CONTACT_FORCE_REWARD_WEIGHT': 0.1,
         'USE_TARGET_REACHED_RESET': True,
         'USE_TIP_LIMIT_HIT_RESET': False,
         'USE_NONZERO_CONTACT_FORCE_RESET': False,
         'SCALE_OBSERVATIONS': True,
         'ACTION_DELAY': 1,
         'physicsModel': {'implicitJointDamping': True,
                          'fpamDampingHeld': False,
                          'staleBodyStateAfterReset': True,
                          'linkAngularDamping': 0.0,
                          'effortLimit': 0.0}},
 'sim': {'dt': 0.00833,
         'substeps': 10,
         'up_axis': 'z',
         'use_gpu_pipeline': '${eq:${...pipeline},"gpu"}',
         'gravity': [0.0, 0.0, -9.81],
         'enable_viewer_sync_at_start': '${resolve_default:True,${...enable_viewer_sync_at_start}}',
         'physx': {'num_threads': '${....num_threads}',
                   'solver_type': '${....solver_type}',
                   'use_gpu': '${contains:"cuda",${....sim_device}}',
                   'num_position_iterations': 8,
                   'num_velocity_iterations': 4,
                   'contact_offset': 0.02,
                   'rest_offset': 0.001,
                   'bounce_threshold_velocity': 0.2,
                   'max_depenetration_velocity': 100.0,
                   'default_buffer_size_multiplier': 2.0,
                   'max_gpu_contact_pairs': 1048576,
                   'num_subscenes': '${....num_subscenes}',
                   'contact_collection': 0}},
 'task': {'vine_randomize': '${resolve_default:True,${...vine_randomize}}',
          'randomization_parameters': {'DYNAMICS_SCALING_MIN': 0.999,
                                       'DYNAMICS_SCALING_MAX': 1.001,
                                       'OBSERVATION_NOISE_STD': 0.0,
                                       'ACTION_NOISE_STD': 0.0}}},
}

# Train configs by name, rl_games schema (consumed by learning/a2c_continuous.py).
TRAIN = {
    "Vine5LinkMovingBasePPO": {'params': {'seed': '${...seed}',
            'algo': {'name': 'a2c_continuous'},
            'model': {'name': 'continuous_a2c_logstd'},
            'network': {'name': 'actor_critic',
                        'separate': False,
                        'space': {'continuous': {'mu_activation': 'None',
                                                 'sigma_activation': 'None',
                                                 'mu_init': {'name': 'default'},
                                                 'sigma_init': {'name': 'const_initializer', 'val': 0},
                                                 'fixed_sigma': True}},
                        'mlp': {'units': [256, 128, 64],
                                'activation': 'elu',
                                'd2rl': False,
                                'initializer': {'name': 'default'},
                                'regularizer': {'name': 'None'}},
                        'rnn': {'name': 'lstm',
                                'units': 256,
                                'layers': 1,
                                'before_mlp': False,
                                'concat_input': True,
                                'layer_norm': True}},
            'load_checkpoint': '${if:${...checkpoint},True,False}',
            'load_path': '${...checkpoint}',
            'config': {'name': '${resolve_default:Vine5LinkMovingBase,${....experiment}}',
                       'full_experiment_name': '${.name}',
                       'env_name': 'rlgpu',
                       'device': '${....rl_device}',
                       'multi_gpu': '${....multi_gpu}',
                       'ppo': True,
                       'mixed_precision': True,
                       # how `mixed_precision: True` is carried out here: 'fp16' (default) = the hand-written update
                       # with float16 GEMM operands, fp32 accumulation/state/loss/optimiser and torch.amp.GradScaler
                       # restated on the device (loss scale + overflow flag inside the loss / column-sum / Adam kernels);
                       # 'bf16' = the same kernels with bfloat16 operands when the library was built with
                       # -DVINE_LP_BF16 (no loss scaling needed), otherwise torch autocast(bf16) over the stock modules
                       'mixed_precision_dtype': 'fp16',
                       'rollout_precision': 'fp32',
                       'normalize_input': True,
                       'normalize_value': True,
                       'value_bootstrap': True,
                       'num_actors': '${....task.env.numEnvs}',
                       'reward_shaper': {'scale_value': 0.01},
                       'normalize_advantage': True,
                       'gamma': 0.99,
                       'tau': 0.95,
                       'learning_rate': 0.0003,
                       'lr_schedule': 'adaptive',
                       'schedule_type': 'legacy',
                       'kl_threshold': 0.008,
                       'score_to_win': 20000000000,
                       'max_epochs': '${resolve_default:500,${....max_iterations}}',
                       'save_best_after': 50,
                       'save_frequency': 50,
                       'grad_norm': 1.0,
                       'entropy_coef': 0.0,
                       'truncate_grads': False,
                       'e_clip': 0.2,
                       'horizon_length': '${resolve_default:16,${....horizon_length}}',
                       'minibatch_size': '${resolve_default:32768,${....minibatch_size}}',
                       'mini_epochs': 4,
                       'critic_coef': 2,
                       'clip_value': True,
                       'seq_len': 4,
                       'bounds_loss_coef': 0.0001,
                                                  # MI355X execution switches of this build (not rl_games keys):
                                                  # replay the 16-step rollout as one hipGraph / use the hand-written
                                                  # HIP kernels around the GEMMs
                                                  'use_graphs': True,
                                                  'use_fused_ops': True,
                                                  # epochs between dumps of the task's dashboard scalars (the
                                                  # reference's wandb_dict keys) into summaries/scalars.csv; 0 = off
                                                  'env_stats_every': 10}}},
}
