"""ctypes mirror of ``include/vine.h`` (declarations only; no library is loaded here).

Every name below restates one declaration of the header.  ``declare(lib)`` attaches
argument/return types to the C-ABI entry points of a loaded shared library and raises
``AttributeError`` if any symbol the header declares is missing.
"""
import ctypes as C

VINE_ABI_VERSION = 3
NUM_LINKS = 5
NUM_DOFS = 6
NUM_ACTIONS = 2
NUM_REWARDS = 13
MAX_OBS = 28
MAX_DELAY = 8

# VineStatus
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_DEVICE, ERR_NO_DEVICE, ERR_ALLOC = 0, -1, -2, -3, -4, -5

# VineObsType (reference ObservationType enum, tasks/Vine5LinkMovingBase.py:67-73)
OBS_POS_AND_FD_VEL_AND_OBJ_INFO = 0
OBS_TIP_AND_CART_AND_OBJ_INFO = 1
OBS_POS_ONLY, OBS_POS_AND_VEL, OBS_POS_AND_FD_VEL, OBS_POS_AND_PREV_POS = 2, 3, 4, 5
OBS_TYPE_BY_NAME = {
    "POS_AND_FD_VEL_AND_OBJ_INFO": OBS_POS_AND_FD_VEL_AND_OBJ_INFO,
    "TIP_AND_CART_AND_OBJ_INFO": OBS_TIP_AND_CART_AND_OBJ_INFO,
    "POS_ONLY": OBS_POS_ONLY,
    "POS_AND_VEL": OBS_POS_AND_VEL,
    "POS_AND_FD_VEL": OBS_POS_AND_FD_VEL,
    "POS_AND_PREV_POS": OBS_POS_AND_PREV_POS,
}
SCALABLE_OBS_TYPES = (OBS_POS_AND_FD_VEL_AND_OBJ_INFO, OBS_TIP_AND_CART_AND_OBJ_INFO)

# VINE_FLAG_*
FLAG_USE_SMOOTHED_FPAM = 1 << 0
FLAG_FORCE_U_FPAM = 1 << 1
FLAG_FORCE_U_RAIL_VELOCITY = 1 << 2
FLAG_CREATE_SHELF = 1 << 3
FLAG_RANDOMIZE_DOF_INIT = 1 << 4
FLAG_RANDOMIZE_TARGETS = 1 << 5
FLAG_USE_TARGET_REACHED_RESET = 1 << 6
FLAG_USE_TIP_LIMIT_HIT_RESET = 1 << 7
FLAG_USE_NONZERO_CONTACT_FORCE_RESET = 1 << 8
FLAG_SCALE_OBSERVATIONS = 1 << 9
FLAG_VINE_RANDOMIZE = 1 << 10
FLAG_STALE_BODY_STATE_AFTER_RESET = 1 << 11
FLAG_IMPLICIT_JOINT_DAMPING = 1 << 12
FLAG_FPAM_DAMPING_HELD = 1 << 13
FLAG_CREATE_PIPE = 1 << 14
FLAG_INTROSPECT = 1 << 15

# VineField
VF_Q0 = 0
VF_QD0 = 6
VF_TIP_Y, VF_TIP_Z, VF_TIP_VY, VF_TIP_VZ = 12, 13, 14, 15
VF_CART_Y, VF_CART_VY = 16, 17
VF_TARGET_Y, VF_TARGET_Z = 18, 19
VF_SMOOTHED_U, VF_U_FPAM, VF_U_RAIL, VF_PREV_U_RAIL = 20, 21, 22, 23
VF_PREV_CART_VEL, VF_PREV_CART_VEL_ERR = 24, 25
VF_OBJ_DEPTH, VF_OBJ_ANGLE = 26, 27
VF_AGG_REW = 28
VF_CONTACT, VF_CONTACT_MEAN = 29, 30
VF_SHELF_Y, VF_SHELF_Z = 31, 32
VF_RAIL_FORCE = 33
VF_PREV_Q0 = 34
VF_PREV_TIP_Y, VF_PREV_TIP_Z = 40, 41
VF_FIFO0 = 42
VF_PIPE_Y, VF_PIPE_Z = 42 + 2 * MAX_DELAY, 43 + 2 * MAX_DELAY
VF_COUNT = 44 + 2 * MAX_DELAY

# VineStat (layout of vine_stats' output vector)
NUM_STATS = 128
(VS_DIST_MEAN, VS_TARGET_REACHED, VS_LIMIT_HIT, VS_TIP_LIMIT_HIT, VS_ABS_TIP_Y, VS_TIP_Z, VS_MAX_ABS_TIP_Y, VS_MAX_TIP_Z,
 VS_TIP_VEL_MEAN, VS_TIP_VEL_MAX, VS_U_RAIL_ABS, VS_PREV_U_RAIL_ABS, VS_RAIL_FORCE_ABS, VS_U_FPAM_ABS, VS_SMOOTHED_ABS,
 VS_PROGRESS_MEAN, VS_CONTACT_MEAN, VS_CONTACT_NONZERO, VS_AGG_MEAN, VS_AGG_STD, VS_REW_MEAN, VS_REW_MAX) = range(22)
VS_VIEW0 = 24
VS_VIEW_U = VS_VIEW0 + 28
VS_TERM0 = 64
VS_COUNT_USED = VS_TERM0 + 3 * NUM_REWARDS


class VineConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_envs", C.c_int32),
        ("obs_type", C.c_int32),
        ("control_freq_inv", C.c_int32),
        ("substeps", C.c_int32),
        ("max_episode_length", C.c_int32),
        ("action_delay", C.c_int32),
        ("flags", C.c_uint32),
        ("seed", C.c_uint64),
        ("dt", C.c_float),
        ("gravity", C.c_float),
        ("clip_observations", C.c_float),
        ("clip_actions", C.c_float),
        ("fpam_min", C.c_float),
        ("fpam_max", C.c_float),
        ("rail_velocity_scale", C.c_float),
        ("damping", C.c_float),
        ("stiffness", C.c_float),
        ("rail_soft_limit", C.c_float),
        ("rail_p_gain", C.c_float),
        ("rail_d_gain", C.c_float),
        ("rail_acceleration", C.c_float),
        ("smoothing_alpha_inflate", C.c_float),
        ("smoothing_alpha_deflate", C.c_float),
        ("random_init_cart_min_y", C.c_float),
        ("random_init_cart_max_y", C.c_float),
        ("success_dist", C.c_float),
        ("min_target_depth", C.c_float),
        ("max_target_depth", C.c_float),
        ("min_target_y", C.c_float),
        ("max_target_y", C.c_float),
        ("min_target_z", C.c_float),
        ("max_target_z", C.c_float),
        ("reward_weights", C.c_float * NUM_REWARDS),
        ("dyn_scale_min", C.c_float),
        ("dyn_scale_max", C.c_float),
        ("obs_noise_std", C.c_float),
        ("action_noise_std", C.c_float),
        ("cart_mass", C.c_float),
        ("link_mass", C.c_float * NUM_LINKS),
        ("link_inertia", C.c_float * NUM_LINKS),
        ("link_length", C.c_float),
        ("link_com", C.c_float),
        ("joint1_z", C.c_float),
        ("phi0", C.c_float),
        ("link_angular_damping", C.c_float),
        ("fpam_K", C.c_float * NUM_LINKS),
        ("fpam_C", C.c_float * NUM_LINKS),
        ("fpam_b", C.c_float * NUM_LINKS),
        ("fpam_B", C.c_float * NUM_LINKS),
        ("obs_scaling", C.c_float * MAX_OBS),
        ("env_id_offset", C.c_int32),
        ("effort_limit", C.c_float),
    ]

    def set_flag(self, flag, on):
        self.flags = (self.flags | flag) if on else (self.flags & ~flag)

    def has_flag(self, flag):
        return bool(self.flags & flag)


_P = C.POINTER
_H = C.c_void_p  # VineHandle*

# name -> (restype, argtypes); one row per declaration in include/vine.h
PROTOTYPES = {
    "vine_config_default": (C.c_int, [_P(VineConfig)]),
    "vine_config_set_obs_type": (C.c_int, [_P(VineConfig), C.c_int, C.c_int]),
    "vine_num_obs": (C.c_int, [_P(VineConfig)]),
    "vine_create": (C.c_int, [_P(VineConfig), C.c_int, C.c_void_p, _P(_H)]),
    "vine_destroy": (None, [_H]),
    "vine_step": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vine_reset_idx": (C.c_int, [_H, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vine_bind_reset_values": (C.c_int, [_H, C.c_void_p]),
    "vine_state_ptr": (C.c_void_p, [_H]),
    "vine_get_step_count": (C.c_int64, [_H]),
    "vine_set_step_count": (C.c_int, [_H, C.c_int64]),
    "vine_bind_reward_matrix": (C.c_int, [_H, C.c_void_p]),
    "vine_set_introspection": (C.c_int, [_H, C.c_int]),
    "vine_stats": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "vine_last_error": (C.c_char_p, []),
    "vine_step_kernel_name": (C.c_char_p, [_H]),
    "vine_backend_name": (C.c_char_p, []),
}


_I64 = C.c_int64
_VP = C.c_void_p
PPO_PARTIAL_BLOCKS = 512   # VINE_PPO_PARTIAL_BLOCKS
PPO_LOSS_SCRATCH_FLOATS = 1024 * 32   # VINE_PPO_LOSS_SCRATCH_FLOATS
ROLLOUT_POST_SCRATCH_FLOATS = 1024 * 3    # VINE_ROLLOUT_POST_SCRATCH_FLOATS
RMS_BLOCKS = 128   # VINE_RMS_BLOCKS
class LossFinalize(C.Structure):
    """``VineLossFinalize`` of include/vine_ppo.h (the deferred last step of ``vine_ln_heads_loss``)."""
    _fields_ = [("partial", C.c_void_p), ("blocks", C.c_int32), ("A", C.c_int32), ("n", C.c_int64), ("logstd", C.c_void_p),
                ("critic_coef", C.c_float), ("entropy_coef", C.c_float), ("bounds_coef", C.c_float), ("stats", C.c_void_p),
                ("grad_logstd", C.c_void_p), ("grad_mu_bias", C.c_void_p), ("grad_value_bias", C.c_void_p),
                ("kl_out", C.c_void_p), ("logstd_grad_accum", C.c_void_p), ("loss_scale", C.c_void_p)]


# include/vine_ppo.h (product library only; the oracle does not implement these)
PPO_PROTOTYPES = {
    "vine_column_sums_batched_fin": (C.c_int, [C.c_int32] + [_VP] * 8 + [_VP, _VP, _VP]),
    "vine_lstm_cell_forward": (C.c_int, [_I64, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP, _VP, _VP,
                                         _VP, _I64, C.c_int32, _I64, _VP]),
    "vine_lstm_step_mfma": (C.c_int, [_I64, _I64, _I64, _VP, _I64, _VP, _I64, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _VP,
                                      _I64, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _I64, _VP]),
    "vine_lstm_seq_forward_mfma": (C.c_int, [_I64, _I64, _I64, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                             C.c_int32, _VP, _VP, _VP]),
    "vine_lstm_seq_backward_mfma": (C.c_int, [_I64, _I64, _I64] + [_VP] * 8 + [C.c_int32, _VP, C.c_int32, _VP]),
    "vine_lstm_tile_weights": (C.c_int, [_I64, _I64, _VP, _I64, C.c_int32, _VP, _VP]),
    "vine_linear_elu_mfma": (C.c_int, [_I64, _I64, _I64, _VP, _I64, _VP, _I64, _VP, C.c_float, _VP, _I64, _VP]),
    "vine_linear_bwd_elu_mfma": (C.c_int, [_I64, _I64, _I64, _VP, _I64, _VP, _I64, _VP, _I64, C.c_float, _VP, _I64, _VP,
                                           _VP]),
    "vine_lstm_cell_backward": (C.c_int, [_I64, _I64, _VP, _I64, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _VP,
                                          _I64, _VP, _VP, _VP, C.c_int32, _VP]),
    "vine_lstm_step_backward_mfma": (C.c_int, [_I64, _I64, _VP, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _I64, _VP, _VP, _VP,
                                               _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP]),
    "vine_mlp3_elu_mfma": (C.c_int, [_I64, _VP, _I64, _VP, _I64, _VP, _VP, C.c_float, C.c_float, _VP, _VP, _I64, _VP, _I64, _VP,
                                     _I64, _VP, _I64, _VP, _I64, C.c_float, _VP, _VP, _VP, _I64, _VP]),
    "vine_lstm_seq_backward_mlp3_mfma": (C.c_int, [_I64, _I64, _I64] + [_VP] * 9 + [_VP, _I64, _VP, _I64, _VP, _I64, _VP, _I64, _VP,
                                                   _VP, C.c_float] + [_VP] * 6 + [_VP]),
    "vine_trunk_phases": (C.c_int, [_VP, _VP]),
    "vine_trunk_args_size": (C.c_int64, []),
    "vine_mlp3_elu_mfma_prep": (C.c_int, [_I64, _VP, _I64, _VP, _I64, _VP, _VP, C.c_float, C.c_float, _VP, _I64, _VP, _I64, _VP,
                                          _I64, _VP, _I64, _VP, _I64, _VP, _I64, C.c_float, _VP, _VP, _VP, _I64,
                                          C.c_int32] + [_VP] * 10 + [_VP]),
    "vine_ln_heads_loss": (C.c_int, [_I64, _I64, C.c_int32, _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                     _VP, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, _VP, _VP, C.c_int32,
                                     _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vine_lp16_format": (C.c_char_p, []),
    "vine_ppo_runtime_init": (C.c_int, []),
    "vine_mlp3_elu_f32": (C.c_int, [_I64, _VP, _I64, _VP, _I64, _VP, _VP, C.c_float, C.c_float, _VP, _I64, _VP, _I64, _VP, _I64,
                                    _VP, _I64, _VP, _I64, _VP, _I64, C.c_float, _VP]),
    "vine_mlp3_elu_f32_fin": (C.c_int, [_I64, _VP, _I64, _VP, _I64, _VP, _VP, C.c_float, C.c_float, _VP, _I64, _VP, _I64, _VP, _I64,
                                        _VP, _I64, _VP, _I64, _VP, _I64, C.c_float, _VP, C.c_float, _VP, _VP, C.c_int32, _VP]),
    "vine_mlp3_elu_f32_split": (C.c_int, [_I64, _VP, _I64, _VP, _I64, _VP, _VP, C.c_float, C.c_float, _VP, _VP, _VP, _VP, C.c_float,
                                          C.c_int, _VP, C.c_float, _VP, _VP, C.c_int32, _VP]),
    "vine_mlp3_tile_weights_split": (C.c_int, [_VP, _I64, _I64, _VP, _I64, _VP, _I64, _VP, _VP]),
    "vine_lstm_step_f32": (C.c_int, [_I64, _I64, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _I64, _VP]),
    "vine_lstm_tile_weights_f32": (C.c_int, [_I64, _I64, _VP, _I64, _VP, _VP]),
    "vine_lstm_step_f32_split": (C.c_int, [_I64, _I64, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _I64, C.c_int, _VP]),
    "vine_lstm_tile_weights_split": (C.c_int, [_I64, _I64, _VP, _I64, _VP, _VP]),
    "vine_ln_heads_loss_rows": (C.c_int, []),
    "vine_mlp3_bwd_elu_mfma": (C.c_int, [_I64, _VP, _I64, _I64, _VP, _I64, _VP, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _I64, _I64,
                                         _I64, C.c_float, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vine_weight_grad_group": (C.c_int, [C.c_int32] + [_VP] * 16 + [_VP]),
    "vine_weight_grad_cat_mfma": (C.c_int, [_I64, _I64, _VP, _I64, _VP, _I64, _I64, _I64, _VP, _I64, _I64, _I64, _I64, _I64,
                                            _VP, _VP, _VP]),
    "vine_weight_grad_cat_seq_mfma": (C.c_int, [_I64, _I64, _VP, _I64, _VP, _I64, _I64, _VP, _I64, _VP, _I64, _I64, _I64, _I64,
                                                _VP, _VP, _VP]),
    "vine_layernorm_forward": (C.c_int, [_I64, _I64, _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP]),
    "vine_layernorm_backward": (C.c_int, [_I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vine_layernorm_heads_forward": (C.c_int, [_I64, _I64, _I64, _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vine_layernorm_heads_backward": (C.c_int, [_I64, _I64, _I64] + [_VP] * 10),
    "vine_elu_backward": (C.c_int, [_I64, _I64, _VP, _I64, _VP, _I64, C.c_float, _VP, _I64, _VP, C.c_int32, C.c_int32,
                                    _VP]),
    "vine_bias_elu": (C.c_int, [_I64, _I64, _VP, _VP, C.c_float, _VP, _I64, C.c_int32, _VP]),
    "vine_ppo_loss": (C.c_int, [_I64, C.c_int32] + [_VP] * 10 + [C.c_float, C.c_int32, C.c_float, C.c_float, C.c_float,
                                                                C.c_float] + [_VP] * 4 + [_I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vine_copy_batched": (C.c_int, [C.c_int32] + [_VP] * 10 + [_VP]),
    "vine_column_sums_batched": (C.c_int, [C.c_int32] + [_VP] * 8 + [_VP, _VP]),
    "vine_column_sums": (C.c_int, [_I64, _I64, _VP, _I64, _VP, _I64, _VP, C.c_int32, _VP]),
    "vine_policy_head": (C.c_int, [_I64, C.c_int32, _I64] + [_VP] * 8 + [C.c_int32, C.c_uint64] + [_VP] * 6 +
                         [_VP, _VP, C.c_float, _VP]),
    "vine_policy_head_rms": (C.c_int, [_I64, C.c_int32, _I64] + [_VP] * 8 + [C.c_float, C.c_uint64] + [_VP] * 6 +
                             [_VP, _VP, C.c_float, _VP]),
    "vine_rollout_post": (C.c_int, [_I64, _I64] + [_VP] * 4 + [C.c_float] * 3 + [_VP] * 7 + [C.c_float, _VP, _VP, _I64,
                                                                                                  C.c_int32, _VP, _VP]),
    "vine_rollout_post_blocks": (C.c_int32, [_I64]),
    "vine_step_rollout": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vine_step_rollout_blocks": (C.c_int32, [_VP]),
    "vine_step_rollout_args_size": (C.c_int32, []),
    "vine_rollout_head_prep": (C.c_int, [_VP] * 9),
    "vine_step_eval": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vine_step_eval_rows": (C.c_int32, [_VP]),
    "vine_step_eval_args_size": (C.c_int32, []),
    "vine_rollout_finalize": (C.c_int, [_VP, C.c_float, _VP, _VP, C.c_int32, _VP]),
    "vine_rollout_post_defer": (C.c_int, [_I64, _I64] + [_VP] * 4 + [C.c_float] * 3 + [_VP] * 6 + [_VP, _I64, C.c_int32, _VP, _VP]),
    "vine_gae": (C.c_int, [C.c_int32, _I64, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _VP, _VP, _VP]),
    "vine_dataset_assemble": (C.c_int, [C.c_int32, _I64, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _VP, _VP, _VP, C.c_float,
                                        C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vine_rms_update": (C.c_int, [_I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vine_rms_update_multi": (C.c_int, [C.c_int32, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vine_normalize_obs": (C.c_int, [_I64, _I64, _VP, _VP, _VP, C.c_float, C.c_float, _VP, _I64, C.c_int32, _VP]),
    "vine_adam_step": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.c_float, _VP, _VP]),
    "vine_adam_step_sched": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.c_float, _VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float, _VP]),
    "vine_adam_step_amp": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float,
                                     C.c_float, _VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float, _VP, _VP, _VP]),
    "vine_grad_sqnorm_parts": (C.c_int32, [_I64]),
    "vine_grad_sqnorm": (C.c_int, [_I64, _VP, _VP, _VP]),
    "vine_adam_step_clip": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.c_float, _VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float, _VP, _VP,
                                      _VP, C.c_int32, C.c_float, _VP, _VP]),
    "vine_adam_step_emit": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.c_float, _VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float, _VP, _VP,
                                      _VP, C.c_int32, C.c_float, _VP, C.c_int32] + [_VP] * 8 + [_VP]),
    "vine_adaptive_lr": (C.c_int, [_VP, _VP, C.c_float, C.c_float, C.c_float, C.c_float, _VP]),
}


class RolloutArgs(C.Structure):
    """VineRolloutArgs of include/vine_ppo.h (vine_step_rollout)."""
    _fields_ = ([(k, C.c_void_p) for k in ("y", "hw", "hc", "logstd", "value_mean", "value_var")] +
                [("ln_eps", C.c_float), ("value_eps", C.c_float), ("seed", C.c_uint64), ("counter", C.c_void_p)] +
                [(k, C.c_void_p) for k in ("mu_out", "sigma_out", "value_out", "action_out", "neglogp_out")] +
                [("reward_shift", C.c_float), ("reward_scale", C.c_float), ("gamma_bootstrap", C.c_float), ("reserved", C.c_int32)] +
                [(k, C.c_void_p) for k in ("shaped_out", "dones_out", "cur_rewards", "cur_lengths", "h_state", "c_state", "h_op")] +
                [("h_op_stride", C.c_int64), ("partial", C.c_void_p)])


# vine_step_eval (include/vine_ppo.h): fields of the per-env episode accumulators, columns of the per-workgroup totals
EVAL_EPISODE_FIELDS = 4
(EVAL_EP_RETURN, EVAL_EP_LENGTH, EVAL_EP_MIN_DIST, EVAL_EP_FIRST_REACH) = range(4)
EVAL_NUM_TOTALS = 12
(EVAL_EPISODES, EVAL_RETURN_SUM, EVAL_LENGTH_SUM, EVAL_REACHED_EVER, EVAL_REACHED_AT_END, EVAL_FIRST_REACH_SUM,
 EVAL_FINAL_DIST_SUM, EVAL_MIN_DIST_SUM, EVAL_END_TIMEOUT, EVAL_END_RAIL_LIMIT, EVAL_END_TIP_LIMIT, EVAL_END_CONTACT) = range(12)


class EvalArgs(C.Structure):
    """VineEvalArgs of include/vine_ppo.h (vine_step_eval)."""
    _fields_ = ([(k, C.c_void_p) for k in ("y", "hw", "hc", "logstd")] +
                [("ln_eps", C.c_float), ("deterministic", C.c_int32), ("seed", C.c_uint64)] +
                [(k, C.c_void_p) for k in ("mu_out", "action_out", "dones_out", "h_state", "c_state", "h_op")] +
                [("h_op_stride", C.c_int64), ("episode", C.c_void_p), ("totals", C.c_void_p)])


class TrunkArgs(C.Structure):
    """VineTrunkArgs of include/vine_ppo.h (vine_trunk_phases)."""
    _fields_ = ([("B", C.c_int64), ("T", C.c_int64), ("x", C.c_void_p), ("ldx", C.c_int64)] +
                [(k, C.c_void_p) for k in ("w_tiled", "bias", "c0", "h0", "done", "h_out", "c_all", "gates", "c_last", "ln_gamma",
                                           "ln_beta")] +
                [("ln_eps", C.c_float), ("clip_value", C.c_int32)] +
                [(k, C.c_void_p) for k in ("w_heads", "b_heads", "logstd", "actions", "old_neglogp", "advantages", "old_values",
                                           "returns", "old_mu", "old_sigma")] +
                [(k, C.c_float) for k in ("e_clip", "critic_coef", "entropy_coef", "bounds_coef", "soft_bound", "alpha")] +
                [(k, C.c_void_p) for k in ("heads", "d_out", "ln_partial", "loss_partial", "stats", "grad_logstd", "grad_mu_bias",
                                           "grad_value_bias", "kl_out", "logstd_grad_accum", "mu_store", "sigma_store",
                                           "loss_scale", "found_inf", "w_hh_tiled", "dgates", "bias_partial")] +
                [("wt0", C.c_void_p), ("ldw0", C.c_int64), ("wt1", C.c_void_p), ("ldw1", C.c_int64), ("wt2", C.c_void_p),
                 ("ldw2", C.c_int64), ("a3", C.c_void_p), ("a3_stride", C.c_int64), ("a2", C.c_void_p), ("a1", C.c_void_p)] +
                [(k, C.c_void_p) for k in ("gz3", "gz2", "gz1", "part3", "part2", "part1")] +
                # appended (all zero: the four-phase launch): the second bias pointer, then phase 0 = the MLP forward
                [("bias2", C.c_void_p), ("mlp_raw", C.c_void_p), ("mlp_F_in", C.c_int64), ("mlp_mean", C.c_void_p),
                 ("mlp_var", C.c_void_p), ("mlp_eps", C.c_float), ("mlp_clip", C.c_float), ("mlp_w1", C.c_void_p),
                 ("mlp_ldw1", C.c_int64), ("mlp_b1", C.c_void_p), ("mlp_w2", C.c_void_p), ("mlp_ldw2", C.c_int64),
                 ("mlp_b2", C.c_void_p), ("mlp_w3", C.c_void_p), ("mlp_ldw3", C.c_int64), ("mlp_b3", C.c_void_p)])


# ---- include/vine_render.h (product library only)
RENDER_ABI_VERSION = 1
RENDER_LINE_PX = 2.5
RENDER_TIP_RADIUS = 0.012
RENDER_MAX_VIEWS = 64
# VineRenderMaterial = palette indices = pixel values
(VR_BACKGROUND, VR_RAIL, VR_LIMIT, VR_PROGRESS, VR_CART, VR_LINK_A, VR_LINK_B, VR_TIP, VR_TARGET, VR_SHELF, VR_STRIP,
 VR_PIPE) = range(12)
VR_NUM_MATERIALS = 12
RENDER_MATERIAL_NAMES = ("background", "rail", "limit", "progress", "cart", "link_a", "link_b", "tip", "target", "shelf",
                         "strip", "pipe")


class VineRenderConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("num_views", C.c_int32),
        ("grid_cols", C.c_int32),
        ("num_frames", C.c_int32),
        ("capture_every", C.c_int32),
        ("centre_y", C.c_float),
        ("centre_z", C.c_float),
        ("metres_per_pixel", C.c_float),
    ]

    @property
    def grid_rows(self):
        return (self.num_views + self.grid_cols - 1) // self.grid_cols

    @property
    def frame_shape(self):
        return (self.grid_rows * self.height, self.grid_cols * self.width)


RENDER_PROTOTYPES = {
    "vine_render_config_default": (C.c_int, [_P(VineRenderConfig)]),
    "vine_render_config_size": (C.c_int, []),
    "vine_render_frame_bytes": (C.c_int64, [_P(VineRenderConfig)]),
    "vine_render_ring_bytes": (C.c_int64, [_P(VineRenderConfig)]),
    "vine_render_palette": (C.c_int, [C.c_void_p, _P(C.c_int)]),
    "vine_render": (C.c_int, [_H, _P(VineRenderConfig), _VP, _VP, _VP, _VP]),
    "vine_render_scheduled": (C.c_int, [_H, _P(VineRenderConfig), _VP, _VP, _VP, _VP]),
}


def _attach(lib, prototypes):
    """Attach prototypes; raises AttributeError naming the first missing symbol."""
    for name, (restype, argtypes) in prototypes.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes


def declare_render(lib):
    _attach(lib, RENDER_PROTOTYPES)
    if lib.vine_render_config_size() != C.sizeof(VineRenderConfig):
        raise RuntimeError("VineRenderConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_record.h (product library only)
RECORD_ABI_VERSION = 1
RECORD_FIELDS = 32
RECORD_MAX_ENVS = 64
# VineRecordField = columns of a row
VRF_Q0, VRF_QD0 = 0, 6
VRF_TIP_Y, VRF_TIP_Z, VRF_TIP_VY, VRF_TIP_VZ = 12, 13, 14, 15
VRF_TARGET_Y, VRF_TARGET_Z = 16, 17
VRF_ACTION0 = 18
VRF_SMOOTHED_U, VRF_REWARD, VRF_RESET, VRF_TIMEOUT, VRF_PROGRESS = 20, 21, 22, 23, 24
VRF_OBJ_DEPTH, VRF_OBJ_ANGLE, VRF_CONTACT = 25, 26, 27
VRF_RESERVED0 = 28


class VineRecordConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("record_every", C.c_int32),
        ("num_steps", C.c_int32),
        ("num_envs", C.c_int32),
    ]


RECORD_PROTOTYPES = {
    "vine_record_config_default": (C.c_int, [_P(VineRecordConfig)]),
    "vine_record_config_size": (C.c_int, []),
    "vine_record_ring_bytes": (C.c_int64, [_P(VineRecordConfig)]),
    "vine_record": (C.c_int, [_H, _P(VineRecordConfig), C.c_int32] + [_VP] * 9),
    "vine_record_scheduled": (C.c_int, [_H, _P(VineRecordConfig)] + [_VP] * 9),
}


def declare_record(lib):
    _attach(lib, RECORD_PROTOTYPES)
    if lib.vine_record_config_size() != C.sizeof(VineRecordConfig):
        raise RuntimeError("VineRecordConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_episodes.h (product library only)
EPISODES_ABI_VERSION = 1
EPISODES_WORDS = 16
EPISODES_THREADS = 256
# VineEpisodeWord = the 32-bit words of a row
VEW_ENV, VEW_END_STEP, VEW_LENGTH, VEW_RETURN = 0, 1, 2, 3
VEW_REACHED_EVER, VEW_REACHED_AT_END, VEW_FIRST_REACH, VEW_FINAL_DIST, VEW_MIN_DIST = 4, 5, 6, 7, 8
VEW_END_REASON = 9
VEW_TARGET_Y, VEW_TARGET_Z, VEW_OBJ_DEPTH, VEW_OBJ_ANGLE = 10, 11, 12, 13
VEW_RESERVED0 = 14
EPISODES_END_TIMEOUT, EPISODES_END_RAIL_LIMIT, EPISODES_END_TIP_LIMIT, EPISODES_END_CONTACT = 1, 2, 4, 8


class VineEpisodesConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("reserved", C.c_int32),
        ("capacity", C.c_int64),
    ]


EPISODES_PROTOTYPES = {
    "vine_episodes_config_default": (C.c_int, [_P(VineEpisodesConfig)]),
    "vine_episodes_config_size": (C.c_int, []),
    "vine_episodes_rows": (C.c_int, [_H]),
    "vine_episodes_table_bytes": (C.c_int64, [_P(VineEpisodesConfig)]),
    "vine_episodes_scheduled": (C.c_int, [_H, _P(VineEpisodesConfig)] + [_VP] * 9),
}


def declare_episodes(lib):
    _attach(lib, EPISODES_PROTOTYPES)
    if lib.vine_episodes_config_size() != C.sizeof(VineEpisodesConfig):
        raise RuntimeError("VineEpisodesConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_env_params.h (product library only)
# VineEnvParam = rows of the per-env parameter table [VP_COUNT, num_envs]
(VP_DAMPING, VP_SMOOTHING_ALPHA_INFLATE, VP_SMOOTHING_ALPHA_DEFLATE, VP_RAIL_VELOCITY_SCALE, VP_RAIL_P_GAIN, VP_RAIL_D_GAIN,
 VP_RAIL_ACCELERATION, VP_ACTION_DELAY) = range(8)
VP_FPAM_K0, VP_FPAM_C0, VP_FPAM_b0, VP_FPAM_B0 = 8, 13, 18, 23
VP_COUNT = 28
# name (the task YAML's key) -> (first row, number of rows)
ENV_PARAM_ROWS = {
    "DAMPING": (VP_DAMPING, 1),
    "SMOOTHING_ALPHA_INFLATE": (VP_SMOOTHING_ALPHA_INFLATE, 1),
    "SMOOTHING_ALPHA_DEFLATE": (VP_SMOOTHING_ALPHA_DEFLATE, 1),
    "RAIL_VELOCITY_SCALE": (VP_RAIL_VELOCITY_SCALE, 1),
    "RAIL_P_GAIN": (VP_RAIL_P_GAIN, 1),
    "RAIL_D_GAIN": (VP_RAIL_D_GAIN, 1),
    "RAIL_ACCELERATION": (VP_RAIL_ACCELERATION, 1),
    "ACTION_DELAY": (VP_ACTION_DELAY, 1),
    "FPAM_K": (VP_FPAM_K0, NUM_LINKS),
    "FPAM_C": (VP_FPAM_C0, NUM_LINKS),
    "FPAM_b": (VP_FPAM_b0, NUM_LINKS),
    "FPAM_B": (VP_FPAM_B0, NUM_LINKS),
}
ENV_PARAM_NAMES = tuple(ENV_PARAM_ROWS)
# one name per row: the FPAM vectors as NAME[j]
ENV_PARAM_ROW_NAMES = tuple(name if cnt == 1 else "%s[%d]" % (name, j)
                            for name, (_, cnt) in ENV_PARAM_ROWS.items() for j in range(cnt))

ENV_PARAMS_PROTOTYPES = {
    "vine_env_params_row": (C.c_int, [_P(VineConfig), _P(C.c_float)]),
    "vine_env_params_check": (C.c_int, [_P(VineConfig), _VP, C.c_int]),
    "vine_bind_env_params": (C.c_int, [_H, _VP]),
    "vine_env_params_bound": (C.c_int, [_H]),
}


def declare_env_params(lib):
    _attach(lib, ENV_PARAMS_PROTOTYPES)
    return lib


# ---- include/vine_env_inertia.h (product library only)
# VineEnvInertia = rows of the per-env inertia table [VI_COUNT, num_envs]: 11 primary rows (what a user states), 20 derived
# rows (what the step kernel reads; vine_env_inertia_derive fills them)
VI_CART_MASS, VI_LINK_MASS0, VI_LINK_INERTIA0, VI_PRIMARY_COUNT = 0, 1, 6, 11
VI_MTOT, VI_B0, VI_GB0, VI_ADIAG0, VI_AOFF1 = 11, 12, 17, 22, 27
VI_COUNT = 31
# one name per row, the library's own (vine_env_inertia_check names a refused value by it)
ENV_INERTIA_ROW_NAMES = (("CART_MASS",) + tuple("LINK_MASS[%d]" % i for i in range(NUM_LINKS))
                         + tuple("LINK_INERTIA[%d]" % i for i in range(NUM_LINKS)) + ("MTOT",)
                         + tuple("%s[%d]" % (name, i) for name in ("B", "GB", "ADIAG") for i in range(NUM_LINKS))
                         + tuple("AOFF[%d]" % i for i in range(1, NUM_LINKS)))
# the names of the ENV_PARAMS spec that fill this table instead of the parameter table (utils/env_params.py): CART_MASS in
# kg, LINK_MASS a factor on the configuration's five link masses and inertias, TIP_LINK_MASS a further factor on link 4's
ENV_INERTIA_NAMES = ("CART_MASS", "LINK_MASS", "TIP_LINK_MASS")

ENV_INERTIA_PROTOTYPES = {
    "vine_env_inertia_row": (C.c_int, [_P(VineConfig), _P(C.c_float)]),
    "vine_env_inertia_derive": (C.c_int, [_P(VineConfig), _VP, C.c_int]),
    "vine_env_inertia_check": (C.c_int, [_P(VineConfig), _VP, C.c_int]),
    "vine_bind_env_inertia": (C.c_int, [_H, _VP]),
    "vine_env_inertia_bound": (C.c_int, [_H]),
}


def declare_env_inertia(lib):
    _attach(lib, ENV_INERTIA_PROTOTYPES)
    return lib


# ---- include/vine_env_redraw.h (product library only)
ENV_REDRAW_ABI_VERSION = 1
ENV_REDRAW_THREADS = 256
# VineEnvRedrawSlot = the names of a spec: the twelve of the parameter table, then the three of the inertia table
ENV_REDRAW_NAMES = ENV_PARAM_NAMES + ENV_INERTIA_NAMES
VR_NAMES = 15
REDRAW_ABSENT, REDRAW_NUMBER, REDRAW_RANGE, REDRAW_VALUES = range(4)


class VineEnvRedrawName(C.Structure):
    _fields_ = [
        ("form", C.c_int32),
        ("values_first", C.c_int32),
        ("values_count", C.c_int32),
        ("reserved", C.c_int32),
        ("key", C.c_uint64),
        ("radix", C.c_uint64),
        ("lo", C.c_double),
        ("hi", C.c_double),
    ]


class VineEnvRedrawSpec(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_values", C.c_int32),
        ("seed", C.c_uint64),
        ("values", C.c_void_p),
        ("name", VineEnvRedrawName * VR_NAMES),
        ("base_params", C.c_float * VP_COUNT),
        ("base_inertia", C.c_float * VI_PRIMARY_COUNT),
        ("link_length", C.c_float),
        ("link_com", C.c_float),
        ("gravity", C.c_float),
        ("checked", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


ENV_REDRAW_PROTOTYPES = {
    "vine_env_redraw_spec_size": (C.c_int, []),
    "vine_env_redraw_spec": (C.c_int, [_P(VineConfig), _P(VineEnvRedrawName), _VP, _VP, C.c_int, _P(VineEnvRedrawSpec)]),
    "vine_env_redraw_scheduled": (C.c_int, [_H, _P(VineEnvRedrawSpec)] + [_VP] * 5),
}


def declare_env_redraw(lib):
    _attach(lib, ENV_REDRAW_PROTOTYPES)
    if lib.vine_env_redraw_spec_size() != C.sizeof(VineEnvRedrawSpec):
        raise RuntimeError("VineEnvRedrawSpec: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_env_sensor.h (product library only)
ENV_SENSOR_ABI_VERSION = 1
ENV_SENSOR_THREADS = 256
SENSOR_MAX_DELAY = 8
SENSOR_SLOTS = SENSOR_MAX_DELAY + 1
SENSOR_RNG_NOISE, SENSOR_RNG_HOLD = 5, 6
# VineEnvSensorSlot = the rows of the sensor table; the draw's name keys are those of "SENSOR_" + name
ENV_SENSOR_NAMES = ["DELAY", "HOLD", "NOISE_STD"]
VSN_DELAY, VSN_HOLD, VSN_NOISE_STD = range(3)
VSN_NAMES = 3


class VineEnvSensorSpec(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_values", C.c_int32),
        ("seed", C.c_uint64),
        ("values", C.c_void_p),
        ("name", VineEnvRedrawName * VSN_NAMES),
        ("num_obs", C.c_int32),
        ("column_mask", C.c_uint32),
        ("clip_observations", C.c_float),
        ("per_episode", C.c_int32),
        ("checked", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


ENV_SENSOR_PROTOTYPES = {
    "vine_env_sensor_spec_size": (C.c_int, []),
    "vine_env_sensor_spec": (C.c_int, [_P(VineConfig), _P(VineEnvRedrawName), _VP, _VP, C.c_int, C.c_uint32, C.c_int,
                                       _P(VineEnvSensorSpec)]),
    "vine_env_sensor_scheduled": (C.c_int, [_H, _P(VineEnvSensorSpec)] + [_VP] * 8),
}


def declare_env_sensor(lib):
    _attach(lib, ENV_SENSOR_PROTOTYPES)
    if lib.vine_env_sensor_spec_size() != C.sizeof(VineEnvSensorSpec):
        raise RuntimeError("VineEnvSensorSpec: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_env_push.h (product library only)
ENV_PUSH_ABI_VERSION = 1
ENV_PUSH_THREADS = 256
PUSH_MAX_POINTS = 6
PUSH_COMPOSITES = 20               # = VI_COUNT - VI_MTOT
PUSH_RNG = 7
# VineEnvPushSlot = the rows of the push table; the draw's name keys are those of "PUSH_" + name
ENV_PUSH_NAMES = ["RATE", "IMPULSE"]
VPU_RATE, VPU_IMPULSE = range(2)
VPU_NAMES = 2


class VineEnvPushSpec(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_values", C.c_int32),
        ("seed", C.c_uint64),
        ("values", C.c_void_p),
        ("name", VineEnvRedrawName * VPU_NAMES),
        ("num_points", C.c_int32),
        ("per_episode", C.c_int32),
        ("points", C.c_int32 * PUSH_MAX_POINTS),
        ("composites", C.c_float * PUSH_COMPOSITES),
        ("checked", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


ENV_PUSH_PROTOTYPES = {
    "vine_env_push_spec_size": (C.c_int, []),
    "vine_env_push_spec": (C.c_int, [_P(VineConfig), _P(VineEnvRedrawName), _VP, _VP, C.c_int, _P(C.c_int32), C.c_int, C.c_int,
                                     _P(VineEnvPushSpec)]),
    "vine_env_push_scheduled": (C.c_int, [_H, _P(VineEnvPushSpec)] + [_VP] * 5),
}


def declare_env_push(lib):
    _attach(lib, ENV_PUSH_PROTOTYPES)
    if lib.vine_env_push_spec_size() != C.sizeof(VineEnvPushSpec):
        raise RuntimeError("VineEnvPushSpec: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_env_target.h (product library only)
ENV_TARGET_ABI_VERSION = 1
ENV_TARGET_THREADS = 256
# VineEnvTargetSlot = the rows of the target table; the draw's name keys are those of "TARGET_" + name
ENV_TARGET_NAMES = ["VEL_ALONG", "VEL_ACROSS", "SPAN_ALONG", "SPAN_ACROSS"]
VTG_VEL_ALONG, VTG_VEL_ACROSS, VTG_SPAN_ALONG, VTG_SPAN_ACROSS = range(4)
VTG_NAMES = 4
# VineEnvTargetRow = the rows of the observer's own per-env state
(VTM_ANCHOR_Y, VTM_ANCHOR_Z, VTM_DEPTH0, VTM_AXIS_C, VTM_AXIS_S, VTM_OFF_ALONG, VTM_OFF_ACROSS, VTM_VEL_ALONG,
 VTM_VEL_ACROSS) = range(9)
VTM_COUNT = 9
TARGET_FREE, TARGET_SHELF, TARGET_PIPE = range(3)


class VineEnvTargetSpec(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_values", C.c_int32),
        ("seed", C.c_uint64),
        ("values", C.c_void_p),
        ("name", VineEnvRedrawName * VTG_NAMES),
        ("mode", C.c_int32),
        ("num_obs", C.c_int32),
        ("vel_column", C.c_int32),
        ("per_episode", C.c_int32),
        ("cdt", C.c_float),
        ("clip_observations", C.c_float),
        ("inv_obs_scale", C.c_float * 2),
        ("checked", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


ENV_TARGET_PROTOTYPES = {
    "vine_env_target_spec_size": (C.c_int, []),
    "vine_env_target_spec": (C.c_int, [_P(VineConfig), _P(VineEnvRedrawName), _VP, _VP, C.c_int, C.c_int, _P(VineEnvTargetSpec)]),
    "vine_env_target_scheduled": (C.c_int, [_H, _P(VineEnvTargetSpec)] + [_VP] * 8),
}


def declare_env_target(lib):
    _attach(lib, ENV_TARGET_PROTOTYPES)
    if lib.vine_env_target_spec_size() != C.sizeof(VineEnvTargetSpec):
        raise RuntimeError("VineEnvTargetSpec: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_env_adr.h (product library only)
ENV_ADR_ABI_VERSION = 1
ENV_ADR_THREADS = 256
ENV_ADR_HISTORY_WORDS = 4
ENV_ADR_KEY_PROBE = 0x32006ca9afc13c78      # env_params.name_key("ADR_PROBE")
ENV_ADR_KEY_WHICH = 0x25473c155fa82938      # env_params.name_key("ADR_WHICH")


class VineEnvAdrName(C.Structure):
    _fields_ = [
        ("on", C.c_int32),
        ("reserved", C.c_int32),
        ("start_lo", C.c_double),
        ("start_hi", C.c_double),
        ("step", C.c_double),
    ]


class VineEnvAdrSpec(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_adr", C.c_int32),
        ("queue", C.c_int32),
        ("history_capacity", C.c_int32),
        ("boundary_fraction", C.c_double),
        ("widen_at", C.c_double),
        ("narrow_at", C.c_double),
        ("name", VineEnvAdrName * VR_NAMES),
        ("max_widen", (C.c_int32 * 2) * VR_NAMES),
        ("adr_slot", C.c_int32 * VR_NAMES),
        ("checked", C.c_uint32),
        ("reserved", C.c_uint32),
        ("redraw", VineEnvRedrawSpec),
    ]


ENV_ADR_PROTOTYPES = {
    "vine_env_adr_spec_size": (C.c_int, []),
    "vine_env_adr_spec": (C.c_int, [_P(VineConfig), _P(VineEnvRedrawSpec), _P(VineEnvAdrName), C.c_double, C.c_int, C.c_double,
                                    C.c_double, C.c_int, _P(VineEnvAdrSpec)]),
    "vine_env_adr_scheduled": (C.c_int, [_H, _P(VineEnvAdrSpec)] + [_VP] * 11),
}


def declare_env_adr(lib):
    _attach(lib, ENV_ADR_PROTOTYPES)
    if lib.vine_env_adr_spec_size() != C.sizeof(VineEnvAdrSpec):
        raise RuntimeError("VineEnvAdrSpec: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_sysid.h (product library only)
SYSID_ABI_VERSION = 1
SYSID_FIELDS = 16


class VineSysidConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_rows", C.c_int32),
        ("horizon", C.c_int32),
        ("reserved", C.c_int32),
        ("weights", C.c_float * SYSID_FIELDS),
    ]


SYSID_PROTOTYPES = {
    "vine_sysid_config_default": (C.c_int, [_P(VineSysidConfig)]),
    "vine_sysid_config_size": (C.c_int, []),
    "vine_sysid_pin": (C.c_int, [_H, _P(VineSysidConfig), _VP, C.c_int64] + [_VP] * 6),
    "vine_sysid_scheduled": (C.c_int, [_H, _P(VineSysidConfig)] + [_VP] * 7),
}


def declare_sysid(lib):
    _attach(lib, SYSID_PROTOTYPES)
    if lib.vine_sysid_config_size() != C.sizeof(VineSysidConfig):
        raise RuntimeError("VineSysidConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_mpc.h (product library only)
MPC_ABI_VERSION = 1
MPC_THREADS = 256
MPC_MAX_HORIZON = 64
MPC_RNG_NOISE = 8


class VineMpcConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_plants", C.c_int32),
        ("samples", C.c_int32),
        ("horizon", C.c_int32),
        ("lambda_", C.c_double),       # `lambda` in the header
        ("sigma", C.c_float * 2),
        ("seed", C.c_uint64),
    ]


MPC_PROTOTYPES = {
    "vine_mpc_config_default": (C.c_int, [_P(VineMpcConfig)]),
    "vine_mpc_config_size": (C.c_int, []),
    "vine_mpc_fork": (C.c_int, [_H, _H, _P(VineMpcConfig)] + [_VP] * 12),
    "vine_mpc_scheduled": (C.c_int, [_H, _P(VineMpcConfig)] + [_VP] * 9),
    "vine_mpc_update": (C.c_int, [_H, _P(VineMpcConfig)] + [_VP] * 8),
}


def declare_mpc(lib):
    _attach(lib, MPC_PROTOTYPES)
    if lib.vine_mpc_config_size() != C.sizeof(VineMpcConfig):
        raise RuntimeError("VineMpcConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_mpc_adapt.h (product library only)
MPC_ADAPT_ABI_VERSION = 1
MPC_ADAPT_MAX_WINDOW = 32
MPC_ADAPT_MAX_DIMS = 8
MPC_ADAPT_FIELDS = 12
MPC_ADAPT_BASE_ROWS = 20
MPC_ADAPT_RNG = 9


class VineMpcAdaptDim(C.Structure):
    _fields_ = [
        ("first_row", C.c_int32),
        ("num_rows", C.c_int32),
        ("lo", C.c_double),
        ("hi", C.c_double),
        ("std_floor", C.c_double),
    ]


class VineMpcAdaptConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_plants", C.c_int32),
        ("samples", C.c_int32),
        ("window", C.c_int32),
        ("every", C.c_int32),
        ("num_dims", C.c_int32),
        ("min_steps", C.c_int32),
        ("forget_on_reset", C.c_int32),
        ("temperature", C.c_double),
        ("rate", C.c_double),
        ("seed", C.c_uint64),
        ("weights", C.c_float * MPC_ADAPT_FIELDS),
        ("base_rows", C.c_float * MPC_ADAPT_BASE_ROWS),
        ("dims", VineMpcAdaptDim * MPC_ADAPT_MAX_DIMS),
    ]


MPC_ADAPT_PROTOTYPES = {
    "vine_mpc_adapt_config_default": (C.c_int, [_P(VineMpcAdaptConfig)]),
    "vine_mpc_adapt_config_size": (C.c_int, []),
    "vine_mpc_adapt_anchor": (C.c_int, [_H, _P(VineMpcAdaptConfig)] + [_VP] * 11),
    "vine_mpc_adapt_trace": (C.c_int, [_H, _P(VineMpcAdaptConfig)] + [_VP] * 11),
    "vine_mpc_adapt_pin": (C.c_int, [_H, _P(VineMpcAdaptConfig)] + [_VP] * 15),
    "vine_mpc_adapt_scheduled": (C.c_int, [_H, _P(VineMpcAdaptConfig)] + [_VP] * 9),
    "vine_mpc_adapt_estimate": (C.c_int, [_H, _P(VineMpcAdaptConfig)] + [_VP] * 10),
}


def declare_mpc_adapt(lib):
    _attach(lib, MPC_ADAPT_PROTOTYPES)
    if lib.vine_mpc_adapt_config_size() != C.sizeof(VineMpcAdaptConfig):
        raise RuntimeError("VineMpcAdaptConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_mpc_policy.h (product library only)
MPC_POLICY_ABI_VERSION = 1
MPC_POLICY_UNITS = 256
MPC_POLICY_ROWS = 512


class VineMpcPolicyConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("obs_width", C.c_int32),
        ("ln_eps", C.c_float),
        ("value_eps", C.c_float),
        ("terminal_value", C.c_double),
    ]


_MPC_POLICY_HEAD = [_H, _P(VineMpcConfig), _P(VineMpcPolicyConfig)]
MPC_POLICY_PROTOTYPES = {
    "vine_mpc_policy_config_default": (C.c_int, [_P(VineMpcPolicyConfig)]),
    "vine_mpc_policy_config_size": (C.c_int, []),
    "vine_mpc_policy_fork": (C.c_int, [_H] + _MPC_POLICY_HEAD + [_VP, C.c_int32, _VP, C.c_int32] + [_VP] * 5 + [_I64, _VP]),
    "vine_mpc_policy_act": (C.c_int, _MPC_POLICY_HEAD + [_VP] * 13),
    "vine_mpc_policy_terminal": (C.c_int, _MPC_POLICY_HEAD + [_VP] * 10),
    "vine_mpc_policy_compose": (C.c_int, _MPC_POLICY_HEAD + [_VP] * 5),
}


def declare_mpc_policy(lib):
    _attach(lib, MPC_POLICY_PROTOTYPES)
    if lib.vine_mpc_policy_config_size() != C.sizeof(VineMpcPolicyConfig):
        raise RuntimeError("VineMpcPolicyConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_mpc_observe.h (product library only)
MPC_OBSERVE_ABI_VERSION = 1
MPC_OBSERVE_THREADS = 256
MPC_OBSERVE_SLOTS = MAX_DELAY + 1
MPC_OBSERVE_LOG = 2 * MAX_DELAY
MPC_OBSERVE_RNG_NOISE = 10
MPC_OBSERVE_RNG_HOLD = 11
MPC_OBSERVE_NAMES = ("DELAY", "HOLD", "NOISE_Q", "NOISE_QD")       # the rows of the per-plant table
VMO_DELAY, VMO_HOLD, VMO_NOISE_Q, VMO_NOISE_QD, VMO_NAMES = 0, 1, 2, 3, 4


class VineMpcObserveConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_plants", C.c_int32),
        ("catchup", C.c_int32),
        ("compensate", C.c_int32),
        ("seed", C.c_uint64),
    ]


MPC_OBSERVE_PROTOTYPES = {
    "vine_mpc_observe_config_default": (C.c_int, [_P(VineMpcObserveConfig)]),
    "vine_mpc_observe_config_size": (C.c_int, []),
    "vine_mpc_observe_measure": (C.c_int, [_H, _P(VineMpcObserveConfig)] + [_VP] * 8),
    "vine_mpc_observe_pin": (C.c_int, [_H, _H, _P(VineMpcObserveConfig)] + [_VP] * 12),
    "vine_mpc_observe_catchup": (C.c_int, [_H, _H, _P(VineMpcObserveConfig), C.c_int32] + [_VP] * 12),
}


def declare_mpc_observe(lib):
    _attach(lib, MPC_OBSERVE_PROTOTYPES)
    if lib.vine_mpc_observe_config_size() != C.sizeof(VineMpcObserveConfig):
        raise RuntimeError("VineMpcObserveConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_mpc_filter.h (product library only)
MPC_FILTER_ABI_VERSION = 1
MPC_FILTER_THREADS = 256
MPC_FILTER_NAMES = ("GAIN_Q", "GAIN_QD")                          # the rows of the per-plant gain table
VMF_GAIN_Q, VMF_GAIN_QD, VMF_NAMES = 0, 1, 2

MPC_FILTER_PROTOTYPES = {
    "vine_mpc_filter_abi_version": (C.c_int, []),
    "vine_mpc_filter_pin": (C.c_int, [_H, _H, _P(VineMpcObserveConfig)] + [_VP] * 12),
    "vine_mpc_filter_correct": (C.c_int, [_H, _H, _P(VineMpcObserveConfig)] + [_VP] * 9),
}


def declare_mpc_filter(lib):
    _attach(lib, MPC_FILTER_PROTOTYPES)
    if lib.vine_mpc_filter_abi_version() != MPC_FILTER_ABI_VERSION:
        raise RuntimeError("vine_mpc_filter.h: the library's ABI version differs from the ctypes mirror")
    return lib


# ---- include/vine_mpc_track.h (product library only)
MPC_TRACK_ABI_VERSION = 1
MPC_TRACK_THREADS = 256
MPC_TRACK_WORDS = 3                                                # TY, TZ, DEPTH of a path entry
MPC_TRACK_PATHS = ("exact", "linear", "held")                      # by VineMpcTrackPath
TRACK_EXACT, TRACK_LINEAR, TRACK_HELD = range(3)


class VineMpcTrackSpec(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_plants", C.c_int32),
        ("samples", C.c_int32),
        ("horizon", C.c_int32),
        ("mode", C.c_int32),
        ("path", C.c_int32),
        ("cdt", C.c_float),
        ("checked", C.c_uint32),
        ("reserved", C.c_uint32 * 8),
    ]


MPC_TRACK_PROTOTYPES = {
    "vine_mpc_track_spec_size": (C.c_int, []),
    "vine_mpc_track_spec": (C.c_int, [_P(VineEnvTargetSpec), _P(VineMpcConfig), C.c_int, _P(VineMpcTrackSpec)]),
    "vine_mpc_track_plan": (C.c_int, [_H, _P(VineMpcTrackSpec)] + [_VP] * 7),
    "vine_mpc_track_scheduled": (C.c_int, [_H, _P(VineMpcTrackSpec)] + [_VP] * 5),
}


def declare_mpc_track(lib):
    _attach(lib, MPC_TRACK_PROTOTYPES)
    if lib.vine_mpc_track_spec_size() != C.sizeof(VineMpcTrackSpec):
        raise RuntimeError("VineMpcTrackSpec: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_mpc_noise.h (product library only)
MPC_NOISE_ABI_VERSION = 1
MPC_NOISE_THREADS = 256


class VineMpcNoiseConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("beta", C.c_float * 2),
        ("adapt", C.c_int32),
        ("rate", C.c_double),
        ("sigma_min", C.c_float * 2),
        ("sigma_max", C.c_float * 2),
    ]


_MPC_NOISE_HEAD = [_H, _P(VineMpcConfig), _P(VineMpcNoiseConfig)]
MPC_NOISE_PROTOTYPES = {
    "vine_mpc_noise_config_default": (C.c_int, [_P(VineMpcNoiseConfig)]),
    "vine_mpc_noise_config_size": (C.c_int, []),
    "vine_mpc_noise_draw": (C.c_int, _MPC_NOISE_HEAD + [_VP] * 3),
    "vine_mpc_noise_scheduled": (C.c_int, _MPC_NOISE_HEAD + [_VP] * 6),
    "vine_mpc_noise_update": (C.c_int, _MPC_NOISE_HEAD + [_VP] * 10),
}


def declare_mpc_noise(lib):
    _attach(lib, MPC_NOISE_PROTOTYPES)
    if lib.vine_mpc_noise_config_size() != C.sizeof(VineMpcNoiseConfig):
        raise RuntimeError("VineMpcNoiseConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_mpc_ensemble.h (product library only)
MPC_ENSEMBLE_ABI_VERSION = 1
MPC_ENSEMBLE_MAX_MEMBERS = 16
MPC_RISK_MEAN, MPC_RISK_MAX, MPC_RISK_ENTROPIC = range(3)
MPC_RISK_NAMES = ("mean", "max", "entropic")                     # the RISK of an ``ensemble=`` mapping, by VINE_MPC_RISK_*


class VineMpcEnsembleConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("members", C.c_int32),
        ("risk", C.c_int32),
        ("theta", C.c_double),
    ]


_MPC_ENSEMBLE_HEAD = [_H, _P(VineMpcConfig), _P(VineMpcEnsembleConfig)]
MPC_ENSEMBLE_PROTOTYPES = {
    "vine_mpc_ensemble_config_default": (C.c_int, [_P(VineMpcEnsembleConfig)]),
    "vine_mpc_ensemble_config_size": (C.c_int, []),
    "vine_mpc_ensemble_scheduled": (C.c_int, _MPC_ENSEMBLE_HEAD + [_VP] * 5),
    "vine_mpc_ensemble_update": (C.c_int, _MPC_ENSEMBLE_HEAD + [_VP] * 9),
}


def declare_mpc_ensemble(lib):
    _attach(lib, MPC_ENSEMBLE_PROTOTYPES)
    if lib.vine_mpc_ensemble_config_size() != C.sizeof(VineMpcEnsembleConfig):
        raise RuntimeError("VineMpcEnsembleConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_mpc_adapt_inertia.h (product library only)
MPC_ADAPT_INERTIA_ABI_VERSION = 1
MPC_ADAPT_INERTIA_MAX_DIMS = 3
MPC_ADAPT_INERTIA_CART, MPC_ADAPT_INERTIA_LINK, MPC_ADAPT_INERTIA_TIP = range(3)      # in the order of ENV_INERTIA_NAMES


class VineMpcAdaptInertiaDim(C.Structure):
    _fields_ = [
        ("name", C.c_int32),
        ("reserved", C.c_int32),
        ("lo", C.c_double),
        ("hi", C.c_double),
        ("std_floor", C.c_double),
    ]


class VineMpcAdaptInertiaConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_mass_dims", C.c_int32),
        ("dims", VineMpcAdaptInertiaDim * MPC_ADAPT_INERTIA_MAX_DIMS),
        ("base_inertia", C.c_float * VI_PRIMARY_COUNT),
        ("link_length", C.c_float),
        ("link_com", C.c_float),
        ("gravity", C.c_float),
    ]


_MPC_ADAPT_INERTIA_HEAD = [_H, _P(VineMpcAdaptConfig), _P(VineMpcAdaptInertiaConfig)]
MPC_ADAPT_INERTIA_PROTOTYPES = {
    "vine_mpc_adapt_inertia_config_default": (C.c_int, [_P(VineMpcAdaptInertiaConfig)]),
    "vine_mpc_adapt_inertia_config_size": (C.c_int, []),
    "vine_mpc_adapt_inertia_pin": (C.c_int, _MPC_ADAPT_INERTIA_HEAD + [_VP] * 5),
    "vine_mpc_adapt_inertia_estimate": (C.c_int, _MPC_ADAPT_INERTIA_HEAD + [_VP] * 11),
}


def declare_mpc_adapt_inertia(lib):
    _attach(lib, MPC_ADAPT_INERTIA_PROTOTYPES)
    if lib.vine_mpc_adapt_inertia_config_size() != C.sizeof(VineMpcAdaptInertiaConfig):
        raise RuntimeError("VineMpcAdaptInertiaConfig: the library's struct size differs from the ctypes mirror")
    return lib


# ---- include/vine_env_draw_adr.h (product library only)
ENV_DRAW_ADR_ABI_VERSION = 1
ENV_DRAW_ADR_THREADS = 256
ENV_DRAW_ADR_HISTORY_WORDS = 4
ENV_DRAW_ADR_KEY_PROBE = 0x13605cadb5285d5e      # named_draw.name_key("DRAW_ADR_PROBE")
ENV_DRAW_ADR_KEY_WHICH = 0x5ce5f9cbbb3b47a7      # named_draw.name_key("DRAW_ADR_WHICH")
VDA_SENSOR, VDA_PUSH, VDA_TARGET = range(3)      # VineEnvDrawAdrGroup: whose table a name's row lies in
VDA_GROUPS = 3
# VineEnvDrawAdrSlotIndex: the draw names of the three observers, one group behind the other
ENV_DRAW_ADR_NAMES = (["SENSOR_" + n for n in ENV_SENSOR_NAMES] + ["PUSH_" + n for n in ENV_PUSH_NAMES]
                      + ["TARGET_" + n for n in ENV_TARGET_NAMES])
VDA_NAMES = 9
ENV_DRAW_ADR_INTEGER = ("SENSOR_DELAY",)


class VineEnvDrawAdrSlot(C.Structure):
    _fields_ = [
        ("adr", VineEnvAdrName),
        ("max_widen", C.c_int32 * 2),
        ("group", C.c_int32),
        ("row", C.c_int32),
        ("integer", C.c_int32),
        ("reserved", C.c_int32),
        ("limits", VineEnvRedrawName),
    ]


class VineEnvDrawAdrSpec(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_adr", C.c_int32),
        ("queue", C.c_int32),
        ("history_capacity", C.c_int32),
        ("boundary_fraction", C.c_double),
        ("widen_at", C.c_double),
        ("narrow_at", C.c_double),
        ("seed", C.c_uint64),
        ("slot", VineEnvDrawAdrSlot * VDA_NAMES),
        ("adr_slot", C.c_int32 * VDA_NAMES),
        ("checked", C.c_uint32),
    ]


ENV_DRAW_ADR_PROTOTYPES = {
    "vine_env_draw_adr_spec_size": (C.c_int, []),
    "vine_env_draw_adr_spec": (C.c_int, [_P(VineConfig), _P(VineEnvSensorSpec), _P(VineEnvPushSpec), _P(VineEnvTargetSpec),
                                         _P(VineEnvAdrName), C.c_double, C.c_int, C.c_double, C.c_double, C.c_int,
                                         _P(VineEnvDrawAdrSpec)]),
    "vine_env_draw_adr_scheduled": (C.c_int, [_H, _P(VineEnvDrawAdrSpec), _VP, _P(C.c_void_p)] + [_VP] * 9),
}


def declare_env_draw_adr(lib):
    _attach(lib, ENV_DRAW_ADR_PROTOTYPES)
    if lib.vine_env_draw_adr_spec_size() != C.sizeof(VineEnvDrawAdrSpec):
        raise RuntimeError("VineEnvDrawAdrSpec: the library's struct size differs from the ctypes mirror")
    return lib


def declare_ppo(lib):
    _attach(lib, PPO_PROTOTYPES)
    return lib


def declare(lib):
    _attach(lib, PROTOTYPES)
    return lib


def declare_all(lib):
    """Every prototype of the library, and the struct-size checks of the observers' configurations."""
    for declare_one in (declare, declare_ppo, declare_render, declare_record, declare_episodes, declare_env_params, declare_env_inertia,
                        declare_env_redraw, declare_env_adr, declare_env_sensor, declare_env_push, declare_env_target, declare_sysid, declare_mpc,
                        declare_mpc_adapt, declare_mpc_policy, declare_mpc_observe, declare_mpc_filter, declare_mpc_track,
                        declare_env_draw_adr, declare_mpc_noise, declare_mpc_adapt_inertia, declare_mpc_ensemble):
        declare_one(lib)
    return lib
