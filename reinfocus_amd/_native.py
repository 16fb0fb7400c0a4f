"""ctypes binding of libreinfocus_hip.so (include/reinfocus_hip.h).

The HIP library is the only compute path of this package: if it is missing or no GPU
is usable the calls below raise, loudly.  There is no CPU fallback (the CPU oracle
under oracle/ is test infrastructure and is never imported from here).
"""

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# REINFOCUS_HIP_LIB: an alternative build of the same library (tests use it for a build with a
# tiny cooperative list); never a different implementation -- there is no CPU fallback
LIB_PATH = os.environ.get("REINFOCUS_HIP_LIB") or os.path.join(_HERE, "libreinfocus_hip.so")

RF_OK = 0
RF_ERR_INVALID = -1
RF_ERR_HIP = -2
RF_ERR_NO_DEVICE = -3
RF_ERR_OOM = -4

GRAY_15BIT = 15
GRAY_14BIT = 14

ACTION_I32, ACTION_I64, ACTION_F32 = range(3)  # RF_ACTION_*

# every symbol include/reinfocus_hip.h declares
SYMBOLS = (
    "rf_last_error",
    "rf_abi_version",
    "rf_device_count",
    "rf_device_info",
    "rf_create",
    "rf_destroy",
    "rf_seed",
    "rf_num_states",
    "rf_get_states",
    "rf_set_states",
    "rf_set_scene",
    "rf_render",
    "rf_get_frames",
    "rf_upload_frames",
    "rf_focus",
    "rf_step",
    "rf_synchronize",
    "rf_timing",
    "rf_timing_read",
    "rf_render_general",
    "rf_env_configure",
    "rf_env_reset",
    "rf_env_step",
    "rf_env_step_begin",
    "rf_env_step_end",
    "rf_env_step_abort",
    "rf_env_step_plan",
    "rf_env_step_run",
    "rf_env_render_states",
    "rf_env_step_end_given",
    "rf_env_get_states",
    "rf_env_scene_len",
    "rf_env_render",
    "rf_env_get_counters",
    "rf_env_last_step_branch",
    "rf_env_configure_jumps",
    "rf_env_step_jumps",
    "rf_env_step_begin_jumps",
    "rf_env_step_plan_jumps",
    "rf_env_configure_composed",
    "rf_env_get_strategy_state",
    "rf_env_configure_observed",
    "rf_env_get_observer_state",
    "rf_env_configure_initializer",
    "rf_env_set_initializer_state",
    "rf_env_get_initializer_state",
    "rf_env_snapshot_size",
    "rf_env_snapshot",
    "rf_env_restore",
    "rf_env_snapshot_resident",
    "rf_env_restore_resident",
    "rf_env_snapshot_drop",
    "rf_env_step_device",
    "rf_env_reset_device",
    "rf_env_device_status",
    "rf_env_configure_records",
    "rf_env_get_records",
    "rf_env_get_record_accumulators",
    "rf_env_step_device_records",
    "rf_env_configure_view",
    "rf_env_get_view",
    "rf_env_view_get_statistics",
    "rf_env_view_set_statistics",
    "rf_env_view_set_training",
    "rf_env_view_get_state",
    "rf_env_step_device_view",
    "rf_env_reset_device_view",
    "rf_rollout_advantages",
    "rf_env_configure_view_grouped",
    "rf_env_view_get_statistics_grouped",
    "rf_env_view_set_statistics_grouped",
    "rf_rollout_advantages_grouped",
    "rf_policy_params_size",
    "rf_policy_forward",
    "rf_ppo_state_size",
    "rf_ppo_workspace_size",
    "rf_ppo_update",
    "rf_policy_forward_grouped",
    "rf_ppo_grouped_state_size",
    "rf_ppo_grouped_workspace_size",
    "rf_ppo_update_grouped",
    "rf_sde_params_size",
    "rf_sde_noise_reset",
    "rf_sde_forward",
    "rf_sde_state_size",
    "rf_sde_workspace_size",
    "rf_sde_update",
    "rf_sde_noise_reset_grouped",
    "rf_sde_forward_grouped",
    "rf_sde_grouped_state_size",
    "rf_sde_grouped_workspace_size",
    "rf_sde_update_grouped",
    "rf_lstm_params_size",
    "rf_lstm_state_size",
    "rf_lstm_forward",
    "rf_lstm_ppo_state_size",
    "rf_lstm_ppo_workspace_size",
    "rf_lstm_ppo_update",
    "rf_lstm_sde_params_size",
    "rf_lstm_sde_noise_reset",
    "rf_lstm_sde_forward",
    "rf_lstm_sde_state_size",
    "rf_lstm_sde_workspace_size",
    "rf_lstm_sde_update",
    "rf_lstm_critic_params_size",
    "rf_lstm_critic_forward",
    "rf_lstm_critic_ppo_state_size",
    "rf_lstm_critic_ppo_workspace_size",
    "rf_lstm_critic_ppo_update",
    "rf_lstm_critic_sde_params_size",
    "rf_lstm_critic_sde_noise_reset",
    "rf_lstm_critic_sde_forward",
    "rf_lstm_critic_sde_state_size",
    "rf_lstm_critic_sde_workspace_size",
    "rf_lstm_critic_sde_update",
    "rf_lstm_forward_grouped",
    "rf_lstm_ppo_grouped_state_size",
    "rf_lstm_ppo_grouped_workspace_size",
    "rf_lstm_ppo_update_grouped",
    "rf_lstm_sde_noise_reset_grouped",
    "rf_lstm_sde_forward_grouped",
    "rf_lstm_sde_grouped_state_size",
    "rf_lstm_sde_grouped_workspace_size",
    "rf_lstm_sde_update_grouped",
    "rf_params_init_workspace_size",
    "rf_params_init",
    "rf_eval_accumulate",
    "rf_eval_finish",
    "rf_eval_keep_rows",
    "rf_env_view_get_statistics_device",
    "rf_env_view_set_statistics_device",
    "rf_render_kernel_name",
    "rf_pixels_rendered",
    "rf_allocations_poisoned",
    "rf_general_redo_pixels",
)


class EnvConfig(ctypes.Structure):
    """rf_env_config (include/reinfocus_hip.h)."""

    _fields_ = [
        ("n", ctypes.c_int),
        ("n_actions", ctypes.c_int),
        ("action_set", ctypes.c_double * 32),
        ("limit_lo", ctypes.c_float),
        ("limit_hi", ctypes.c_float),
        ("max_steps", ctypes.c_int),
        ("diverge_threshold", ctypes.c_float),
        ("early_end_steps", ctypes.c_int),
        ("mid", ctypes.c_float * 4),
        ("scale", ctypes.c_float * 4),
        ("reward_scale", ctypes.c_float),
        ("on_target_span", ctypes.c_float),
        ("half_width", ctypes.c_double),
        ("half_height", ctypes.c_double),
        ("tan_half_r", ctypes.c_double),
        ("look_from", ctypes.c_float * 3),
        ("cam_u", ctypes.c_float * 3),
        ("cam_v", ctypes.c_float * 3),
        ("cam_w", ctypes.c_float * 3),
        ("lens_radius", ctypes.c_double),
        ("frame_height", ctypes.c_int),
        ("spp", ctypes.c_int),
        ("gray_mode", ctypes.c_int),
    ]


MAX_LEAVES = 8  # RF_ENV_MAX_LEAVES
MAX_OPS = 2 * MAX_LEAVES - 1  # RF_ENV_MAX_OPS
MAX_STOPPED_STEPS = 31  # RF_ENV_MAX_STOPPED_STEPS


class EnvEnder(ctypes.Structure):
    """rf_env_ender (include/reinfocus_hip.h)."""

    _fields_ = [("kind", ctypes.c_int), ("index0", ctypes.c_int), ("index1", ctypes.c_int), ("steps", ctypes.c_int),
                ("threshold", ctypes.c_double)]


class EnvRewarder(ctypes.Structure):
    """rf_env_rewarder (include/reinfocus_hip.h)."""

    _fields_ = [("kind", ctypes.c_int), ("index0", ctypes.c_int), ("index1", ctypes.c_int), ("p", ctypes.c_double * 3)]


class PolicyDesc(ctypes.Structure):
    """rf_policy_desc (include/reinfocus_hip.h)."""

    _fields_ = [("obs_width", ctypes.c_int), ("n_actions", ctypes.c_int), ("activation", ctypes.c_int),
                ("pi_layers", ctypes.c_int), ("pi_width", ctypes.c_int * 2), ("vf_layers", ctypes.c_int),
                ("vf_width", ctypes.c_int * 2)]

    def __init__(self, obs_width=0, n_actions=0, activation=0, pi_layers=0, pi0=0, pi1=0, vf_layers=0, vf0=0, vf1=0):
        super().__init__(obs_width, n_actions, activation, pi_layers, (ctypes.c_int * 2)(pi0, pi1), vf_layers,
                         (ctypes.c_int * 2)(vf0, vf1))


class LstmPolicyDesc(ctypes.Structure):
    """rf_lstm_policy_desc (include/reinfocus_hip.h): the rf_policy_desc, then lstm_hidden."""

    _fields_ = [("policy", PolicyDesc), ("lstm_hidden", ctypes.c_int)]

    def __init__(self, *desc):
        """The nine integers of rf_policy_desc in order, then lstm_hidden."""
        super().__init__(PolicyDesc(*desc[:9]), *desc[9:])


LSTM_CRITIC_LSTM, LSTM_CRITIC_LINEAR = 0, 1  # RF_LSTM_CRITIC_LSTM, RF_LSTM_CRITIC_LINEAR


class LstmCriticDesc(ctypes.Structure):
    """rf_lstm_critic_desc (include/reinfocus_hip.h, "lstm critic"): the rf_lstm_policy_desc, then critic."""

    _fields_ = [("lstm", LstmPolicyDesc), ("critic", ctypes.c_int)]

    def __init__(self, *desc):
        """The ten integers of rf_lstm_policy_desc in order, then critic (LSTM_CRITIC_LSTM or LSTM_CRITIC_LINEAR)."""
        super().__init__(LstmPolicyDesc(*desc[:10]), *desc[10:])


class PpoDesc(ctypes.Structure):
    """rf_ppo_desc (include/reinfocus_hip.h): the hyper-parameters of one update, by value per call."""

    _fields_ = [("learning_rate", ctypes.c_double), ("clip_range", ctypes.c_double), ("ent_coef", ctypes.c_double),
                ("vf_coef", ctypes.c_double), ("max_grad_norm", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("adam_eps", ctypes.c_double), ("normalize_advantage", ctypes.c_int),
                ("reserved", ctypes.c_int)]


class EnvProgram(ctypes.Structure):
    """rf_env_program (include/reinfocus_hip.h): a composed environment's strategies."""

    _fields_ = [
        ("transformer", ctypes.c_int),
        ("move_index", ctypes.c_int),
        ("n_actions", ctypes.c_int),
        ("action_set", ctypes.c_double * 32),
        ("limit_lo", ctypes.c_double),
        ("limit_hi", ctypes.c_double),
        ("speed", ctypes.c_double),
        ("stop_threshold", ctypes.c_double),
        ("n_enders", ctypes.c_int),
        ("n_ender_ops", ctypes.c_int),
        ("enders", EnvEnder * MAX_LEAVES),
        ("ender_ops", ctypes.c_int * MAX_OPS),
        ("n_rewarders", ctypes.c_int),
        ("n_reward_ops", ctypes.c_int),
        ("rewarders", EnvRewarder * MAX_LEAVES),
        ("reward_ops", ctypes.c_int * MAX_OPS),
        ("reward_f64", ctypes.c_int * MAX_OPS),
    ]


MAX_OBS_NODES = 16  # RF_ENV_MAX_OBS_NODES
MAX_OBS_COLUMNS = 16  # RF_ENV_MAX_OBS_COLUMNS
OBS_INDEXED, OBS_FOCUS, OBS_DELTA, OBS_NORMALIZED = range(4)  # RF_OBS_*


class EnvObserverNode(ctypes.Structure):
    """rf_env_observer_node (include/reinfocus_hip.h)."""

    _fields_ = [("kind", ctypes.c_int), ("index", ctypes.c_int), ("first", ctypes.c_int), ("width", ctypes.c_int),
                ("include_original", ctypes.c_int), ("old_first", ctypes.c_int),
                ("mid", ctypes.c_float * MAX_OBS_COLUMNS), ("scale", ctypes.c_float * MAX_OBS_COLUMNS)]


class EnvObserverProgram(ctypes.Structure):
    """rf_env_observer_program (include/reinfocus_hip.h): a composed environment's observer tree."""

    _fields_ = [("n_nodes", ctypes.c_int), ("width", ctypes.c_int), ("n_old", ctypes.c_int),
                ("nodes", EnvObserverNode * MAX_OBS_NODES)]


MAX_RANGES = 8  # RF_ENV_MAX_RANGES


class EnvInitializerProgram(ctypes.Structure):
    """rf_env_initializer_program (include/reinfocus_hip.h): a RangedInitializer of two elements and its generator."""

    _fields_ = [("counts", ctypes.c_int * 2), ("low", (ctypes.c_double * MAX_RANGES) * 2),
                ("span", (ctypes.c_double * MAX_RANGES) * 2), ("state", ctypes.c_uint64 * 2),
                ("inc", ctypes.c_uint64 * 2)]


class EnvViewConfig(ctypes.Structure):
    """rf_env_view_config (include/reinfocus_hip.h, "learner view"): VecNormalize + VecFrameStack on the device."""

    _fields_ = [("frame_stack", ctypes.c_int32), ("norm_obs", ctypes.c_int32), ("norm_reward", ctypes.c_int32),
                ("training", ctypes.c_int32), ("gamma", ctypes.c_double), ("epsilon", ctypes.c_double),
                ("clip_obs", ctypes.c_double), ("clip_reward", ctypes.c_double)]


def words128(value):
    """(low word, high word) of a 128-bit integer, as the library takes a PCG64DXSM state or increment."""
    assert 0 <= value < 1 << 128, f"{value!r} is not a 128-bit integer"
    return value & (2 ** 64 - 1), value >> 64


class NativeLibraryMissing(ImportError):
    """libreinfocus_hip.so has not been built (python -c 'import __graft_entry__ as g; g.build()')."""


_lib = None


def load():
    """Loads the shared library (once) and declares the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} not found: build it with `make -C reinfocus_amd/csrc` "
            "(or __graft_entry__.build()); reinfocus_amd has no CPU fallback"
        )
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, u64, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_double
    lib.rf_last_error.restype = ctypes.c_char_p
    lib.rf_last_error.argtypes = []
    lib.rf_abi_version.argtypes = []
    lib.rf_device_count.argtypes = [ctypes.POINTER(i32)]
    lib.rf_device_info.argtypes = [i32, ctypes.c_char_p, i32, ctypes.POINTER(i32)]
    lib.rf_create.argtypes = [i32, ctypes.POINTER(vp)]
    lib.rf_destroy.argtypes = [vp]
    lib.rf_seed.argtypes = [vp, u64, u64, u64]
    lib.rf_num_states.argtypes = [vp, ctypes.POINTER(u64)]
    lib.rf_get_states.argtypes = [vp, u64, u64, vp]
    lib.rf_set_states.argtypes = [vp, u64, u64, vp]
    lib.rf_set_scene.argtypes = [vp, i32, vp, vp, vp, vp, vp, dbl]
    lib.rf_render.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.rf_get_frames.argtypes = [vp, i32, i32, vp]
    lib.rf_upload_frames.argtypes = [vp, i32, i32, i32, vp]
    lib.rf_focus.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.rf_step.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    lib.rf_synchronize.argtypes = [vp]
    lib.rf_timing.argtypes = [vp, i32]
    lib.rf_timing_read.argtypes = [vp, ctypes.POINTER(dbl), ctypes.POINTER(u64), ctypes.POINTER(dbl),
                                   ctypes.POINTER(u64)]
    lib.rf_render_general.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp]
    lib.rf_env_configure.argtypes = [vp, ctypes.POINTER(EnvConfig)]
    lib.rf_env_reset.argtypes = [vp, vp, vp]
    lib.rf_env_step.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.POINTER(i32)]
    lib.rf_env_step_begin.argtypes = [vp, vp, vp, vp, ctypes.POINTER(i32)]
    lib.rf_env_step_end.argtypes = [vp, vp, vp]
    lib.rf_env_step_abort.argtypes = [vp]
    lib.rf_env_step_plan.argtypes = [vp, vp, ctypes.POINTER(i32)]
    lib.rf_env_step_run.argtypes = [vp, vp, vp, vp, vp]
    lib.rf_env_render_states.argtypes = [vp, i32, vp, vp]
    lib.rf_env_step_end_given.argtypes = [vp, vp, vp, vp]
    lib.rf_env_get_states.argtypes = [vp, vp]
    lib.rf_env_scene_len.argtypes = [vp, ctypes.POINTER(i32)]
    lib.rf_env_render.argtypes = [vp, i32, i32, vp]
    lib.rf_env_get_counters.argtypes = [vp, vp, vp]
    lib.rf_env_last_step_branch.argtypes = [vp, ctypes.POINTER(i32)]
    lib.rf_env_configure_jumps.argtypes = [vp, ctypes.POINTER(EnvConfig), ctypes.c_float]
    lib.rf_env_step_jumps.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.POINTER(i32)]
    lib.rf_env_step_begin_jumps.argtypes = [vp, vp, vp, vp, ctypes.POINTER(i32)]
    lib.rf_env_step_plan_jumps.argtypes = [vp, vp, ctypes.POINTER(i32)]
    lib.rf_env_configure_composed.argtypes = [vp, ctypes.POINTER(EnvConfig), ctypes.POINTER(EnvProgram)]
    lib.rf_env_get_strategy_state.argtypes = [vp, vp, vp, vp, vp]
    lib.rf_env_configure_observed.argtypes = [vp, ctypes.POINTER(EnvConfig), ctypes.POINTER(EnvProgram),
                                              ctypes.POINTER(EnvObserverProgram)]
    lib.rf_env_get_observer_state.argtypes = [vp, vp]
    lib.rf_env_configure_initializer.argtypes = [vp, ctypes.POINTER(EnvInitializerProgram)]
    lib.rf_env_set_initializer_state.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.rf_env_get_initializer_state.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.rf_env_snapshot_size.argtypes = [vp, ctypes.POINTER(u64)]
    lib.rf_env_snapshot.argtypes = [vp, vp, u64]
    lib.rf_env_restore.argtypes = [vp, vp, u64]
    lib.rf_env_snapshot_resident.argtypes = [vp, i32]
    lib.rf_env_restore_resident.argtypes = [vp, i32]
    lib.rf_env_snapshot_drop.argtypes = [vp, i32]
    lib.rf_env_step_device.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    lib.rf_env_reset_device.argtypes = [vp, vp, vp]
    lib.rf_env_device_status.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.rf_env_configure_records.argtypes = [vp, i32]
    lib.rf_env_get_records.argtypes = [vp, vp, vp, vp]
    lib.rf_env_get_record_accumulators.argtypes = [vp, vp, vp]
    lib.rf_env_step_device_records.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rf_env_configure_view.argtypes = [vp, ctypes.POINTER(EnvViewConfig)]
    lib.rf_env_get_view.argtypes = [vp, vp, vp, vp]
    lib.rf_env_view_get_statistics.argtypes = [vp, vp, vp, vp]
    lib.rf_env_view_set_statistics.argtypes = [vp, vp, vp, vp]
    lib.rf_env_view_set_training.argtypes = [vp, i32]
    lib.rf_env_view_get_state.argtypes = [vp, vp, vp]
    lib.rf_env_step_device_view.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rf_env_reset_device_view.argtypes = [vp, vp, vp, vp]
    lib.rf_rollout_advantages.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, ctypes.c_double, ctypes.c_double, vp, vp, vp]
    lib.rf_env_configure_view_grouped.argtypes = [vp, ctypes.POINTER(EnvViewConfig), i32, vp]
    lib.rf_env_view_get_statistics_grouped.argtypes = [vp, vp, vp, vp]
    lib.rf_env_view_set_statistics_grouped.argtypes = [vp, vp, vp, vp]
    lib.rf_rollout_advantages_grouped.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rf_policy_params_size.restype = ctypes.c_ulonglong
    lib.rf_policy_params_size.argtypes = [vp, vp]
    lib.rf_policy_forward.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.rf_ppo_state_size.restype = ctypes.c_ulonglong
    lib.rf_ppo_state_size.argtypes = [vp, vp]
    lib.rf_ppo_workspace_size.restype = ctypes.c_ulonglong
    lib.rf_ppo_workspace_size.argtypes = [vp, vp, i32]
    lib.rf_ppo_update.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.rf_policy_forward_grouped.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, ctypes.c_ulonglong, i32, vp, vp, vp, vp, vp,
                                              vp]
    lib.rf_ppo_grouped_state_size.restype = ctypes.c_ulonglong
    lib.rf_ppo_grouped_state_size.argtypes = [vp, vp, i32, i32]
    lib.rf_ppo_grouped_workspace_size.restype = ctypes.c_ulonglong
    lib.rf_ppo_grouped_workspace_size.argtypes = [vp, vp, i32, i32, i32, i32]
    lib.rf_ppo_update_grouped.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.rf_sde_params_size.restype = ctypes.c_ulonglong
    lib.rf_sde_params_size.argtypes = [vp, vp]
    lib.rf_sde_noise_reset.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    lib.rf_sde_forward.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rf_sde_state_size.restype = ctypes.c_ulonglong
    lib.rf_sde_state_size.argtypes = [vp, vp]
    lib.rf_sde_workspace_size.restype = ctypes.c_ulonglong
    lib.rf_sde_workspace_size.argtypes = [vp, vp, i32]
    lib.rf_sde_update.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.rf_sde_noise_reset_grouped.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.rf_sde_forward_grouped.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rf_sde_grouped_state_size.restype = ctypes.c_ulonglong
    lib.rf_sde_grouped_state_size.argtypes = [vp, vp, i32, i32]
    lib.rf_sde_grouped_workspace_size.restype = ctypes.c_ulonglong
    lib.rf_sde_grouped_workspace_size.argtypes = [vp, vp, i32, i32, i32, i32]
    lib.rf_sde_update_grouped.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.rf_lstm_params_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_params_size.argtypes = [vp, vp]
    lib.rf_lstm_state_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_state_size.argtypes = [vp, vp, i32]
    lib.rf_lstm_forward.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.rf_lstm_ppo_state_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_ppo_state_size.argtypes = [vp, vp]
    lib.rf_lstm_ppo_workspace_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_ppo_workspace_size.argtypes = [vp, vp, i32]
    lib.rf_lstm_ppo_update.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    lib.rf_lstm_sde_params_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_sde_params_size.argtypes = [vp, vp]
    lib.rf_lstm_sde_noise_reset.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    lib.rf_lstm_sde_forward.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rf_lstm_sde_state_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_sde_state_size.argtypes = [vp, vp]
    lib.rf_lstm_sde_workspace_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_sde_workspace_size.argtypes = [vp, vp, i32]
    lib.rf_lstm_sde_update.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    for head in ("", "sde_"):  # "lstm critic": each sibling has its rf_lstm_ function's arguments over another desc
        for name in ("params_size", "forward") + (("noise_reset",) if head else ()):
            ours, theirs = getattr(lib, f"rf_lstm_critic_{head}{name}"), getattr(lib, f"rf_lstm_{head}{name}")
            ours.restype, ours.argtypes = theirs.restype, theirs.argtypes
        for name in ("state_size", "workspace_size", "update"):
            ours, theirs = getattr(lib, f"rf_lstm_critic_{head or 'ppo_'}{name}"), getattr(lib, f"rf_lstm_{head or 'ppo_'}{name}")
            ours.restype, ours.argtypes = theirs.restype, theirs.argtypes
    lib.rf_lstm_forward_grouped.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.c_ulonglong, i32, vp, vp, vp,
                                            vp, vp, vp]
    lib.rf_lstm_ppo_grouped_state_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_ppo_grouped_state_size.argtypes = [vp, vp, i32, i32]
    lib.rf_lstm_ppo_grouped_workspace_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_ppo_grouped_workspace_size.argtypes = [vp, vp, i32, i32, i32, i32]
    lib.rf_lstm_ppo_update_grouped.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp,
                                               vp]
    lib.rf_lstm_sde_noise_reset_grouped.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.rf_lstm_sde_forward_grouped.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp,
                                                vp]
    lib.rf_lstm_sde_grouped_state_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_sde_grouped_state_size.argtypes = [vp, vp, i32, i32]
    lib.rf_lstm_sde_grouped_workspace_size.restype = ctypes.c_ulonglong
    lib.rf_lstm_sde_grouped_workspace_size.argtypes = [vp, vp, i32, i32, i32, i32]
    lib.rf_lstm_sde_update_grouped.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp,
                                               vp]
    lib.rf_params_init_workspace_size.restype = ctypes.c_ulonglong
    lib.rf_params_init_workspace_size.argtypes = [vp, vp, i32, i32]
    lib.rf_params_init.argtypes = [vp, vp, i32, i32, ctypes.c_uint, vp, vp, vp, vp, vp, vp]
    lib.rf_eval_accumulate.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.rf_eval_finish.argtypes = [vp, i32, i32, i32, i32, ctypes.c_ulonglong, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.rf_eval_keep_rows.argtypes = [vp, i32, ctypes.c_uint, ctypes.c_uint, vp, vp, vp, vp]
    lib.rf_env_view_get_statistics_device.argtypes = [vp, vp, vp]
    lib.rf_env_view_set_statistics_device.argtypes = [vp, vp, vp]
    lib.rf_render_kernel_name.restype = ctypes.c_char_p
    lib.rf_render_kernel_name.argtypes = [vp]
    lib.rf_pixels_rendered.restype = ctypes.c_ulonglong
    lib.rf_pixels_rendered.argtypes = []
    lib.rf_allocations_poisoned.restype = ctypes.c_int
    lib.rf_allocations_poisoned.argtypes = []
    lib.rf_general_redo_pixels.restype = ctypes.c_uint
    lib.rf_general_redo_pixels.argtypes = [vp]
    _lib = lib
    return lib


def _check(rc):
    if rc == RF_OK:
        return
    msg = load().rf_last_error().decode("utf-8", "replace")
    if rc == RF_ERR_INVALID:
        raise AssertionError(msg)
    if rc == RF_ERR_OOM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def device_count():
    n = ctypes.c_int(0)
    _check(load().rf_device_count(ctypes.byref(n)))
    return n.value


def device_info(device):
    """{"device", "pci_bus_id", "numa_node"} of a HIP device index (rf_device_info); numa_node is -1 when the
    host does not say."""
    bus = ctypes.create_string_buffer(32)
    node = ctypes.c_int(-1)
    _check(load().rf_device_info(int(device), bus, 32, ctypes.byref(node)))
    return {"device": int(device), "pci_bus_id": bus.value.decode(), "numa_node": node.value}


def numa_cpus(node, sysfs="/sys/devices/system/node"):
    """CPUs of a NUMA node ("0-15,128-143" in <sysfs>/node<N>/cpulist) as a set; empty if unknown."""
    cpus = set()
    try:
        text = open(os.path.join(sysfs, f"node{int(node)}", "cpulist")).read().strip()
    except (OSError, ValueError):
        return cpus
    for part in filter(None, text.split(",")):
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def pin_to_numa_node(node, whole_process=False, sysfs="/sys/devices/system/node"):
    """Restricts the calling thread (or every thread of the process: the HIP runtime's helper threads exist by the
    time a device can be asked where it sits) to the CPUs of `node` that the process may use at all.  Returns the
    sorted CPU list now in force, or None when nothing was changed (unknown node, no such CPUs, no permission)."""
    if node is None or int(node) < 0 or not hasattr(os, "sched_setaffinity"):
        return None
    allowed = numa_cpus(node, sysfs) & set(os.sched_getaffinity(0))
    if not allowed:
        return None
    try:
        tasks = [int(t) for t in os.listdir("/proc/self/task")] if whole_process else [0]
    except OSError:
        tasks = [0]
    changed = False
    for task in tasks:
        try:
            os.sched_setaffinity(task, allowed)
            changed = True
        except OSError:  # a thread that has ended meanwhile, or no permission
            pass
    return sorted(allowed) if changed else None


def pixels_rendered():
    """Pixels all render launches of this process were made for (rf_pixels_rendered)."""
    return int(load().rf_pixels_rendered())


def allocations_poisoned():
    """True when the library fills its allocations with 0xA5 bytes first (REINFOCUS_POISON_ALLOC; rf_allocations_poisoned)."""
    return bool(load().rf_allocations_poisoned())


def default_device():
    """One process per GPU: torchrun's LOCAL_RANK selects the device."""
    return int(os.environ.get("REINFOCUS_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Context:
    """Owner of one rf_ctx (one renderer's device state on one GPU)."""

    def __init__(self, device=None):
        self._lib = load()
        self._h = ctypes.c_void_p()
        dev = default_device() if device is None else int(device)
        _check(self._lib.rf_create(dev, ctypes.byref(self._h)))
        self.device = dev

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rf_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    # --- RNG ---------------------------------------------------------------------------
    def seed(self, n_states, seed=0, first_state_index=0):
        _check(self._lib.rf_seed(self._h, int(n_states), int(seed), int(first_state_index)))

    def num_states(self):
        n = ctypes.c_uint64(0)
        _check(self._lib.rf_num_states(self._h, ctypes.byref(n)))
        return n.value

    def get_states(self, first=0, count=None):
        count = self.num_states() - first if count is None else count
        out = np.zeros((int(count), 2), dtype=np.uint64)
        _check(self._lib.rf_get_states(self._h, int(first), int(count), _ptr(out)))
        return out

    def set_states(self, states, first=0):
        states = np.ascontiguousarray(states, dtype=np.uint64)
        assert states.ndim == 2 and states.shape[1] == 2
        _check(self._lib.rf_set_states(self._h, int(first), states.shape[0], _ptr(states)))

    # --- scene / render / focus ----------------------------------------------------------
    def set_scene(self, cam_dyn, rect, origin, u, v, lens_radius):
        cam_dyn = np.ascontiguousarray(cam_dyn, dtype=np.float32)
        rect = np.ascontiguousarray(rect, dtype=np.float32)
        n = rect.shape[0]
        assert cam_dyn.shape == (n, 3, 3), "cam_dyn must be float32[n,3,3]"
        assert rect.shape == (n, 2), "rect must be float32[n,2]"
        origin = np.ascontiguousarray(origin, dtype=np.float32)
        u = np.ascontiguousarray(u, dtype=np.float32)
        v = np.ascontiguousarray(v, dtype=np.float32)
        _check(self._lib.rf_set_scene(self._h, n, _ptr(cam_dyn), _ptr(rect), _ptr(origin), _ptr(u), _ptr(v),
                                      float(lens_radius)))

    def render(self, n, h, w, spp, to_host=False):
        out = np.empty((n, h, w, 3), dtype=np.uint8) if to_host else None
        _check(self._lib.rf_render(self._h, n, h, w, spp, _ptr(out) if to_host else None))
        return out

    def get_frames(self, shape, first_env=0, n_envs=None):
        n, h, w = shape[:3]
        n_envs = n - first_env if n_envs is None else n_envs
        out = np.empty((n_envs, h, w, 3), dtype=np.uint8)
        _check(self._lib.rf_get_frames(self._h, first_env, n_envs, _ptr(out)))
        return out

    def upload_frames(self, frames):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        assert frames.ndim == 4 and frames.shape[3] == 3, "frames must be uint8[n,h,w,3]"
        n, h, w = frames.shape[:3]
        _check(self._lib.rf_upload_frames(self._h, n, h, w, _ptr(frames)))

    def focus(self, n, h, w, gray_mode=GRAY_15BIT):
        out = np.empty(n, dtype=np.float64)
        _check(self._lib.rf_focus(self._h, n, h, w, gray_mode, _ptr(out)))
        return out

    def step(self, n, h, w, spp, gray_mode=GRAY_15BIT):
        out = np.empty(n, dtype=np.float64)
        _check(self._lib.rf_step(self._h, n, h, w, spp, gray_mode, _ptr(out)))
        return out

    # --- general renderer ------------------------------------------------------------------
    def render_general(self, cameras, params, types, sizes, h, w, spp, to_host=True):
        """rf_render_general; to_host=False leaves the frames on the device (rf_get_frames fetches them)."""
        cameras = np.ascontiguousarray(cameras, dtype=np.float64)
        params = np.ascontiguousarray(params, dtype=np.float32)
        types = np.ascontiguousarray(types, dtype=np.int32)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        n, most, width = params.shape
        assert cameras.shape == (n, 19) and types.shape == (n, most) and sizes.shape == (n,)
        if width < 7:  # the kernel reads up to 7 parameters per shape
            params = np.ascontiguousarray(np.pad(params, ((0, 0), (0, 0), (0, 7 - width))))
            width = 7
        out = np.empty((n, h, w, 3), dtype=np.uint8) if to_host else None
        _check(self._lib.rf_render_general(self._h, n, h, w, spp, _ptr(cameras), _ptr(params), _ptr(types),
                                           _ptr(sizes), most, width, _ptr(out) if to_host else None))
        return out

    # --- device-resident env step ----------------------------------------------------------
    def _env_configured(self, n, obs_width=4):
        """obs_width: the columns of every observation array the rf_env_* calls fill (float32[n, obs_width]): 4, or the
        width of the observer program the context is configured with."""
        self._env_n = n
        self._env_obs_width = int(obs_width)
        self._env_n_old = 0
        self._env_k = ctypes.c_int(0)  # (env_step's count of ended environments, and its reference, made once)
        self._env_k_ref = ctypes.byref(self._env_k)

    def env_configure(self, cfg):
        self._env_configured(cfg.n)
        _check(self._lib.rf_env_configure(self._h, ctypes.byref(cfg)))

    def env_configure_jumps(self, cfg, stop_threshold):
        """rf_env_configure_jumps: the context steps ContinuousJumps (float32 actions, the env_step*_jumps calls)."""
        self._env_configured(cfg.n)
        _check(self._lib.rf_env_configure_jumps(self._h, ctypes.byref(cfg), float(stop_threshold)))

    def env_configure_composed(self, cfg, program):
        """rf_env_configure_composed: the context steps the composed environment `program` (an EnvProgram; int32
        actions for a discrete transformer, the float32 env_step*_jumps calls for a continuous one)."""
        self._env_configured(cfg.n)
        _check(self._lib.rf_env_configure_composed(self._h, ctypes.byref(cfg), ctypes.byref(program)))
        self._env_program = (program.n_enders, program.n_rewarders,
                             sum(program.enders[i].steps + 1 for i in range(program.n_enders)
                                 if program.enders[i].kind == 3))  # (RF_ENDER_STOPPED)

    def env_configure_observed(self, cfg, program, observer_program):
        """rf_env_configure_observed: env_configure_composed with the observer tree as a program too (an
        EnvObserverProgram); observations are float32[n, observer_program.width] from then on."""
        assert 1 <= observer_program.width <= MAX_OBS_COLUMNS, f"{observer_program.width} observation columns"
        _check(self._lib.rf_env_configure_observed(self._h, ctypes.byref(cfg), ctypes.byref(program),
                                                   ctypes.byref(observer_program)))  # (refused: nothing changes)
        self._env_configured(cfg.n, observer_program.width)
        self._env_n_old = observer_program.n_old
        self._env_program = (program.n_enders, program.n_rewarders,
                             sum(program.enders[i].steps + 1 for i in range(program.n_enders)
                                 if program.enders[i].kind == 3))  # (RF_ENDER_STOPPED)

    def env_observer_state(self):
        """rf_env_get_observer_state: the DELTA nodes' old values, float32[n_old, n], node-major."""
        old = np.empty((self._env_n_old, self._env_n), dtype=np.float32)
        _check(self._lib.rf_env_get_observer_state(self._h, _ptr(old)))
        return old

    def env_configure_initializer(self, program):
        """rf_env_configure_initializer: the context draws its reset states itself from `program` (an
        EnvInitializerProgram) -- env_reset() without states, env_step / env_step_jumps without a pool."""
        _check(self._lib.rf_env_configure_initializer(self._h, ctypes.byref(program)))

    def env_set_initializer_state(self, state, inc):
        """rf_env_set_initializer_state: reseeds the device's generator (128-bit Python ints)."""
        state, inc = (ctypes.c_uint64 * 2)(*words128(state)), (ctypes.c_uint64 * 2)(*words128(inc))
        _check(self._lib.rf_env_set_initializer_state(self._h, state, inc))

    def env_initializer_state(self):
        """rf_env_get_initializer_state: (state, inc) of the device's generator as Python ints."""
        state, inc = (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 2)()
        _check(self._lib.rf_env_get_initializer_state(self._h, state, inc))
        return state[0] | state[1] << 64, inc[0] | inc[1] << 64

    def env_strategy_state(self):
        """rf_env_get_strategy_state: (counters int32[n_enders, n], floats float32[n_enders, n], histories
        float32[rows, n], old values float32[n_rewarders, n])."""
        n_enders, n_rewarders, rows = self._env_program
        n = self._env_n
        counters = np.empty((n_enders, n), dtype=np.int32)
        floats = np.empty((n_enders, n), dtype=np.float32)
        histories = np.empty((rows, n), dtype=np.float32)
        old = np.empty((n_rewarders, n), dtype=np.float32)
        _check(self._lib.rf_env_get_strategy_state(self._h, _ptr(counters), _ptr(floats),
                                                   _ptr(histories) if rows else None, _ptr(old)))
        return counters, floats, histories, old

    # --- snapshots (rf_env_snapshot* / rf_env_restore*) ---------------------------------------
    def env_snapshot_size(self):
        """Bytes of a snapshot of the configured context (rf_env_snapshot_size)."""
        size = ctypes.c_uint64(0)
        _check(self._lib.rf_env_snapshot_size(self._h, ctypes.byref(size)))
        return size.value

    def env_snapshot(self):
        """rf_env_snapshot: everything that decides the environment's future as one uint8 array (the blob of
        include/reinfocus_hip.h: header, state arrays, generator, RNG states)."""
        blob = np.empty(self.env_snapshot_size(), dtype=np.uint8)
        _check(self._lib.rf_env_snapshot(self._h, _ptr(blob), blob.size))
        return blob

    def env_restore(self, blob):
        """rf_env_restore: puts a blob of env_snapshot back, in place; refused (AssertionError, nothing changes) unless
        it was taken under this context's configuration."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
        _check(self._lib.rf_env_restore(self._h, _ptr(blob), blob.size))

    def env_snapshot_resident(self, slot=0):
        """rf_env_snapshot_resident: the same copy into the context's slot in HBM (enqueued, not waited for)."""
        _check(self._lib.rf_env_snapshot_resident(self._h, int(slot)))

    def env_restore_resident(self, slot=0):
        """rf_env_restore_resident: the slot's copy back, in place (enqueued, not waited for)."""
        _check(self._lib.rf_env_restore_resident(self._h, int(slot)))

    def env_snapshot_drop(self, slot=0):
        """rf_env_snapshot_drop: frees the slot's memory."""
        _check(self._lib.rf_env_snapshot_drop(self._h, int(slot)))

    def env_reset(self, states=None):
        """states None: the context's device initializer draws them (env_configure_initializer)."""
        if states is not None:
            states = np.ascontiguousarray(states, dtype=np.float32).reshape(self._env_n, 2)
        obs = np.empty((self._env_n, self._env_obs_width), dtype=np.float32)
        _check(self._lib.rf_env_reset(self._h, None if states is None else _ptr(states), _ptr(obs)))
        return obs

    # --- device io (rf_env_step_device ...): addresses of device memory as plain integers, nothing waited for --------
    def env_step_device(self, actions_ptr, action_dtype, obs_ptr, rewards_ptr, truncated_ptr, n_reset_ptr, stream):
        """rf_env_step_device: one whole step from / to device arrays given by address (ACTION_I32 / _I64 / _F32;
        n_reset_ptr may be None), ordered after and before `stream` (a hipStream_t as an integer).  Only enqueues."""
        rc = self._lib.rf_env_step_device(self._h, actions_ptr, action_dtype, obs_ptr, rewards_ptr, truncated_ptr,
                                          n_reset_ptr, stream)
        if rc != 0:
            _check(rc)

    def env_reset_device(self, obs_ptr, stream):
        """rf_env_reset_device: env_reset() with the observations to a device array.  Only enqueues."""
        _check(self._lib.rf_env_reset_device(self._h, obs_ptr, stream))

    def env_device_status(self):
        """rf_env_device_status: synchronises, settles what device steps left open; None, or (step, env) of the
        earliest invalid action since the last reset."""
        step, env = ctypes.c_int(-1), ctypes.c_int(-1)
        _check(self._lib.rf_env_device_status(self._h, ctypes.byref(step), ctypes.byref(env)))
        return None if step.value < 0 else (step.value, env.value)

    # --- rollout (rf_rollout_advantages): addresses of device memory as plain integers, nothing waited for ------------
    def rollout_advantages(self, steps, num_envs, rewards_ptr, values_ptr, truncated_ptr, final_values_ptr,
                           last_values_ptr, gamma, gae_lambda, advantages_ptr, returns_ptr, stream):
        """rf_rollout_advantages: GAE advantages and returns of [steps][num_envs] device arrays given by address
        (final_values_ptr may be None: no bootstrap), one launch on `stream` (a hipStream_t as an integer).  Only
        enqueues."""
        rc = self._lib.rf_rollout_advantages(self._h, steps, num_envs, rewards_ptr, values_ptr, truncated_ptr,
                                             final_values_ptr, last_values_ptr, gamma, gae_lambda, advantages_ptr,
                                             returns_ptr, stream)
        if rc != 0:
            _check(rc)

    def rollout_advantages_grouped(self, steps, num_envs, groups, rewards_ptr, values_ptr, truncated_ptr, final_values_ptr,
                                   last_values_ptr, discounts_ptr, advantages_ptr, returns_ptr, stream):
        """rf_rollout_advantages_grouped: rollout_advantages with the discounts of `groups` groups of consecutive
        environments, device float32 [groups][2] holding (g, gl), in place of the two scalars.  Only enqueues."""
        rc = self._lib.rf_rollout_advantages_grouped(self._h, steps, num_envs, groups, rewards_ptr, values_ptr,
                                                     truncated_ptr, final_values_ptr, last_values_ptr, discounts_ptr,
                                                     advantages_ptr, returns_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- policy (rf_policy_forward): addresses of device memory as plain integers, nothing waited for -----------------
    def policy_params_size(self, desc):
        """rf_policy_params_size: floats of the packed parameters of `desc` (the nine integers of rf_policy_desc in
        order); 0 for a desc outside the limits."""
        return int(self._lib.rf_policy_params_size(self._h, ctypes.byref(PolicyDesc(*desc))))

    def policy_forward(self, desc, params_ptr, num_envs, obs_ptr, final_obs_ptr, gen, flags, actions_ptr, log_probs_ptr,
                       values_ptr, final_values_ptr, logits_ptr, stream):
        """rf_policy_forward: the actor-critic forward with sampling over device arrays given by address (each output
        and final_obs_ptr may be None), one launch on `stream` (a hipStream_t as an integer).  desc: the nine integers of
        rf_policy_desc in order; gen: the generator's four 64-bit words, or None.  Only enqueues."""
        words = None if gen is None else (ctypes.c_ulonglong * 4)(*gen)
        rc = self._lib.rf_policy_forward(self._h, ctypes.byref(PolicyDesc(*desc)), params_ptr, num_envs, obs_ptr,
                                         final_obs_ptr, words, flags, actions_ptr, log_probs_ptr, values_ptr,
                                         final_values_ptr, logits_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- ppo update (rf_ppo_update): addresses of device memory as plain integers, nothing waited for -----------------
    def ppo_state_size(self, desc):
        """rf_ppo_state_size: bytes of the optimizer state (header, m, v) of the network `desc`; 0 if refused."""
        return int(self._lib.rf_ppo_state_size(self._h, ctypes.byref(PolicyDesc(*desc))))

    def ppo_workspace_size(self, desc, max_batch):
        """rf_ppo_workspace_size: bytes of the workspace for minibatches of up to max_batch samples; 0 if refused."""
        return int(self._lib.rf_ppo_workspace_size(self._h, ctypes.byref(PolicyDesc(*desc)), max_batch))

    def ppo_update(self, desc, hyper, params_ptr, state_ptr, workspace_ptr, rows, obs_ptr, actions_ptr, old_log_probs_ptr,
                   advantages_ptr, returns_ptr, batch, index_ptr, stats_ptr, stream):
        """rf_ppo_update: one PPO minibatch update (loss, backward, clip, Adam) over device arrays given by address,
        three launches on `stream`.  desc: the nine integers of rf_policy_desc; hyper: the nine values of rf_ppo_desc in
        order (learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm, beta1, beta2, adam_eps,
        normalize_advantage).  Only enqueues."""
        rc = self._lib.rf_ppo_update(self._h, ctypes.byref(PolicyDesc(*desc)), ctypes.byref(PpoDesc(*hyper)), params_ptr,
                                     state_ptr, workspace_ptr, rows, obs_ptr, actions_ptr, old_log_probs_ptr,
                                     advantages_ptr, returns_ptr, batch, index_ptr, stats_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- population (rf_*_grouped): the two groups above over G groups of m environments, one launch per stage ----------
    def policy_forward_grouped(self, desc, groups, per_group, params_ptr, obs_ptr, final_obs_ptr, gens_ptr, consumed, flags,
                               actions_ptr, log_probs_ptr, values_ptr, final_values_ptr, logits_ptr, stream):
        """rf_policy_forward_grouped: policy_forward over groups x per_group rows, parameters [groups][P]; gens_ptr: the
        device table uint64 [groups][4] of the generators' words (or None), consumed: the draws each has given so far.
        Only enqueues."""
        rc = self._lib.rf_policy_forward_grouped(self._h, ctypes.byref(PolicyDesc(*desc)), groups, per_group, params_ptr,
                                                 obs_ptr, final_obs_ptr, gens_ptr, consumed, flags, actions_ptr,
                                                 log_probs_ptr, values_ptr, final_values_ptr, logits_ptr, stream)
        if rc != 0:
            _check(rc)

    def ppo_grouped_state_size(self, desc, groups, per_group):
        """rf_ppo_grouped_state_size: bytes of the optimizer states of `groups` networks `desc`; 0 if refused."""
        return int(self._lib.rf_ppo_grouped_state_size(self._h, ctypes.byref(PolicyDesc(*desc)), groups, per_group))

    def ppo_grouped_workspace_size(self, desc, groups, per_group, steps, batch):
        """rf_ppo_grouped_workspace_size: bytes of the workspaces of `groups` minibatches of `batch` samples out of
        per_group x steps rows each; 0 if refused."""
        return int(self._lib.rf_ppo_grouped_workspace_size(self._h, ctypes.byref(PolicyDesc(*desc)), groups, per_group,
                                                           steps, batch))

    def ppo_update_grouped(self, desc, groups, per_group, steps, hyper_ptr, params_ptr, state_ptr, workspace_ptr, obs_ptr,
                           actions_ptr, old_log_probs_ptr, advantages_ptr, returns_ptr, batch, index_ptr, stats_ptr, stream):
        """rf_ppo_update_grouped: ppo_update of `groups` learners at once, three launches on `stream`; every array holds
        the groups' pieces back to back (per_group x steps rows each), hyper_ptr: the device array of rf_ppo_hyper,
        index_ptr: int64 [groups][batch] of rows local to each group.  Only enqueues."""
        rc = self._lib.rf_ppo_update_grouped(self._h, ctypes.byref(PolicyDesc(*desc)), groups, per_group, steps, hyper_ptr,
                                             params_ptr, state_ptr, workspace_ptr, obs_ptr, actions_ptr, old_log_probs_ptr,
                                             advantages_ptr, returns_ptr, batch, index_ptr, stats_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- population sde (rf_sde_*_grouped): the sde policy below over G groups of m environments, one launch per stage ---
    def sde_noise_reset_grouped(self, desc, groups, per_group, params_ptr, gens_ptr, consumed_ptr, select_ptr, theta_ptr,
                                stream):
        """rf_sde_noise_reset_grouped: theta float32 [groups x per_group][L], group g's rows from generator g of the device
        table gens_ptr (uint64 [groups][4]) advanced by consumed_ptr[g] (device uint64 [groups]) and from the log_std of
        params[g]; select_ptr: device uint8 [groups] (0: the group keeps its rows) or None for every group.  Only
        enqueues."""
        rc = self._lib.rf_sde_noise_reset_grouped(self._h, ctypes.byref(PolicyDesc(*desc)), groups, per_group, params_ptr,
                                                  gens_ptr, consumed_ptr, select_ptr, theta_ptr, stream)
        if rc != 0:
            _check(rc)

    def sde_forward_grouped(self, desc, groups, per_group, params_ptr, obs_ptr, final_obs_ptr, theta_ptr, flags, actions_ptr,
                            env_actions_ptr, log_probs_ptr, values_ptr, final_values_ptr, mean_ptr, sigma_ptr, stream):
        """rf_sde_forward_grouped: sde_forward over groups x per_group rows, parameters [groups][P + L].  Only enqueues."""
        rc = self._lib.rf_sde_forward_grouped(self._h, ctypes.byref(PolicyDesc(*desc)), groups, per_group, params_ptr, obs_ptr,
                                              final_obs_ptr, theta_ptr, flags, actions_ptr, env_actions_ptr, log_probs_ptr,
                                              values_ptr, final_values_ptr, mean_ptr, sigma_ptr, stream)
        if rc != 0:
            _check(rc)

    def sde_grouped_state_size(self, desc, groups, per_group):
        """rf_sde_grouped_state_size: bytes of the optimizer states of `groups` sde networks `desc`; 0 if refused."""
        return int(self._lib.rf_sde_grouped_state_size(self._h, ctypes.byref(PolicyDesc(*desc)), groups, per_group))

    def sde_grouped_workspace_size(self, desc, groups, per_group, steps, batch):
        """rf_sde_grouped_workspace_size: as ppo_grouped_workspace_size, over the sde layout; 0 if refused."""
        return int(self._lib.rf_sde_grouped_workspace_size(self._h, ctypes.byref(PolicyDesc(*desc)), groups, per_group,
                                                           steps, batch))

    def sde_update_grouped(self, desc, groups, per_group, steps, hyper_ptr, params_ptr, state_ptr, workspace_ptr, obs_ptr,
                           actions_ptr, old_log_probs_ptr, advantages_ptr, returns_ptr, batch, index_ptr, stats_ptr, stream):
        """rf_sde_update_grouped: ppo_update_grouped with the Gaussian head (actions float32, the raw ones).  Only
        enqueues."""
        rc = self._lib.rf_sde_update_grouped(self._h, ctypes.byref(PolicyDesc(*desc)), groups, per_group, steps, hyper_ptr,
                                             params_ptr, state_ptr, workspace_ptr, obs_ptr, actions_ptr, old_log_probs_ptr,
                                             advantages_ptr, returns_ptr, batch, index_ptr, stats_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- population lstm (rf_lstm_*_grouped): the recurrent policy and update below over G groups of m environments; `desc`
    # is the eleven integers of rf_lstm_critic_desc (either critic) ---------------------------------------------------------
    def lstm_forward_grouped(self, desc, groups, per_group, params_ptr, obs_ptr, episode_starts_ptr, final_obs_ptr,
                             state_in_ptr, state_out_ptr, gens_ptr, consumed, flags, actions_ptr, log_probs_ptr, values_ptr,
                             final_values_ptr, logits_ptr, stream):
        """rf_lstm_forward_grouped: lstm_forward over groups x per_group rows, parameters [groups][P], the state in its single
        form [2][2][groups x per_group][H]; row e of group g takes draw consumed + e of generator g of the device table
        gens_ptr (uint64 [groups][4]; None for a deterministic call).  Only enqueues."""
        rc = self._lib.rf_lstm_forward_grouped(self._h, ctypes.byref(LstmCriticDesc(*desc)), groups, per_group, params_ptr,
                                               obs_ptr, episode_starts_ptr, final_obs_ptr, state_in_ptr, state_out_ptr,
                                               gens_ptr, consumed, flags, actions_ptr, log_probs_ptr, values_ptr,
                                               final_values_ptr, logits_ptr, stream)
        if rc != 0:
            _check(rc)

    def lstm_ppo_grouped_state_size(self, desc, groups, per_group):
        """rf_lstm_ppo_grouped_state_size: bytes of the optimizer states of `groups` recurrent networks; 0 if refused."""
        return int(self._lib.rf_lstm_ppo_grouped_state_size(self._h, ctypes.byref(LstmCriticDesc(*desc)), groups, per_group))

    def lstm_ppo_grouped_workspace_size(self, desc, groups, per_group, steps, batch):
        """rf_lstm_ppo_grouped_workspace_size: bytes of the workspaces of `groups` groups for minibatches of `batch` out of
        per_group x steps rows each; 0 if refused."""
        return int(self._lib.rf_lstm_ppo_grouped_workspace_size(self._h, ctypes.byref(LstmCriticDesc(*desc)), groups,
                                                                per_group, steps, batch))

    def lstm_ppo_update_grouped(self, desc, groups, per_group, steps, hyper_ptr, params_ptr, state_ptr, workspace_ptr,
                                observations_ptr, actions_ptr, log_probs_ptr, advantages_ptr, returns_ptr,
                                episode_starts_ptr, lstm_states_ptr, firsts_ptr, batch, stats_ptr, stream):
        """rf_lstm_ppo_update_grouped: one recurrent minibatch update of every group, six launches on `stream`; group g's
        rows are (firsts[g] + b) mod (per_group x steps), b < batch, of its piece of the flat arrays (firsts_ptr: device
        int32 [groups]), hyper_ptr the device array of `groups` rf_ppo_hyper, stats_ptr float32 [groups][8].  Only enqueues."""
        rc = self._lib.rf_lstm_ppo_update_grouped(self._h, ctypes.byref(LstmCriticDesc(*desc)), groups, per_group, steps,
                                                  hyper_ptr, params_ptr, state_ptr, workspace_ptr, observations_ptr,
                                                  actions_ptr, log_probs_ptr, advantages_ptr, returns_ptr, episode_starts_ptr,
                                                  lstm_states_ptr, firsts_ptr, batch, stats_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- population lstm sde (rf_lstm_sde_*_grouped): the two sections above together -- the recurrent policy with the
    # Gaussian head over G groups; `desc` is the eleven integers of rf_lstm_critic_desc (either critic) ---------------------
    def lstm_sde_noise_reset_grouped(self, desc, groups, per_group, params_ptr, gens_ptr, consumed_ptr, select_ptr, theta_ptr,
                                     stream):
        """rf_lstm_sde_noise_reset_grouped: sde_noise_reset_grouped over the lstm-sde layout's log_std.  Only enqueues."""
        rc = self._lib.rf_lstm_sde_noise_reset_grouped(self._h, ctypes.byref(LstmCriticDesc(*desc)), groups, per_group,
                                                       params_ptr, gens_ptr, consumed_ptr, select_ptr, theta_ptr, stream)
        if rc != 0:
            _check(rc)

    def lstm_sde_forward_grouped(self, desc, groups, per_group, params_ptr, obs_ptr, episode_starts_ptr, final_obs_ptr,
                                 state_in_ptr, state_out_ptr, theta_ptr, flags, actions_ptr, env_actions_ptr, log_probs_ptr,
                                 values_ptr, final_values_ptr, mean_ptr, sigma_ptr, stream):
        """rf_lstm_sde_forward_grouped: lstm_sde_forward over groups x per_group rows, parameters [groups][P + L], theta
        [groups x per_group][L] (None: deterministic), the state in its single form [2][2][groups x per_group][H].  Only
        enqueues."""
        rc = self._lib.rf_lstm_sde_forward_grouped(self._h, ctypes.byref(LstmCriticDesc(*desc)), groups, per_group, params_ptr,
                                                   obs_ptr, episode_starts_ptr, final_obs_ptr, state_in_ptr, state_out_ptr,
                                                   theta_ptr, flags, actions_ptr, env_actions_ptr, log_probs_ptr, values_ptr,
                                                   final_values_ptr, mean_ptr, sigma_ptr, stream)
        if rc != 0:
            _check(rc)

    def lstm_sde_grouped_state_size(self, desc, groups, per_group):
        """rf_lstm_sde_grouped_state_size: bytes of the optimizer states of `groups` lstm-sde networks; 0 if refused."""
        return int(self._lib.rf_lstm_sde_grouped_state_size(self._h, ctypes.byref(LstmCriticDesc(*desc)), groups, per_group))

    def lstm_sde_grouped_workspace_size(self, desc, groups, per_group, steps, batch):
        """rf_lstm_sde_grouped_workspace_size: as lstm_ppo_grouped_workspace_size, over the lstm-sde layout; 0 if refused."""
        return int(self._lib.rf_lstm_sde_grouped_workspace_size(self._h, ctypes.byref(LstmCriticDesc(*desc)), groups,
                                                                per_group, steps, batch))

    def lstm_sde_update_grouped(self, desc, groups, per_group, steps, hyper_ptr, params_ptr, state_ptr, workspace_ptr,
                                observations_ptr, actions_ptr, log_probs_ptr, advantages_ptr, returns_ptr,
                                episode_starts_ptr, lstm_states_ptr, firsts_ptr, batch, stats_ptr, stream):
        """rf_lstm_sde_update_grouped: lstm_ppo_update_grouped with the Gaussian head (actions float32, the raw ones).  Only
        enqueues."""
        rc = self._lib.rf_lstm_sde_update_grouped(self._h, ctypes.byref(LstmCriticDesc(*desc)), groups, per_group, steps,
                                                  hyper_ptr, params_ptr, state_ptr, workspace_ptr, observations_ptr,
                                                  actions_ptr, log_probs_ptr, advantages_ptr, returns_ptr, episode_starts_ptr,
                                                  lstm_states_ptr, firsts_ptr, batch, stats_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- parameter init (rf_params_init*): `segments` is a ctypes array of rf_param_segment (environments/param_init.py) --
    def params_init_workspace_size(self, segments, count, groups):
        """rf_params_init_workspace_size: bytes of the workspace of params_init (0 without orthogonal segments or if refused)."""
        return int(self._lib.rf_params_init_workspace_size(self._h, segments, count, groups))

    def params_init(self, segments, count, groups, stride, params_ptr, gens_ptr, select_ptr, constants_ptr, workspace_ptr,
                    stream):
        """rf_params_init: the packed parameters float32 [groups][stride] initialised from the table, two launches on
        `stream`; gens_ptr device uint64 [groups][4], select_ptr uint8 [groups] or None, constants_ptr float32 [groups] or
        None.  Only enqueues."""
        rc = self._lib.rf_params_init(self._h, segments, count, groups, stride, params_ptr, gens_ptr, select_ptr,
                                      constants_ptr, workspace_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- evaluation (rf_eval_*; environments/evaluation.py): device pointers in, launches on `stream`, nothing waited for ----
    def eval_accumulate(self, n, groups, m, episodes, final_return_ptr, final_length_ptr, counts_ptr, returns_ptr,
                        lengths_ptr, stream):
        """rf_eval_accumulate: the step's episode records into the tables int32 [n], float64 [n][K], int32 [n][K]."""
        rc = self._lib.rf_eval_accumulate(self._h, n, groups, m, episodes, final_return_ptr, final_length_ptr, counts_ptr,
                                          returns_ptr, lengths_ptr, stream)
        if rc != 0:
            _check(rc)

    def eval_finish(self, n, groups, m, episodes, serial, counts_ptr, returns_ptr, lengths_ptr, results_ptr, best_mean_ptr,
                    best_serial_ptr, improved_ptr, stream):
        """rf_eval_finish: the rows float64 [groups][8] and the best rule (float64 [G], int64 [G], uint8 [G])."""
        rc = self._lib.rf_eval_finish(self._h, n, groups, m, episodes, serial, counts_ptr, returns_ptr, lengths_ptr,
                                      results_ptr, best_mean_ptr, best_serial_ptr, improved_ptr, stream)
        if rc != 0:
            _check(rc)

    def eval_keep_rows(self, groups, words, stride, select_ptr, src_ptr, dst_ptr, stream):
        """rf_eval_keep_rows: dst row g := src row g where select[g] != 0; rows of `words` 4-byte words, `stride` apart."""
        rc = self._lib.rf_eval_keep_rows(self._h, groups, words, stride, select_ptr, src_ptr, dst_ptr, stream)
        if rc != 0:
            _check(rc)

    def env_view_statistics_device(self, out_ptr, stream):
        """rf_env_view_get_statistics_device: the view's moments into device float64 [G][3][W + 1] ([3][W + 1] ungrouped)."""
        rc = self._lib.rf_env_view_get_statistics_device(self._h, out_ptr, stream)
        if rc != 0:
            _check(rc)

    def env_view_set_statistics_device(self, in_ptr, stream):
        """rf_env_view_set_statistics_device: the view's moments from device float64 [G][3][W + 1] ([3][W + 1] ungrouped)."""
        rc = self._lib.rf_env_view_set_statistics_device(self._h, in_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- sde policy (rf_sde_*): the Gaussian head's counterparts of the two groups above --------------------------------
    def sde_params_size(self, desc):
        """rf_sde_params_size: floats of the packed parameters (log_std included); 0 for a desc outside the limits."""
        return int(self._lib.rf_sde_params_size(self._h, ctypes.byref(PolicyDesc(*desc))))

    def sde_noise_reset(self, desc, params_ptr, num_envs, gen, theta_ptr, stream):
        """rf_sde_noise_reset: theta float32 [num_envs][L] from the generator's four words and the log_std inside the
        parameters, one launch on `stream`.  Only enqueues."""
        rc = self._lib.rf_sde_noise_reset(self._h, ctypes.byref(PolicyDesc(*desc)), params_ptr, num_envs,
                                          None if gen is None else (ctypes.c_ulonglong * 4)(*gen), theta_ptr, stream)
        if rc != 0:
            _check(rc)

    def sde_forward(self, desc, params_ptr, num_envs, obs_ptr, final_obs_ptr, theta_ptr, flags, actions_ptr,
                    env_actions_ptr, log_probs_ptr, values_ptr, final_values_ptr, mean_ptr, sigma_ptr, stream):
        """rf_sde_forward: the Gaussian actor-critic forward over device arrays given by address (each output,
        final_obs_ptr and theta_ptr may be None), one launch on `stream`.  Only enqueues."""
        rc = self._lib.rf_sde_forward(self._h, ctypes.byref(PolicyDesc(*desc)), params_ptr, num_envs, obs_ptr, final_obs_ptr,
                                      theta_ptr, flags, actions_ptr, env_actions_ptr, log_probs_ptr, values_ptr,
                                      final_values_ptr, mean_ptr, sigma_ptr, stream)
        if rc != 0:
            _check(rc)

    def sde_state_size(self, desc):
        """rf_sde_state_size: bytes of the optimizer state (header, m, v over P + L parameters); 0 if refused."""
        return int(self._lib.rf_sde_state_size(self._h, ctypes.byref(PolicyDesc(*desc))))

    def sde_workspace_size(self, desc, max_batch):
        """rf_sde_workspace_size: bytes of the workspace for minibatches of up to max_batch samples; 0 if refused."""
        return int(self._lib.rf_sde_workspace_size(self._h, ctypes.byref(PolicyDesc(*desc)), max_batch))

    def sde_update(self, desc, hyper, params_ptr, state_ptr, workspace_ptr, rows, obs_ptr, actions_ptr, old_log_probs_ptr,
                   advantages_ptr, returns_ptr, batch, index_ptr, stats_ptr, stream):
        """rf_sde_update: rf_ppo_update with the Gaussian head (actions float32, the raw ones).  Only enqueues."""
        rc = self._lib.rf_sde_update(self._h, ctypes.byref(PolicyDesc(*desc)), ctypes.byref(PpoDesc(*hyper)), params_ptr,
                                     state_ptr, workspace_ptr, rows, obs_ptr, actions_ptr, old_log_probs_ptr,
                                     advantages_ptr, returns_ptr, batch, index_ptr, stats_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- lstm policy (rf_lstm_*): the recurrent actor-critic's forward with its state -----------------------------------
    def lstm_params_size(self, desc):
        """rf_lstm_params_size: floats of the packed parameters of `desc` (the nine integers of rf_policy_desc in order,
        then lstm_hidden); 0 for a desc outside the limits."""
        return int(self._lib.rf_lstm_params_size(self._h, ctypes.byref(LstmPolicyDesc(*desc))))

    def lstm_state_size(self, desc, num_envs):
        """rf_lstm_state_size: floats of the state [2][2][num_envs][lstm_hidden]; 0 if refused."""
        return int(self._lib.rf_lstm_state_size(self._h, ctypes.byref(LstmPolicyDesc(*desc)), num_envs))

    def lstm_forward(self, desc, params_ptr, num_envs, obs_ptr, episode_starts_ptr, final_obs_ptr, state_in_ptr,
                     state_out_ptr, gen, flags, actions_ptr, log_probs_ptr, values_ptr, final_values_ptr, logits_ptr, stream):
        """rf_lstm_forward: the recurrent actor-critic forward over device arrays given by address (final_obs_ptr,
        state_out_ptr and each output may be None), one launch on `stream`.  gen: the generator's four 64-bit words, or
        None.  Only enqueues."""
        words = None if gen is None else (ctypes.c_ulonglong * 4)(*gen)
        rc = self._lib.rf_lstm_forward(self._h, ctypes.byref(LstmPolicyDesc(*desc)), params_ptr, num_envs, obs_ptr,
                                       episode_starts_ptr, final_obs_ptr, state_in_ptr, state_out_ptr, words, flags,
                                       actions_ptr, log_probs_ptr, values_ptr, final_values_ptr, logits_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- lstm update (rf_lstm_ppo_*): the recurrent PPO minibatch update ------------------------------------------------
    def lstm_ppo_state_size(self, desc):
        """rf_lstm_ppo_state_size: bytes of the optimizer state (header, m, v) of the recurrent network `desc`; 0 if
        refused."""
        return int(self._lib.rf_lstm_ppo_state_size(self._h, ctypes.byref(LstmPolicyDesc(*desc))))

    def lstm_ppo_workspace_size(self, desc, max_batch):
        """rf_lstm_ppo_workspace_size: bytes of the workspace for minibatches of up to max_batch rows; 0 if refused."""
        return int(self._lib.rf_lstm_ppo_workspace_size(self._h, ctypes.byref(LstmPolicyDesc(*desc)), max_batch))

    def lstm_ppo_update(self, desc, hyper, params_ptr, state_ptr, workspace_ptr, n_steps, num_envs, obs_ptr, actions_ptr,
                        log_probs_ptr, advantages_ptr, returns_ptr, episode_starts_ptr, lstm_states_ptr, first, batch,
                        stats_ptr, stream):
        """rf_lstm_ppo_update: one recurrent PPO minibatch update (sequences, forward, loss, BPTT, clip, Adam) over rows
        (first + b) mod (n_steps * num_envs), b < batch, of flat()'s arrays and the rollout's episode_starts and
        lstm_states slabs, all device arrays given by address; six launches on `stream`.  desc and hyper as lstm_forward's
        and ppo_update's.  Only enqueues."""
        rc = self._lib.rf_lstm_ppo_update(self._h, ctypes.byref(LstmPolicyDesc(*desc)), ctypes.byref(PpoDesc(*hyper)),
                                          params_ptr, state_ptr, workspace_ptr, n_steps, num_envs, obs_ptr, actions_ptr,
                                          log_probs_ptr, advantages_ptr, returns_ptr, episode_starts_ptr, lstm_states_ptr,
                                          first, batch, stats_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- lstm sde policy and update (rf_lstm_sde_*): the Gaussian head on top of the recurrent actor-critic -------------
    def lstm_sde_params_size(self, desc):
        """rf_lstm_sde_params_size: floats of the packed parameters (log_std included); 0 for a desc outside the limits."""
        return int(self._lib.rf_lstm_sde_params_size(self._h, ctypes.byref(LstmPolicyDesc(*desc))))

    def lstm_sde_noise_reset(self, desc, params_ptr, num_envs, gen, theta_ptr, stream):
        """rf_lstm_sde_noise_reset: theta float32 [num_envs][L] from the generator's four words and the log_std inside the
        parameters; one launch on `stream`.  Only enqueues."""
        rc = self._lib.rf_lstm_sde_noise_reset(self._h, ctypes.byref(LstmPolicyDesc(*desc)), params_ptr, num_envs,
                                               (ctypes.c_ulonglong * 4)(*gen), theta_ptr, stream)
        if rc != 0:
            _check(rc)

    def lstm_sde_forward(self, desc, params_ptr, num_envs, obs_ptr, episode_starts_ptr, final_obs_ptr, state_in_ptr,
                         state_out_ptr, theta_ptr, flags, actions_ptr, env_actions_ptr, log_probs_ptr, values_ptr,
                         final_values_ptr, mean_ptr, sigma_ptr, stream):
        """rf_lstm_sde_forward: lstm_forward with the Gaussian head (theta_ptr in place of gen; final_obs_ptr, state_out_ptr,
        theta_ptr and each output may be None), one launch on `stream`.  Only enqueues."""
        rc = self._lib.rf_lstm_sde_forward(self._h, ctypes.byref(LstmPolicyDesc(*desc)), params_ptr, num_envs, obs_ptr,
                                           episode_starts_ptr, final_obs_ptr, state_in_ptr, state_out_ptr, theta_ptr, flags,
                                           actions_ptr, env_actions_ptr, log_probs_ptr, values_ptr, final_values_ptr,
                                           mean_ptr, sigma_ptr, stream)
        if rc != 0:
            _check(rc)

    def lstm_sde_state_size(self, desc):
        """rf_lstm_sde_state_size: bytes of the optimizer state (header, m, v over P + L parameters); 0 if refused."""
        return int(self._lib.rf_lstm_sde_state_size(self._h, ctypes.byref(LstmPolicyDesc(*desc))))

    def lstm_sde_workspace_size(self, desc, max_batch):
        """rf_lstm_sde_workspace_size: bytes of the workspace for minibatches of up to max_batch rows; 0 if refused."""
        return int(self._lib.rf_lstm_sde_workspace_size(self._h, ctypes.byref(LstmPolicyDesc(*desc)), max_batch))

    def lstm_sde_update(self, desc, hyper, params_ptr, state_ptr, workspace_ptr, n_steps, num_envs, obs_ptr, actions_ptr,
                        log_probs_ptr, advantages_ptr, returns_ptr, episode_starts_ptr, lstm_states_ptr, first, batch,
                        stats_ptr, stream):
        """rf_lstm_sde_update: lstm_ppo_update with the Gaussian head (actions float32, the raw ones).  Only enqueues."""
        rc = self._lib.rf_lstm_sde_update(self._h, ctypes.byref(LstmPolicyDesc(*desc)), ctypes.byref(PpoDesc(*hyper)),
                                          params_ptr, state_ptr, workspace_ptr, n_steps, num_envs, obs_ptr, actions_ptr,
                                          log_probs_ptr, advantages_ptr, returns_ptr, episode_starts_ptr, lstm_states_ptr,
                                          first, batch, stats_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- lstm critic (rf_lstm_critic_*): the recurrent entry points over rf_lstm_critic_desc ----------------------------
    # `desc` is the eleven integers of rf_lstm_critic_desc (rf_lstm_policy_desc's ten, then critic); every other argument
    # is the sibling's.  Only the update and forward calls enqueue.
    def lstm_critic_params_size(self, desc, sde=False):
        """rf_lstm_critic_params_size (rf_lstm_critic_sde_params_size with sde): floats of the packed parameters; 0 if
        refused."""
        call = self._lib.rf_lstm_critic_sde_params_size if sde else self._lib.rf_lstm_critic_params_size
        return int(call(self._h, ctypes.byref(LstmCriticDesc(*desc))))

    def lstm_critic_state_size(self, desc, sde=False):
        """rf_lstm_critic_ppo_state_size / rf_lstm_critic_sde_state_size: bytes of the optimizer state; 0 if refused."""
        call = self._lib.rf_lstm_critic_sde_state_size if sde else self._lib.rf_lstm_critic_ppo_state_size
        return int(call(self._h, ctypes.byref(LstmCriticDesc(*desc))))

    def lstm_critic_workspace_size(self, desc, max_batch, sde=False):
        """rf_lstm_critic_ppo_workspace_size / rf_lstm_critic_sde_workspace_size: bytes of the workspace; 0 if refused."""
        call = self._lib.rf_lstm_critic_sde_workspace_size if sde else self._lib.rf_lstm_critic_ppo_workspace_size
        return int(call(self._h, ctypes.byref(LstmCriticDesc(*desc)), max_batch))

    def lstm_critic_forward(self, desc, params_ptr, num_envs, obs_ptr, episode_starts_ptr, final_obs_ptr, state_in_ptr,
                            state_out_ptr, gen, flags, actions_ptr, log_probs_ptr, values_ptr, final_values_ptr, logits_ptr,
                            stream):
        """rf_lstm_critic_forward: lstm_forward over rf_lstm_critic_desc.  Only enqueues."""
        words = None if gen is None else (ctypes.c_ulonglong * 4)(*gen)
        rc = self._lib.rf_lstm_critic_forward(self._h, ctypes.byref(LstmCriticDesc(*desc)), params_ptr, num_envs, obs_ptr,
                                              episode_starts_ptr, final_obs_ptr, state_in_ptr, state_out_ptr, words, flags,
                                              actions_ptr, log_probs_ptr, values_ptr, final_values_ptr, logits_ptr, stream)
        if rc != 0:
            _check(rc)

    def lstm_critic_ppo_update(self, desc, hyper, params_ptr, state_ptr, workspace_ptr, n_steps, num_envs, obs_ptr,
                               actions_ptr, log_probs_ptr, advantages_ptr, returns_ptr, episode_starts_ptr, lstm_states_ptr,
                               first, batch, stats_ptr, stream, sde=False):
        """rf_lstm_critic_ppo_update (rf_lstm_critic_sde_update with sde: float32 raw actions): lstm_ppo_update /
        lstm_sde_update over rf_lstm_critic_desc.  Only enqueues."""
        call = self._lib.rf_lstm_critic_sde_update if sde else self._lib.rf_lstm_critic_ppo_update
        rc = call(self._h, ctypes.byref(LstmCriticDesc(*desc)), ctypes.byref(PpoDesc(*hyper)), params_ptr, state_ptr,
                  workspace_ptr, n_steps, num_envs, obs_ptr, actions_ptr, log_probs_ptr, advantages_ptr, returns_ptr,
                  episode_starts_ptr, lstm_states_ptr, first, batch, stats_ptr, stream)
        if rc != 0:
            _check(rc)

    def lstm_critic_sde_update(self, *args):
        """rf_lstm_critic_sde_update: lstm_critic_ppo_update with the Gaussian head."""
        self.lstm_critic_ppo_update(*args, sde=True)

    def lstm_critic_sde_noise_reset(self, desc, params_ptr, num_envs, gen, theta_ptr, stream):
        """rf_lstm_critic_sde_noise_reset: lstm_sde_noise_reset over rf_lstm_critic_desc.  Only enqueues."""
        rc = self._lib.rf_lstm_critic_sde_noise_reset(self._h, ctypes.byref(LstmCriticDesc(*desc)), params_ptr, num_envs,
                                                      (ctypes.c_ulonglong * 4)(*gen), theta_ptr, stream)
        if rc != 0:
            _check(rc)

    def lstm_critic_sde_forward(self, desc, params_ptr, num_envs, obs_ptr, episode_starts_ptr, final_obs_ptr, state_in_ptr,
                                state_out_ptr, theta_ptr, flags, actions_ptr, env_actions_ptr, log_probs_ptr, values_ptr,
                                final_values_ptr, mean_ptr, sigma_ptr, stream):
        """rf_lstm_critic_sde_forward: lstm_sde_forward over rf_lstm_critic_desc.  Only enqueues."""
        rc = self._lib.rf_lstm_critic_sde_forward(self._h, ctypes.byref(LstmCriticDesc(*desc)), params_ptr, num_envs, obs_ptr,
                                                  episode_starts_ptr, final_obs_ptr, state_in_ptr, state_out_ptr, theta_ptr,
                                                  flags, actions_ptr, env_actions_ptr, log_probs_ptr, values_ptr,
                                                  final_values_ptr, mean_ptr, sigma_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- episode records (rf_env_configure_records ...) ---------------------------------------------------------
    def env_configure_records(self, on=True):
        """rf_env_configure_records: the context keeps final observations, episode returns and lengths from now on
        (after env_configure*, before the first env_reset)."""
        _check(self._lib.rf_env_configure_records(self._h, 1 if on else 0))

    def env_records(self):
        """rf_env_get_records: the last step's (final_observation float32[n, W], episode_return float64[n],
        episode_length int32[n]) as fresh arrays -- rows of environments that did not end are NaN / NaN / 0."""
        n = self._env_n
        final_obs = np.empty((n, self._env_obs_width), dtype=np.float32)
        returns = np.empty(n, dtype=np.float64)
        lengths = np.empty(n, dtype=np.int32)
        rc = self._lib.rf_env_get_records(self._h, final_obs.ctypes.data, returns.ctypes.data, lengths.ctypes.data)
        if rc != 0:
            _check(rc)
        return final_obs, returns, lengths

    def env_record_accumulators(self):
        """rf_env_get_record_accumulators: the running (returns float64[n], lengths int32[n])."""
        returns = np.empty(self._env_n, dtype=np.float64)
        lengths = np.empty(self._env_n, dtype=np.int32)
        _check(self._lib.rf_env_get_record_accumulators(self._h, _ptr(returns), _ptr(lengths)))
        return returns, lengths

    def env_step_device_records(self, actions_ptr, action_dtype, obs_ptr, rewards_ptr, truncated_ptr, n_reset_ptr,
                                final_obs_ptr, returns_ptr, lengths_ptr, stream):
        """rf_env_step_device_records: env_step_device with the episode records to three more device arrays."""
        rc = self._lib.rf_env_step_device_records(self._h, actions_ptr, action_dtype, obs_ptr, rewards_ptr, truncated_ptr,
                                                  n_reset_ptr, final_obs_ptr, returns_ptr, lengths_ptr, stream)
        if rc != 0:
            _check(rc)

    # --- learner view (rf_env_configure_view ...) ------------------------------------------------------------------
    _env_view_stack = 0  # frame_stack of the configured learner view (0: none)
    _env_view_groups = 0  # G of a grouped learner view (0: none, or ungrouped)

    def env_configure_view(self, config):
        """rf_env_configure_view: an EnvViewConfig -- the context keeps a learner view from now on (after env_configure*
        and env_configure_records, before the first env_reset) --, or None: it stops."""
        _check(self._lib.rf_env_configure_view(self._h, None if config is None else ctypes.byref(config)))
        self._env_view_stack = 0 if config is None else int(config.frame_stack)
        self._env_view_groups = 0

    def env_configure_view_grouped(self, config, groups, gammas=None):
        """rf_env_configure_view_grouped: env_configure_view with `groups` groups of n / groups consecutive environments,
        each with running moments of its own and its own gamma (gammas: `groups` values, or None for config.gamma)."""
        if gammas is not None:
            gammas = np.ascontiguousarray(gammas, dtype=np.float64)
            assert gammas.shape == (groups,), f"gammas of shape {gammas.shape}, not ({groups},)"
        _check(self._lib.rf_env_configure_view_grouped(self._h, ctypes.byref(config), groups,
                                                       None if gammas is None else _ptr(gammas)))
        self._env_view_stack = int(config.frame_stack)
        self._env_view_groups = int(groups)

    def env_view_statistics_grouped(self):
        """rf_env_view_get_statistics_grouped: (mean, var, count), float64[G, W + 1] each, the returns last."""
        arrays = [np.empty((max(self._env_view_groups, 1), self._env_obs_width + 1), dtype=np.float64) for _ in range(3)]
        _check(self._lib.rf_env_view_get_statistics_grouped(self._h, *[_ptr(a) for a in arrays]))
        return tuple(arrays)

    def env_view_set_statistics_grouped(self, mean, var, count):
        """rf_env_view_set_statistics_grouped: float64[G, W + 1] each, the returns last."""
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (mean, var, count)]
        shape = (max(self._env_view_groups, 1), self._env_obs_width + 1)
        for a in arrays:
            assert a.shape == shape, f"statistics of shape {a.shape}, not {shape}"
        _check(self._lib.rf_env_view_set_statistics_grouped(self._h, *[_ptr(a) for a in arrays]))

    def env_view(self, rewards=True, final=False):
        """rf_env_get_view: the view of the last step or reset as fresh arrays -- (obs float32[n, V], rewards float64[n]
        or None, view_final float32[n, V] or None)."""
        n, cells = self._env_n, self._env_obs_width * self._env_view_stack
        obs = np.empty((n, cells), dtype=np.float32)
        view_rewards = np.empty(n, dtype=np.float64) if rewards else None
        view_final = np.empty((n, cells), dtype=np.float32) if final else None
        rc = self._lib.rf_env_get_view(self._h, obs.ctypes.data, view_rewards.ctypes.data if rewards else None,
                                       view_final.ctypes.data if final else None)
        if rc != 0:
            _check(rc)
        return obs, view_rewards, view_final

    def env_view_statistics(self):
        """rf_env_view_get_statistics: (mean, var, count), float64[W + 1] each, the returns last."""
        arrays = [np.empty(self._env_obs_width + 1, dtype=np.float64) for _ in range(3)]
        _check(self._lib.rf_env_view_get_statistics(self._h, *[_ptr(a) for a in arrays]))
        return tuple(arrays)

    def env_view_set_statistics(self, mean, var, count):
        """rf_env_view_set_statistics: float64[W + 1] each, the returns last."""
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (mean, var, count)]
        for a in arrays:
            assert a.shape == (self._env_obs_width + 1,), f"statistics of shape {a.shape}, not ({self._env_obs_width + 1},)"
        _check(self._lib.rf_env_view_set_statistics(self._h, *[_ptr(a) for a in arrays]))

    def env_view_set_training(self, training):
        """rf_env_view_set_training: False freezes the moments and the returns."""
        _check(self._lib.rf_env_view_set_training(self._h, 1 if training else 0))

    def env_view_state(self):
        """rf_env_view_get_state: (stack float32[n, V], returns float64[n])."""
        stack = np.empty((self._env_n, self._env_obs_width * self._env_view_stack), dtype=np.float32)
        returns = np.empty(self._env_n, dtype=np.float64)
        _check(self._lib.rf_env_view_get_state(self._h, _ptr(stack), _ptr(returns)))
        return stack, returns

    def env_step_device_view(self, actions_ptr, action_dtype, obs_ptr, rewards_ptr, truncated_ptr, n_reset_ptr,
                             final_obs_ptr, returns_ptr, lengths_ptr, view_obs_ptr, view_rewards_ptr, view_final_ptr,
                             stream):
        """rf_env_step_device_view: env_step_device_records with the learner view to three more device arrays."""
        rc = self._lib.rf_env_step_device_view(self._h, actions_ptr, action_dtype, obs_ptr, rewards_ptr, truncated_ptr,
                                               n_reset_ptr, final_obs_ptr, returns_ptr, lengths_ptr, view_obs_ptr,
                                               view_rewards_ptr, view_final_ptr, stream)
        if rc != 0:
            _check(rc)

    def env_reset_device_view(self, obs_ptr, view_obs_ptr, stream):
        """rf_env_reset_device_view: env_reset_device with the view observation to a device array.  Only enqueues."""
        _check(self._lib.rf_env_reset_device_view(self._h, obs_ptr, view_obs_ptr, stream))

    # the int32 calls and their float32 (_jumps) twins: one body each, given the C function and the actions' dtype
    def _env_step(self, function, dtype, actions, pool):
        # (addresses as plain integers: the ctypes casts of _ptr cost 2 us each, a sixth of a small environment's step)
        n = self._env_n
        actions = np.ascontiguousarray(actions, dtype=dtype).reshape(n)
        if pool is not None:  # (None: the context's device initializer draws the reset states)
            pool = np.ascontiguousarray(pool, dtype=np.float32).reshape(n, 2)
        obs = np.empty((n, self._env_obs_width), dtype=np.float32)
        rewards = np.empty(n, dtype=np.float64)
        truncated = np.empty(n, dtype=np.bool_)  # (the library writes 0 / 1 bytes)
        k = self._env_k
        rc = function(self._h, actions.ctypes.data, None if pool is None else pool.ctypes.data, obs.ctypes.data,
                      rewards.ctypes.data, truncated.ctypes.data, self._env_k_ref)
        if rc != 0:
            _check(rc)
        return obs, rewards, truncated, k.value

    def _env_step_begin(self, function, dtype, actions):
        n = self._env_n
        actions = np.ascontiguousarray(actions, dtype=dtype).reshape(n)
        rewards = np.empty(n, dtype=np.float64)
        truncated = np.empty(n, dtype=np.uint8)
        k = ctypes.c_int(0)
        _check(function(self._h, _ptr(actions), _ptr(rewards), _ptr(truncated), ctypes.byref(k)))
        return rewards, truncated.astype(bool), k.value

    def _env_step_plan(self, function, dtype, actions):
        actions = np.ascontiguousarray(actions, dtype=dtype).reshape(self._env_n)
        k = ctypes.c_int(0)
        _check(function(self._h, _ptr(actions), ctypes.byref(k)))
        return k.value

    def env_step(self, actions, pool=None):
        """One whole step: (observations, rewards, truncated, number of environments that ended and took rows of
        `pool`; None on a context with a device initializer)."""
        return self._env_step(self._lib.rf_env_step, np.int32, actions, pool)

    def env_step_jumps(self, actions, pool=None):
        """env_step with float32 actions in [-1, 1] (rf_env_step_jumps; anything else is refused by the library)."""
        return self._env_step(self._lib.rf_env_step_jumps, np.float32, actions, pool)

    def env_step_begin(self, actions):
        """First half of a two-phase step: (rewards, truncated, number of environments that ended)."""
        return self._env_step_begin(self._lib.rf_env_step_begin, np.int32, actions)

    def env_step_begin_jumps(self, actions):
        """env_step_begin with float32 actions (rf_env_step_begin_jumps)."""
        return self._env_step_begin(self._lib.rf_env_step_begin_jumps, np.float32, actions)

    def env_step_plan(self, actions):
        """First half of a step cut BEFORE its render (transform, enders, ranking): how many environments end."""
        return self._env_step_plan(self._lib.rf_env_step_plan, np.int32, actions)

    def env_step_plan_jumps(self, actions):
        """env_step_plan with float32 actions (rf_env_step_plan_jumps)."""
        return self._env_step_plan(self._lib.rf_env_step_plan_jumps, np.float32, actions)

    def env_step_end(self, pool_rows):
        """Second half: the environments that ended take pool_rows float32[k, 2]; observations."""
        n = self._env_n
        pool_rows = np.ascontiguousarray(pool_rows, dtype=np.float32).reshape(-1, 2)
        obs = np.empty((n, self._env_obs_width), dtype=np.float32)
        _check(self._lib.rf_env_step_end(self._h, _ptr(pool_rows) if len(pool_rows) else None, _ptr(obs)))
        return obs

    def env_step_run(self, pool_rows):
        """The rest of a planned step with pool_rows float32[k, 2] for the environments that end:
        (observations, rewards, truncated)."""
        n = self._env_n
        pool_rows = np.ascontiguousarray(pool_rows, dtype=np.float32).reshape(-1, 2)
        obs = np.empty((n, self._env_obs_width), dtype=np.float32)
        rewards = np.empty(n, dtype=np.float64)
        truncated = np.empty(n, dtype=np.uint8)
        _check(self._lib.rf_env_step_run(self._h, _ptr(pool_rows) if len(pool_rows) else None, _ptr(obs), _ptr(rewards),
                                         _ptr(truncated)))
        return obs, rewards, truncated.astype(bool)

    def env_render_states(self, states):
        """Exact mode of a sharded environment: float32[k, 2] states rendered and scored as compacted rows
        0..k-1 from this context's RNG state 0; float64[k] focus values."""
        states = np.ascontiguousarray(states, dtype=np.float32).reshape(-1, 2)
        focus = np.empty(len(states), dtype=np.float64)
        _check(self._lib.rf_env_render_states(self._h, len(states), _ptr(states), _ptr(focus)))
        return focus

    def env_step_end_given(self, pool_rows, focus):
        """Second half of a two-phase step whose reset renders happened elsewhere: observations."""
        n = self._env_n
        pool_rows = np.ascontiguousarray(pool_rows, dtype=np.float32).reshape(-1, 2)
        focus = np.ascontiguousarray(focus, dtype=np.float64).reshape(-1)
        assert len(focus) == len(pool_rows)
        obs = np.empty((n, self._env_obs_width), dtype=np.float32)
        some = len(pool_rows) > 0
        _check(self._lib.rf_env_step_end_given(self._h, _ptr(pool_rows) if some else None,
                                               _ptr(focus) if some else None, _ptr(obs)))
        return obs

    def env_step_abort(self):
        """Drops an open two-phase step (another shard failed): env_reset must come next."""
        _check(self._lib.rf_env_step_abort(self._h))

    def env_scene_len(self):
        n = ctypes.c_int(0)
        _check(self._lib.rf_env_scene_len(self._h, ctypes.byref(n)))
        return n.value

    def env_render(self, frame_height, spp):
        """uint8[len, h, h, 3] of the scene set the environment uploaded last."""
        out = np.empty((self.env_scene_len(), frame_height, frame_height, 3), dtype=np.uint8)
        _check(self._lib.rf_env_render(self._h, int(frame_height), int(spp), _ptr(out)))
        return out

    def env_counters(self):
        steps = np.empty(self._env_n, dtype=np.int32)
        diverging = np.empty(self._env_n, dtype=np.int32)
        _check(self._lib.rf_env_get_counters(self._h, _ptr(steps), _ptr(diverging)))
        return steps, diverging

    def env_last_step_branch(self):
        """'none' | 'one-sync' | 'graph' | 'count-sized': how the last rf_env_step was scheduled."""
        branch = ctypes.c_int(0)
        _check(self._lib.rf_env_last_step_branch(self._h, ctypes.byref(branch)))
        return ("none", "one-sync", "graph", "count-sized", "fused", "fused-graph")[branch.value]

    def render_kernel_name(self):
        return self._lib.rf_render_kernel_name(self._h).decode()

    def general_redo_pixels(self):
        """Pixels the last render_general call left to its fix-up kernel (rf_general_redo_pixels)."""
        return int(self._lib.rf_general_redo_pixels(self._h))

    def env_states(self):
        out = np.empty((self._env_n, 2), dtype=np.float32)
        _check(self._lib.rf_env_get_states(self._h, _ptr(out)))
        return out

    def synchronize(self):
        _check(self._lib.rf_synchronize(self._h))

    def timing(self, enable=True):
        _check(self._lib.rf_timing(self._h, 1 if enable else 0))

    def timing_read(self):
        rm, fm = ctypes.c_double(0), ctypes.c_double(0)
        rn, fn = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self._lib.rf_timing_read(self._h, ctypes.byref(rm), ctypes.byref(rn), ctypes.byref(fm),
                                        ctypes.byref(fn)))
        return {"render_ms": rm.value, "render_launches": rn.value, "focus_ms": fm.value,
                "focus_launches": fn.value}
