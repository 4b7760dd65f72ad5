"""ctypes binding of libusvhip.so (C-ABI declared in include/usv_hip.h).

The library is built in-tree (``__graft_entry__.build()`` / ``python -m gym_usv_amd.build``)
and loaded from this package directory.  There is no fallback: if the HIP library is missing
or fails to load, every env constructor raises ``UsvLibError``.
"""
from __future__ import annotations

import ctypes
import os

LIB_NAME = "libusvhip.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)
# diagnostic builds (tools/) may point at another in-tree copy of the library
LIB_PATH = os.environ.get("USV_LIB_PATH", LIB_PATH)

ABI_VERSION = 5
MODE_SIMPLE, MODE_ASMC_SIMPLE, MODE_ASMC_V0, MODE_ASMC_YE_INT_V0, MODE_PID_V0 = 0, 1, 2, 3, 4
F32, F64 = 0, 1
AUTORESET_SAME_STEP, AUTORESET_DISABLED = 0, 1
LIDAR_BRUTE, LIDAR_WINDOW = 0, 1
RESET_PHILOX, RESET_NUMPY_PCG64 = 0, 1
OBS_DIM, SENSOR_COUNT, ACT_DIM, ASMC_STATE = 143, 128, 2, 16
FLAG_PERTURB = 1
FLAG_IGNORE_OBSTACLES = 2
# usv_info_key order (include/usv_hip.h): reference info keys (simple_env.py:102-115, 189-199) -> column
INFO_KEYS = ("x", "y", "psi", "u", "v", "r", "path_x0", "path_y0", "path_x1", "path_y1", "action0",
             "action1", "ye", "angle_to_target", "ye_reward", "angle_to_target_reward",
             "delta_action_reward", "delta_action", "velocity_track_reward", "reference_velocity",
             "reward_velocity", "reference_velocity_error")
INFO_DIM = len(INFO_KEYS)
EXP_MAX_OBS = 64


class UsvLibError(RuntimeError):
    pass


class UsvConfig(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("precision", ctypes.c_int32), ("num_envs", ctypes.c_int32),
                ("obstacle_cap", ctypes.c_int32), ("max_episode_steps", ctypes.c_int32),
                ("autoreset", ctypes.c_int32), ("lidar_algo", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("env_id_offset", ctypes.c_uint64),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class UsvResetOptions(ctypes.Structure):
    _fields_ = [("place_obstacles_on_path", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class UsvExperiment(ctypes.Structure):
    _fields_ = [("n_obs", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("obstacle_x", ctypes.c_double * EXP_MAX_OBS), ("obstacle_y", ctypes.c_double * EXP_MAX_OBS),
                ("obstacle_r", ctypes.c_double * EXP_MAX_OBS), ("path_start", ctypes.c_double * 2),
                ("angle", ctypes.c_double), ("position", ctypes.c_double * 3)]


WRAP_CLEAR_KEEPS_SIGN = 1


class UsvWrap(ctypes.Structure):
    """usv_wrap: the caller-owned device buffers of the fused wrappers (usv_wrap_step / usv_wrap_reset)."""
    _fields_ = [("n", ctypes.c_int32), ("obs_dim", ctypes.c_int32), ("n_stack", ctypes.c_int32),
                ("reward_bytes", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("ring", ctypes.c_void_p), ("ep_ret", ctypes.c_void_p),
                ("ep_len", ctypes.c_void_p), ("episode", ctypes.c_void_p), ("cum_ret", ctypes.c_void_p),
                ("cum_len", ctypes.c_void_p), ("cum_eps", ctypes.c_void_p)]


NORM_TRAINING, NORM_OBS, NORM_REWARD = 1, 2, 4


class UsvNorm(ctypes.Structure):
    """usv_norm: the caller-owned statistics of the fused VecNormalize (usv_wrap_step_norm / _reset_norm)."""
    _fields_ = [("n", ctypes.c_int32), ("obs_dim", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("clip_obs", ctypes.c_double), ("clip_reward", ctypes.c_double),
                ("gamma", ctypes.c_double), ("epsilon", ctypes.c_double),
                ("obs_mean", ctypes.c_void_p), ("obs_var", ctypes.c_void_p), ("obs_inv_std", ctypes.c_void_p),
                ("obs_count", ctypes.c_void_p), ("ret_mean", ctypes.c_void_p), ("ret_var", ctypes.c_void_p),
                ("ret_inv_std", ctypes.c_void_p), ("ret_count", ctypes.c_void_p), ("returns", ctypes.c_void_p),
                ("scratch", ctypes.c_void_p)]


class UsvRollout(ctypes.Structure):
    """usv_rollout: the caller-owned device buffers of the rollout buffer (usv_rollout_put_obs / _put_step / _gae)."""
    _fields_ = [("n", ctypes.c_int32), ("n_steps", ctypes.c_int32), ("obs_width", ctypes.c_int32),
                ("act_dim", ctypes.c_int32), ("term_cap", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("obs", ctypes.c_void_p), ("act", ctypes.c_void_p), ("rew", ctypes.c_void_p),
                ("val", ctypes.c_void_p), ("logp", ctypes.c_void_p), ("adv", ctypes.c_void_p),
                ("ret", ctypes.c_void_p), ("start", ctypes.c_void_p), ("term_slot", ctypes.c_void_p),
                ("term_obs", ctypes.c_void_p), ("term_count", ctypes.c_void_p), ("scratch", ctypes.c_void_p)]


ROLLOUT_FRAMES_CLEAR_KEEPS_SIGN = 1


class UsvRolloutFrames(ctypes.Structure):
    """usv_rollout_frames: the frame-deduplicated obs storage of a rollout and the gather's counter
    (usv_rollout_put_obs_frames / usv_rollout_gather)."""
    _fields_ = [("k", ctypes.c_int32), ("d", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("frames", ctypes.c_void_p), ("bad_count", ctypes.c_void_p)]


class UsvSde(ctypes.Structure):
    """usv_sde: shape, generator key and Box bounds of the fused gSDE head (usv_sde_sample / usv_sde_weights /
    usv_sde_squash_forward / _backward / usv_sde_eval_forward / _backward)."""
    _fields_ = [("n", ctypes.c_int32), ("latent_dim", ctypes.c_int32), ("act_dim", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64), ("gid0", ctypes.c_uint64),
                ("low", ctypes.c_float * 4), ("high", ctypes.c_float * 4)]


REPLAY_CLEAR_KEEPS_SIGN = 1


class UsvReplay(ctypes.Structure):
    """usv_replay: the caller-owned device buffers of the replay buffer (usv_replay_put_obs / _put_step / _gather)."""
    _fields_ = [("n", ctypes.c_int32), ("rows", ctypes.c_int32), ("obs_width", ctypes.c_int32),
                ("act_dim", ctypes.c_int32), ("k", ctypes.c_int32), ("d", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("frames", ctypes.c_void_p), ("next_frame", ctypes.c_void_p),
                ("act", ctypes.c_void_p), ("rew", ctypes.c_void_p), ("done", ctypes.c_void_p),
                ("timeout", ctypes.c_void_p), ("age", ctypes.c_void_p), ("age_now", ctypes.c_void_p),
                ("bad_count", ctypes.c_void_p)]


class UsvPolyakPair(ctypes.Structure):
    """usv_polyak_pair: one (parameters, target parameters) tensor pair of usv_polyak_update."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("numel", ctypes.c_int64)]


class UsvAdamTensor(ctypes.Structure):
    """usv_adam_tensor: one (parameter, gradient) tensor of usv_adam_step."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("numel", ctypes.c_int64)]


# (name, restype, argtypes) for every function in include/usv_hip.h
_vp, _i32, _u64, _sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_size_t
_i64, _u32, _f32 = ctypes.c_int64, ctypes.c_uint32, ctypes.c_float
SIGNATURES = [
    ("usv_abi_version", ctypes.c_int, []),
    ("usv_last_error", ctypes.c_char_p, []),
    ("usv_config_default", None, [ctypes.POINTER(UsvConfig), _i32, _i32]),
    ("usv_create", ctypes.c_int, [ctypes.POINTER(UsvConfig), _i32, ctypes.POINTER(_vp)]),
    ("usv_destroy", None, [_vp]),
    ("usv_num_envs", ctypes.c_int, [_vp]),
    ("usv_obs_dim", ctypes.c_int, [_vp]),
    ("usv_act_dim", ctypes.c_int, [_vp]),
    ("usv_reward_bytes", ctypes.c_int, [_vp]),
    ("usv_seed", ctypes.c_int, [_vp, _u64]),
    ("usv_set_reset_rng", ctypes.c_int, [_vp, _i32]),
    ("usv_reset", ctypes.c_int, [_vp, _vp, _vp, _vp]),
    ("usv_reset_ex", ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(UsvResetOptions), _vp, _vp]),
    ("usv_set_experiment", ctypes.c_int, [_vp, ctypes.POINTER(UsvExperiment)]),
    ("usv_step", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("usv_step_ex", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("usv_field_info", ctypes.c_int, [_vp, _i32, ctypes.POINTER(_i32), ctypes.POINTER(_i32),
                                      ctypes.POINTER(ctypes.c_char_p)]),
    ("usv_get_field", ctypes.c_int, [_vp, _i32, _vp, _sz]),
    ("usv_set_field", ctypes.c_int, [_vp, _i32, _vp, _sz]),
    ("usv_state_bytes", _sz, [_vp]),
    ("usv_get_state", ctypes.c_int, [_vp, _vp, _sz]),
    ("usv_set_state", ctypes.c_int, [_vp, _vp, _sz]),
    ("usv_set_kernel_variant", ctypes.c_int, [_vp, _i32, _i32, _i32]),
    ("usv_set_ignore_obstacles", ctypes.c_int, [_vp, _i32]),
    ("usv_get_ignore_obstacles", ctypes.c_int, [_vp]),
    ("usv_config_size", _sz, []),
    ("usv_asmc_compute", ctypes.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    ("usv_wrap_ring_stride", _sz, [_i32, _i32]),
    ("usv_wrap_window_offset", _sz, [_i32, _i32, _i64]),
    ("usv_wrap_reset", ctypes.c_int, [ctypes.POINTER(UsvWrap), _i64, _vp, _vp, _vp]),
    ("usv_wrap_step", ctypes.c_int, [ctypes.POINTER(UsvWrap), _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("usv_norm_scratch_bytes", _sz, [_i32, _i32]),
    ("usv_wrap_step_norm", ctypes.c_int, [ctypes.POINTER(UsvWrap), ctypes.POINTER(UsvNorm), _i64, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp]),
    ("usv_wrap_reset_norm", ctypes.c_int, [ctypes.POINTER(UsvWrap), ctypes.POINTER(UsvNorm), _i64, _vp, _vp, _vp]),
    ("usv_rollout_scratch_bytes", _sz, [_i32]),
    ("usv_rollout_put_obs", ctypes.c_int, [ctypes.POINTER(UsvRollout), _i32, _vp, _sz, _vp, _vp, _vp, _vp]),
    ("usv_rollout_put_step", ctypes.c_int, [ctypes.POINTER(UsvRollout), _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    ("usv_rollout_gae", ctypes.c_int, [ctypes.POINTER(UsvRollout), _vp, _vp, ctypes.c_double, ctypes.c_double, _vp]),
    ("usv_rollout_put_obs_frames", ctypes.c_int, [ctypes.POINTER(UsvRollout), ctypes.POINTER(UsvRolloutFrames), _i32,
                                                  _vp, _sz, _vp, _vp, _vp, _vp]),
    ("usv_rollout_gather", ctypes.c_int, [ctypes.POINTER(UsvRollout), ctypes.POINTER(UsvRolloutFrames), _vp, _i32, _vp,
                                          _vp, _vp, _vp, _vp, _vp, _vp]),
    ("usv_sde_sample", ctypes.c_int, [ctypes.POINTER(UsvSde), _u32, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    ("usv_sde_weights", ctypes.c_int, [ctypes.POINTER(UsvSde), _u32, _vp, _vp, _vp]),
    ("usv_sde_squash_forward", ctypes.c_int, [ctypes.POINTER(UsvSde), _u32, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp,
                                              _vp]),
    ("usv_sde_squash_scratch_floats", _sz, [ctypes.POINTER(UsvSde)]),
    ("usv_sde_squash_backward", ctypes.c_int, [ctypes.POINTER(UsvSde), _u32, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _vp, _sz, _vp, _vp, _vp]),
    ("usv_sde_eval_forward", ctypes.c_int, [ctypes.POINTER(UsvSde), _i32, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _f32, _vp,
                                            _vp, _vp, _vp, _vp]),
    ("usv_sde_eval_scratch_floats", _sz, [ctypes.POINTER(UsvSde), _i32]),
    ("usv_sde_eval_backward", ctypes.c_int, [ctypes.POINTER(UsvSde), _i32, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _f32,
                                             _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("usv_replay_put_obs", ctypes.c_int, [ctypes.POINTER(UsvReplay), _i64, _vp, _sz, _vp, _vp]),
    ("usv_replay_put_step", ctypes.c_int, [ctypes.POINTER(UsvReplay), _i64, _vp, _i32, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("usv_replay_gather", ctypes.c_int, [ctypes.POINTER(UsvReplay), _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("usv_replay_gather_nstep", ctypes.c_int, [ctypes.POINTER(UsvReplay), _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp,
                                               _vp, _vp, _vp]),
    ("usv_sac_scratch_floats", _sz, [_i32]),
    ("usv_sac_critic_loss", ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp,
                                           _vp, _vp]),
    ("usv_sac_policy_loss", ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("usv_sac_loss_backward", ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("usv_polyak_table_bytes", _sz, [ctypes.POINTER(UsvPolyakPair), _i32]),
    ("usv_polyak_update", ctypes.c_int, [ctypes.POINTER(UsvPolyakPair), _i32, _vp, _sz, _i32, ctypes.c_double, _vp]),
    ("usv_caps_perturb", ctypes.c_int, [_i32, _i32, _vp, _vp, _f32, _u64, _u32, _vp]),
    ("usv_caps_loss", ctypes.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("usv_adam_state_floats", _sz, [ctypes.POINTER(UsvAdamTensor), _i32]),
    ("usv_adam_scratch_floats", _sz, [ctypes.POINTER(UsvAdamTensor), _i32]),
    ("usv_adam_step", ctypes.c_int, [ctypes.POINTER(UsvAdamTensor), _i32, _vp, _vp, _sz, _i64, ctypes.c_double,
                                     ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _vp, _sz, _vp,
                                     _vp]),
    ("usv_ppo_scratch_floats", _sz, [_i32]),
    ("usv_ppo_loss", ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _f32, _f32, _f32, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp]),
    ("usv_ppo_explained_variance", ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp]),
    ("usv_counter_add", ctypes.c_int, [_vp, _u32, _vp]),
    ("usv_sde_sample_dev", ctypes.c_int, [ctypes.POINTER(UsvSde), _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    ("usv_sde_weights_dev", ctypes.c_int, [ctypes.POINTER(UsvSde), _vp, _vp, _vp, _vp]),
    ("usv_sde_squash_forward_dev", ctypes.c_int, [ctypes.POINTER(UsvSde), _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp,
                                                  _vp, _vp]),
    ("usv_sde_squash_backward_dev", ctypes.c_int, [ctypes.POINTER(UsvSde), _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp,
                                                   _vp, _vp, _sz, _vp, _vp, _vp]),
    ("usv_caps_perturb_dev", ctypes.c_int, [_i32, _i32, _vp, _vp, _f32, _u64, _vp, _vp]),
    ("usv_adam_clock_bytes", _sz, []),
    ("usv_adam_step_dev", ctypes.c_int, [ctypes.POINTER(UsvAdamTensor), _i32, _vp, _vp, _sz, _vp, _sz, ctypes.c_double,
                                         ctypes.c_double, ctypes.c_double, ctypes.c_double, _vp, _sz, _vp, _vp]),
    ("usv_polyak_prepare", ctypes.c_int, [ctypes.POINTER(UsvPolyakPair), _i32, _vp, _sz]),
    ("usv_rollout_cursor_bytes", _sz, []),
    ("usv_rollout_gather_perm", ctypes.c_int, [ctypes.POINTER(UsvRollout), ctypes.POINTER(UsvRolloutFrames), _vp, _u64,
                                               _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
]

_LIBS = {}


def load(path=None):
    """Load (once per path) and return the HIP library; raise UsvLibError if it is unavailable.
    ``path`` selects another build of the same C-ABI (e.g. libusvhip_safe.so); each path is its
    own ctypes handle (RTLD_LOCAL), so two builds can be used side by side."""
    path = path or LIB_PATH
    if path in _LIBS:
        return _LIBS[path]
    if not os.path.exists(path):
        raise UsvLibError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise UsvLibError(f"cannot load {path}: {e}") from e
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.usv_abi_version() != ABI_VERSION:
        raise UsvLibError("libusvhip ABI version mismatch")
    if lib.usv_config_size() != ctypes.sizeof(UsvConfig):
        raise UsvLibError(f"usv_config is {lib.usv_config_size()} B in the library, "
                          f"{ctypes.sizeof(UsvConfig)} B in this binding")
    _LIBS[path] = lib
    return lib


SAFE_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libusvhip_safe.so")


def check(rc, lib=None):
    if rc != 0:
        msg = (lib or load()).usv_last_error().decode(errors="replace")
        raise UsvLibError(f"libusvhip error {rc}: {msg}")
    return rc


# ---- what the classes over device tensors share (torch is theirs to import: this module stays ctypes-only)
def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream_ptr(device):
    """The current stream of ``device`` as the ``void* stream`` of the C entries."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def word_read(word):
    """The uint32 a one-element int32 device tensor holds (a capturable object's noise epoch): a host sync."""
    return int(word.item()) & 0xFFFFFFFF


def word_write(word, value):
    """``value`` mod 2^32 into the one-element int32 device tensor ``word``: a stream-ordered write."""
    value = int(value) & 0xFFFFFFFF
    word.fill_(value - (1 << 32) if value >= 1 << 31 else value)


def cuda_device(device, who):
    """``device`` (a torch.device, a string or a GPU index) as a torch.device; ``who`` has no CPU fallback."""
    import torch
    device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    if device.type != "cuda":
        raise UsvLibError(f"{who} runs on a ROCm GPU only (no CPU fallback)")
    return device


def check_rows(name, t, dtype, shape, device, stride_multiple=1, align=1):
    """A 2-D tensor read row by row in place: inner stride 1, a row stride >= the row length that is a
    multiple of ``stride_multiple`` elements, and a base aligned to ``align`` bytes.  Returns the row stride
    in elements; a single row has no stride of its own and reports its length."""
    n, w = shape
    stride = t.stride(0) if t.dim() == 2 and n > 1 else w
    if (t.dim() != 2 or t.dtype != dtype or tuple(t.shape) != shape or t.device != device or t.stride(1) != 1 or
            stride < w or stride % stride_multiple != 0 or t.data_ptr() % align != 0):
        raise ValueError(f"{name} must be a {dtype} tensor of shape {shape} on {device} with inner stride 1, a row "
                         f"stride >= {w} that is a multiple of {stride_multiple}, and a {align}-B aligned base")
    return stride


def check_tensor(name, t, dtype, shape, device):
    if t.dtype != dtype or tuple(t.shape) != shape or t.device != device or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape} on {device}")
