"""The reference's training wrappers on the device, one HIP launch per step.

The reference trains on ``VecFrameStack(make_vec_env(...), 5)`` (train_test/sb3_train_vec.py:67-70; each
env inside a ``Monitor``) or on ``RecordEpisodeStatistics`` (:43).  ``DeviceWrappers`` is both, behind
``UsvVectorEnv.step`` on the same stream (``usv_wrap_step`` / ``usv_wrap_reset``, include/usv_hip.h)::

    env = gym_usv_amd.make_vec("usv-simple", 65536, copy=False)
    wr = DeviceWrappers(env.num_envs, env.obs_dim, 5, env.device, env.reward.dtype)
    obs, _ = env.reset(seed=0)
    stacked = wr.reset(obs)
    obs, rew, term, trunc, info = env.step(actions)
    stacked, final_stack, episode = wr.step(obs, rew, info["_final_obs"], info["final_obs"])

The stack is a mirrored ring (gym-usv_amd/csrc/usv_wrap_layout.hpp): a step writes the new frame once or
twice and shifts nothing; ``stacked`` is a ``[N, k * D]`` column window of the ring (inner stride 1, row
stride ``ring.stride(0)``), SB3's channels-last ``StackedObservations`` layout without a copy.

Validity: a returned ``stacked`` view is valid until the next ``step`` / ``reset``, which writes into the
same ring (the contract of ``UsvVectorEnv(copy=False)``); ``.clone()`` it to keep it.  ``final_stack`` and
``episode`` are persistent buffers: the rows of the envs done in this step are current, the other rows
keep what an earlier step wrote.  Neither ``reset`` nor ``step`` synchronises with the host.
"""
from __future__ import annotations

import ctypes
import dataclasses

import torch

from . import _lib
from ._lib import ptr as _ptr


@dataclasses.dataclass
class NormalizeConfig:
    """The settings of SB3's ``VecNormalize`` with its defaults (vec_normalize.py ``__init__``)."""
    training: bool = True
    norm_obs: bool = True
    norm_reward: bool = True
    clip_obs: float = 10.0
    clip_reward: float = 10.0
    gamma: float = 0.99
    epsilon: float = 1e-8

    @classmethod
    def of(cls, normalize):
        """From a dict of settings (``{}``: the defaults) or an instance."""
        cfg = dataclasses.replace(normalize) if isinstance(normalize, cls) else None
        if cfg is None:
            if not isinstance(normalize, dict):
                raise TypeError("normalize must be None, a dict of VecNormalize settings or a NormalizeConfig")
            unknown = set(normalize) - {f.name for f in dataclasses.fields(cls)}
            if unknown:
                raise ValueError(f"normalize: unknown settings {sorted(unknown)}")
            cfg = cls(**normalize)
        if not (cfg.clip_obs >= 0 and cfg.clip_reward >= 0):
            raise ValueError("normalize: clip_obs and clip_reward must be >= 0")
        if not 0 <= cfg.gamma <= 1:
            raise ValueError("normalize: gamma must be in [0, 1]")
        if not cfg.epsilon > 0:
            raise ValueError("normalize: epsilon must be > 0")
        return cfg


class DeviceWrappers:
    """``VecFrameStack(n_stack)`` + episode statistics for ``num_envs`` envs of ``obs_dim`` floats.

    ``n_stack=1`` keeps the statistics only (``stacked`` is then the pushed obs).  ``reward_dtype`` is the
    dtype of the rewards ``step`` will be given (float32, or float64 for an f64 env); the episode return
    accumulates in float64 either way.  A done env's older frames become +0.0, as SB3's
    ``stacked_obs[i] = 0`` and ``DeviceFrameStack`` leave them; ``clear_keeps_sign=True`` multiplies them
    by zero instead (-0.0 where a frame was negative), which is what the default path of ``Sb3VecEnv``
    computes with its mask multiply and what its ``fused=True`` mode therefore asks for.

    ``normalize`` (a dict of SB3 ``VecNormalize`` settings, ``{}`` for its defaults, or a
    ``NormalizeConfig``) puts ``VecNormalize`` between the env and the stack,
    ``VecFrameStack(VecNormalize(venv))``: ``stacked`` and ``final_stack`` then hold clipped normalised
    frames, ``norm_rew`` (float32 [N], persistent) the clipped normalised rewards of the last step, and
    the running statistics are the device tensors ``obs_mean`` / ``obs_var`` / ``obs_inv_std`` [D],
    ``obs_count``, ``ret_mean`` / ``ret_var`` / ``ret_inv_std`` / ``ret_count`` [1] and ``returns`` [N],
    all float64, written by the kernels (usv_wrap_step_norm, include/usv_hip.h).  ``training``,
    ``norm_obs`` and ``norm_reward`` may be set at any time and hold from the next call on.  The
    episode statistics keep the raw reward.  The statistics belong to this process: ranks of a
    multi-GPU run each keep their own, nothing is reduced across them."""

    def __init__(self, num_envs, obs_dim, n_stack, device, reward_dtype=torch.float32, lib_path=None,
                 clear_keeps_sign=False, normalize=None):
        self._cfg = NormalizeConfig.of(normalize) if normalize is not None else None
        device = _lib.cuda_device(device, "DeviceWrappers")
        if reward_dtype not in (torch.float32, torch.float64):
            raise ValueError("reward_dtype must be torch.float32 or torch.float64")
        self.lib = _lib.load(lib_path)
        self.n, self.d, self.k = int(num_envs), int(obs_dim), int(n_stack)
        self.device, self.reward_dtype = device, reward_dtype
        self.flags = _lib.WRAP_CLEAR_KEEPS_SIGN if clear_keeps_sign else 0
        stride = self.lib.usv_wrap_ring_stride(self.d, self.k)
        if self.n <= 0 or stride == 0:
            raise ValueError("num_envs and obs_dim must be > 0 and n_stack >= 1")
        kw = dict(device=device)
        n, w = self.n, self.k * self.d
        self.ring = torch.zeros((n, stride), dtype=torch.float32, **kw)
        self.ep_ret = torch.zeros(n, dtype=torch.float64, **kw)
        self.ep_len = torch.zeros(n, dtype=torch.int32, **kw)
        self.episode = torch.zeros((n, 2), dtype=torch.float64, **kw)      # (r, l) rows of done envs
        self.final_stack = torch.zeros((n, w), dtype=torch.float32, **kw)  # terminal stacks of done envs
        self.cum_ret = torch.zeros(n, dtype=torch.float64, **kw)
        self.cum_len = torch.zeros(n, dtype=torch.int64, **kw)
        self.cum_eps = torch.zeros(n, dtype=torch.int64, **kw)
        self._j = 0                                     # step counter: index of the newest frame
        if self._cfg is not None:
            c, f8 = self._cfg, dict(dtype=torch.float64, device=device)
            self.training, self.norm_obs, self.norm_reward = bool(c.training), bool(c.norm_obs), bool(c.norm_reward)
            self.clip_obs, self.clip_reward = float(c.clip_obs), float(c.clip_reward)
            self.gamma, self.epsilon = float(c.gamma), float(c.epsilon)
            # RunningMeanStd.__init__: mean 0, var 1, count 1e-4
            self.obs_mean, self.obs_var = torch.zeros(self.d, **f8), torch.ones(self.d, **f8)
            self.obs_inv_std = (self.obs_var + self.epsilon).rsqrt()
            self.obs_count = torch.full((1,), 1e-4, **f8)
            self.ret_mean, self.ret_var = torch.zeros(1, **f8), torch.ones(1, **f8)
            self.ret_inv_std = (self.ret_var + self.epsilon).rsqrt()
            self.ret_count = torch.full((1,), 1e-4, **f8)
            self.returns = torch.zeros(n, **f8)
            self.norm_rew = torch.zeros(n, dtype=torch.float32, device=device)
            self._scratch = torch.empty(self.lib.usv_norm_scratch_bytes(self.n, self.d) // 8, **f8)
        self._bind()

    def _bind(self):
        """The C struct over the current buffers (again after a buffer was replaced)."""
        rb = 4 if self.reward_dtype == torch.float32 else 8
        self._w = _lib.UsvWrap(self.n, self.d, self.k, rb, self.flags, 0, self.ring.data_ptr(), self.ep_ret.data_ptr(),
                               self.ep_len.data_ptr(), self.episode.data_ptr(), self.cum_ret.data_ptr(),
                               self.cum_len.data_ptr(), self.cum_eps.data_ptr())
        self._wp = ctypes.byref(self._w)
        self._fs_ptr = _ptr(self.final_stack)
        if self._cfg is not None:
            self._z = _lib.UsvNorm(self.n, self.d, 0, 0, self.clip_obs, self.clip_reward, self.gamma, self.epsilon,
                                   *(t.data_ptr() for t in (self.obs_mean, self.obs_var, self.obs_inv_std,
                                                            self.obs_count, self.ret_mean, self.ret_var,
                                                            self.ret_inv_std, self.ret_count, self.returns,
                                                            self._scratch)))
            self._zp = ctypes.byref(self._z)
            self._nr_ptr = _ptr(self.norm_rew)

    def _norm_flags(self):
        """The three switches as they stand now, into the C struct."""
        self._z.flags = (_lib.NORM_TRAINING * bool(self.training) | _lib.NORM_OBS * bool(self.norm_obs) |
                         _lib.NORM_REWARD * bool(self.norm_reward))

    def _check_rows(self, name, t, dtype, shape):
        _lib.check_tensor(name, t, dtype, shape, self.device)

    def _stream(self):
        return _lib.stream_ptr(self.device)

    @property
    def stacked(self):
        """The current stacked observation: a [N, k * D] view of the ring (see the module docstring)."""
        off = self.lib.usv_wrap_window_offset(self.d, self.k, self._j)
        return self.ring[:, off:off + self.k * self.d]

    def reset(self, obs, mask=None):
        """``StackedObservations.reset`` + ``Monitor.reset`` for every env, or for those where ``mask``
        (bool / uint8 [N]); the other envs keep their stacks and counters.  Returns ``stacked``."""
        self._check_rows("obs", obs, torch.float32, (self.n, self.d))
        if mask is not None:
            if mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError("mask must be a bool or uint8 tensor")
            self._check_rows("mask", mask, mask.dtype, (self.n,))
        if self._cfg is not None:
            self._norm_flags()
            rc = self.lib.usv_wrap_reset_norm(self._wp, self._zp, self._j, _ptr(mask), _ptr(obs), self._stream())
        else:
            rc = self.lib.usv_wrap_reset(self._wp, self._j, _ptr(mask), _ptr(obs), self._stream())
        _lib.check(rc, self.lib)
        return self.stacked

    def step(self, obs, rew, done, final_obs=None):
        """Push ``obs`` behind an env step that returned (obs, rew, done = terminated | truncated,
        final_obs = the terminal obs rows of done envs).  Returns ``(stacked, final_stack, episode)``:
        ``final_stack`` [N, k * D] holds SB3's ``terminal_observation`` in the rows of done envs (None
        without ``final_obs``), ``episode`` [N, 2] float64 their (return, length)."""
        n, d = self.n, self.d
        self._check_rows("obs", obs, torch.float32, (n, d))
        self._check_rows("rew", rew, self.reward_dtype, (n,))
        if done.dtype not in (torch.bool, torch.uint8):
            raise ValueError("done must be a bool or uint8 tensor")
        self._check_rows("done", done, done.dtype, (n,))
        if final_obs is not None:
            self._check_rows("final_obs", final_obs, torch.float32, (n, d))
        j = self._j + 1
        fs = self._fs_ptr if final_obs is not None else None
        if self._cfg is not None:
            self._norm_flags()
            rc = self.lib.usv_wrap_step_norm(self._wp, self._zp, j, _ptr(obs), _ptr(rew), _ptr(done), _ptr(final_obs), fs,
                                             self._nr_ptr, self._stream())
        else:
            rc = self.lib.usv_wrap_step(self._wp, j, _ptr(obs), _ptr(rew), _ptr(done), _ptr(final_obs), fs,
                                        self._stream())
        _lib.check(rc, self.lib)
        self._j = j
        return self.stacked, (self.final_stack if final_obs is not None else None), self.episode

    def totals(self):
        """(sum of returns, episodes, sum of lengths) over every episode emitted so far, as Python
        numbers: one reduction and one host copy (the only sync of this class).  The counters are not
        cleared; a caller reporting per interval subtracts its previous totals."""
        t = torch.stack((self.cum_ret.sum(), self.cum_eps.sum().to(torch.float64),
                         self.cum_len.sum().to(torch.float64))).cpu()
        return float(t[0]), int(t[1]), int(t[2])

    # ---- VecNormalize's helpers and its save / load (cold paths: torch ops on the device statistics)
    _STATE = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "returns")

    def _need_norm(self):
        if self._cfg is None:
            raise ValueError("this DeviceWrappers was built without normalize=")

    def _inv(self, var):
        return 1.0 / torch.sqrt(var + self.epsilon)

    def normalize_obs(self, x):
        """``VecNormalize.normalize_obs`` for [.., D] obs, with the kernels' formula:
        float32(clip((float64(x) - mean) * inv_std))."""
        self._need_norm()
        if not self.norm_obs:
            return x
        y = (x.to(torch.float64) - self.obs_mean) * self._inv(self.obs_var)
        return y.clamp(-self.clip_obs, self.clip_obs).to(torch.float32)

    def unnormalize_obs(self, x):
        self._need_norm()
        if not self.norm_obs:
            return x
        return (x.to(torch.float64) / self._inv(self.obs_var) + self.obs_mean).to(torch.float32)

    def normalize_reward(self, r):
        self._need_norm()
        if not self.norm_reward:
            return r
        y = r.to(torch.float64) * self._inv(self.ret_var)
        return y.clamp(-self.clip_reward, self.clip_reward).to(torch.float32)

    def unnormalize_reward(self, r):
        self._need_norm()
        if not self.norm_reward:
            return r
        return (r.to(torch.float64) / self._inv(self.ret_var)).to(torch.float32)

    def state_dict(self):
        """The running statistics as copies (``VecNormalize.save`` without pickle)."""
        self._need_norm()
        return {k: getattr(self, k).clone() for k in self._STATE}

    def load_state_dict(self, state):
        """Statistics of another ``DeviceWrappers`` (``VecNormalize.load``), e.g. training statistics
        into an evaluation env with ``training = False``; ``returns`` is taken when its length fits."""
        self._need_norm()
        for k in self._STATE:
            if k not in state:
                raise KeyError(f"load_state_dict: no {k!r}")
            src, dst = torch.as_tensor(state[k]), getattr(self, k)
            if k == "returns" and src.numel() != dst.numel():
                continue
            if src.numel() != dst.numel():
                raise ValueError(f"load_state_dict: {k} has {src.numel()} values, expected {dst.numel()}")
            dst.copy_(src.reshape(dst.shape).to(dst.dtype))
        self.obs_inv_std.copy_(self._inv(self.obs_var))
        self.ret_inv_std.copy_(self._inv(self.ret_var))
