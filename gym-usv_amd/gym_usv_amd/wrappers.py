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

import torch

from . import _lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class DeviceWrappers:
    """``VecFrameStack(n_stack)`` + episode statistics for ``num_envs`` envs of ``obs_dim`` floats.

    ``n_stack=1`` keeps the statistics only (``stacked`` is then the pushed obs).  ``reward_dtype`` is the
    dtype of the rewards ``step`` will be given (float32, or float64 for an f64 env); the episode return
    accumulates in float64 either way.  A done env's older frames become +0.0, as SB3's
    ``stacked_obs[i] = 0`` and ``DeviceFrameStack`` leave them; ``clear_keeps_sign=True`` multiplies them
    by zero instead (-0.0 where a frame was negative), which is what the default path of ``Sb3VecEnv``
    computes with its mask multiply and what its ``fused=True`` mode therefore asks for."""

    def __init__(self, num_envs, obs_dim, n_stack, device, reward_dtype=torch.float32, lib_path=None,
                 clear_keeps_sign=False):
        device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if device.type != "cuda":
            raise _lib.UsvLibError("DeviceWrappers runs on a ROCm GPU only (no CPU fallback)")
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
        self._bind()

    def _bind(self):
        """The C struct over the current buffers (again after a buffer was replaced)."""
        rb = 4 if self.reward_dtype == torch.float32 else 8
        self._w = _lib.UsvWrap(self.n, self.d, self.k, rb, self.flags, 0, self.ring.data_ptr(), self.ep_ret.data_ptr(),
                               self.ep_len.data_ptr(), self.episode.data_ptr(), self.cum_ret.data_ptr(),
                               self.cum_len.data_ptr(), self.cum_eps.data_ptr())
        self._wp = ctypes.byref(self._w)
        self._fs_ptr = _ptr(self.final_stack)

    def _check_rows(self, name, t, dtype, shape):
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape} on {self.device}")

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

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
        _lib.check(self.lib.usv_wrap_reset(self._wp, self._j, _ptr(mask), _ptr(obs), self._stream()), self.lib)
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
        _lib.check(self.lib.usv_wrap_step(self._wp, j, _ptr(obs), _ptr(rew), _ptr(done), _ptr(final_obs),
                                          self._fs_ptr if final_obs is not None else None, self._stream()),
                   self.lib)
        self._j = j
        return self.stacked, (self.final_stack if final_obs is not None else None), self.episode

    def totals(self):
        """(sum of returns, episodes, sum of lengths) over every episode emitted so far, as Python
        numbers: one reduction and one host copy (the only sync of this class).  The counters are not
        cleared; a caller reporting per interval subtracts its previous totals."""
        t = torch.stack((self.cum_ret.sum(), self.cum_eps.sum().to(torch.float64),
                         self.cum_len.sum().to(torch.float64))).cpu()
        return float(t[0]), int(t[1]), int(t[2])
