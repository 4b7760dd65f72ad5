"""SB3's ``StateDependentNoiseDistribution`` at rollout time as one HIP launch per step.

``DeviceSDE`` is gSDE's ``sample_weights`` / ``get_noise`` / ``log_prob`` (stable_baselines3/common/
distributions.py; ``full_std``, no ``use_expln``, latent not learned through the noise) behind
``usv_sde_sample`` (include/usv_hip.h), on the current stream and without a host sync::

    head = DeviceSDE(env.num_envs, 256, env.act_dim, env.device, seed + 1, low, high)
    for t in range(T):
        if t % sde_sample_freq == 0:
            head.reset_noise()                            # a host integer: no device work
        lat = policy.pi_body(obs)                         # [N, 256], the ReLU body's output
        a, a_env, logp = head.sample(policy.mu(lat), lat, policy.log_std.exp())
        ro.put_obs(t, obs, a, value, logp)                # the unclipped action and its log-probability
        env.step(a_env)                                   # clipped to the Box

The per-env exploration matrix ``W`` [N, L, A] of the torch formulation (2 KiB per env at L = 256, A = 2)
is never allocated: element (j, k) of env e is ``std[j, k]`` times a normal that is a pure function of
(seed, global env id, epoch, j * A + k) through Philox4x32-10 and Box-Muller, rebuilt in registers by the
launch that uses it.  ``reset_noise`` only increments ``epoch``.  ``weights(std)`` writes the matrix out for
inspection, tests and checkpoints; a one-hot latent row makes ``sample`` return a row of it bit for bit.

The arithmetic is float32 in the order gym-usv_amd/csrc/usv_sde_math.hpp fixes; tests/sde_ref.py restates
it in float64.  The update-time ``log_prob`` and its gradient stay torch autograd: they never needed W.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import ptr as _ptr

MAX_LATENT = 4096


class DeviceSDE:
    """The gSDE head of ``num_envs`` envs with ``latent_dim`` latents (a multiple of 4 in [4, 4096]) and
    ``act_dim`` (1 or 2) actions clipped to the Box ``[low, high]``.

    ``seed``: the key of the noise generator.  **Pass a seed different from the env's**: the in-kernel
    resets draw from the same Philox keyed by the env's seed with counter (global env id, episode, draw),
    so the same key would correlate reset draws with W.  ``env_id_offset`` is the global id of env 0: a
    shard ``DeviceSDE(4, ..., env_id_offset=4)`` computes rows 4..7 of the 8-env head's outputs.

    ``epoch`` (readable and settable, a uint32 that wraps): the noise epoch; save and restore it with a
    checkpoint and the noise continues where it was.  It starts at 0; ``reset_noise()`` increments it.

    ``copy=False`` (default): ``sample`` returns this object's persistent buffers, overwritten by the next
    ``sample`` (stream-ordered: consume them on the same stream first, as ``DeviceRollout.put_obs`` and
    ``env.step`` do).  ``copy=True`` returns fresh tensors.  There is no CPU fallback."""

    def __init__(self, num_envs, latent_dim, act_dim, device, seed, low, high, env_id_offset=0, copy=False,
                 lib_path=None):
        n, L, A = int(num_envs), int(latent_dim), int(act_dim)
        if n <= 0:
            raise ValueError("num_envs must be > 0")
        if A not in (1, 2):
            raise ValueError("act_dim must be 1 or 2")
        if not 4 <= L <= MAX_LATENT or L % 4 != 0:
            raise ValueError(f"latent_dim must be a multiple of 4 in [4, {MAX_LATENT}]")
        lo = [float(x) for x in torch.as_tensor(low, dtype=torch.float32).flatten().tolist()]
        hi = [float(x) for x in torch.as_tensor(high, dtype=torch.float32).flatten().tolist()]
        if len(lo) != A or len(hi) != A or not all(a <= b for a, b in zip(lo, hi)):
            raise ValueError(f"low and high must hold {A} values with low <= high")
        seed, gid0 = int(seed), int(env_id_offset)
        if not 0 <= seed < 2 ** 64 or not 0 <= gid0 < 2 ** 64:
            raise ValueError("seed and env_id_offset must be in [0, 2^64)")
        device = _lib.cuda_device(device, "DeviceSDE")
        self.lib = _lib.load(lib_path)
        self.n, self.latent_dim, self.act_dim = n, L, A
        self.device, self.seed, self.env_id_offset, self.copy = device, seed, gid0, bool(copy)
        self.low = torch.tensor(lo, dtype=torch.float32, device=device)
        self.high = torch.tensor(hi, dtype=torch.float32, device=device)
        self._epoch = 0
        self._s = _lib.UsvSde(n, L, A, 0, seed, gid0, (ctypes.c_float * 4)(*lo), (ctypes.c_float * 4)(*hi))
        self._sp = ctypes.byref(self._s)
        f4 = dict(dtype=torch.float32, device=device)
        self._out = (torch.zeros((n, A), **f4), torch.zeros((n, A), **f4), torch.zeros((n,), **f4))

    @property
    def epoch(self):
        return self._epoch

    @epoch.setter
    def epoch(self, v):
        self._epoch = int(v) & 0xFFFFFFFF

    def reset_noise(self):
        """SB3's ``reset_noise`` / ``sample_weights``: a new matrix for every env from the next ``sample``
        on.  A host integer; nothing runs on the device."""
        self.epoch = self._epoch + 1

    def sample(self, mean, latent, std, out=None):
        """``(a, a_env, logp)`` in one launch: ``a = mean + latent @ W`` [N, A] (unclipped, the rollout
        buffer's), ``a_env = max(min(a, high), low)`` [N, A] and
        ``logp = Normal(mean, sqrt(latent^2 @ std^2 + 1e-6)).log_prob(a).sum(-1)`` [N].

        ``mean`` [N, A] and ``std`` [L, A] (``log_std.exp()``) are contiguous float32; ``latent`` is
        float32 [N, L] with inner stride 1, a row stride that is a multiple of 4 and >= L, and a 16-B
        aligned base.  ``out``: three contiguous float32 tensors of those shapes to write instead."""
        n, L, A = self.n, self.latent_dim, self.act_dim
        _lib.check_tensor("mean", mean, torch.float32, (n, A), self.device)
        _lib.check_tensor("std", std, torch.float32, (L, A), self.device)
        # a single env's row has no stride of its own: the kernel is then given L
        stride = _lib.check_rows("latent", latent, torch.float32, (n, L), self.device, stride_multiple=4, align=16)
        if out is None:
            out = self._out
        else:
            for name, t, s in zip(("out[0]", "out[1]", "out[2]"), out, ((n, A), (n, A), (n,))):
                _lib.check_tensor(name, t, torch.float32, s, self.device)
        a, a_env, logp = out
        _lib.check(self.lib.usv_sde_sample(self._sp, self._epoch, _ptr(mean), _ptr(latent), stride, _ptr(std), _ptr(a),
                                           _ptr(a_env), _ptr(logp), _lib.stream_ptr(self.device)), self.lib)
        if self.copy and out is self._out:
            return a.clone(), a_env.clone(), logp.clone()
        return a, a_env, logp

    def weights(self, std, out=None):
        """SB3's ``exploration_mat`` of the current epoch for every env, [N, L, A]: a fresh tensor, or
        ``out``.  Off the hot path (``sample`` does not read it)."""
        n, L, A = self.n, self.latent_dim, self.act_dim
        _lib.check_tensor("std", std, torch.float32, (L, A), self.device)
        if out is None:
            out = torch.empty((n, L, A), dtype=torch.float32, device=self.device)
        else:
            _lib.check_tensor("out", out, torch.float32, (n, L, A), self.device)
        _lib.check(self.lib.usv_sde_weights(self._sp, self._epoch, _ptr(std), _ptr(out),
                                            _lib.stream_ptr(self.device)), self.lib)
        return out
