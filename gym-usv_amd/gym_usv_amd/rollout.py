"""SB3's ``RolloutBuffer`` on the device, behind ``UsvVectorEnv.step`` and ``DeviceWrappers.step``.

``DeviceRollout`` is ``RolloutBuffer.add`` and ``compute_returns_and_advantage``
(stable_baselines3/common/buffers.py) plus the truncation bootstrap of
``OnPolicyAlgorithm.collect_rollouts`` as HIP kernels (``usv_rollout_*``, include/usv_hip.h) on the
current stream.  A rollout of T steps makes no host sync between its first action and its advantages::

    wr = DeviceWrappers(env.num_envs, env.obs_dim, 5, env.device, env.reward.dtype)
    ro = DeviceRollout(env.num_envs, T, 5 * env.obs_dim, env.act_dim, env.device, env.reward.dtype)
    for t in range(T):
        a, v, logp = policy(wr.stacked)                   # the ring's window, read in place
        ro.put_obs(t, wr.stacked, a, v, logp)             # before the step: the next push overwrites it
        obs, rew, term, trunc, info = env.step(clip(a))
        _, final_stack, _ = wr.step(obs, rew, info["_final_obs"], info["final_obs"])
        ro.put_step(t, rew, term, trunc, final_stack)
    ro.gae(value(wr.stacked), value(ro.term_obs), gamma, gae_lambda)
    ro.adv, ro.ret                                        # [T, N]

All buffer arithmetic is float32 with every operation rounded on its own, as NumPy computes SB3's;
tests/rollout_ref.py restates it and the kernels equal it bit for bit.  ``rew`` keeps the raw reward: the
bootstrapped value enters inside ``gae`` only, so ``gae`` may be called again and gives the same bits.

The other half of ``RolloutBuffer``, ``get``, is one more kernel (``usv_rollout_gather``)::

    for mb in ro.get(batch_size):                         # one device randperm, consecutive slices
        mb.observations, mb.actions, mb.old_values, mb.old_log_prob, mb.advantages, mb.returns
    mb = ro.gather(idx)                                   # any int64 [B] of flat indices t * N + e

``ro.sampler(batch_size, seed)`` is ``get`` without a stored permutation, in the form a HIP graph can replay
(``usv_rollout_gather_perm``)::

    smp = ro.sampler(4096, seed)                          # batch_size must divide T * N
    for _ in range(n_epochs * smp.batches_per_epoch):
        mb = smp.next()                                   # one C call; every epoch visits every sample once

Which minibatch comes next is a two-word cursor in device memory that the call itself advances, and the sample of
each position is a keyed bijection of [0, T * N) computed in the gather kernel from (seed, epoch, position)
(gym-usv_amd/csrc/usv_rollout_perm_math.hpp; tests/rollout_perm_ref.py restates it): no ``randperm``, no index
tensor, and no kernel argument that changes from one minibatch to the next.

``DeviceRollout(..., n_stack=k)`` keeps one ``D``-float frame per (step, env) in ``frames``
[N, T + k - 1, D] where the default keeps the whole ``k * D`` stack in ``obs``; ``gather`` rebuilds the
stacked rows, bit for bit the rows full storage would hold (tests/rollout_frames_ref.py).
"""
from __future__ import annotations

import collections
import ctypes

import torch

from . import _lib
from ._lib import ptr as _ptr


# The fields of SB3's RolloutBufferSamples (common/type_aliases.py), in its order.
RolloutSamples = collections.namedtuple(
    "RolloutSamples", ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns"))


class DeviceRollout:
    """``n_steps`` steps of ``num_envs`` envs whose observations are ``obs_width`` floats (the stacked
    width, ``k * D``) and whose actions are ``act_dim`` floats.

    Buffers (torch tensors on ``device``): ``obs`` [T, N, W], ``act`` [T, N, A], ``rew`` / ``val`` /
    ``logp`` / ``adv`` / ``ret`` [T, N] float32, ``start`` [T + 1, N] uint8 (SB3's ``episode_starts``;
    row 0 starts as ones and ``gae`` carries row T into it for the next rollout), ``term_slot`` [T, N]
    int32 and ``term_obs`` [term_cap, W].

    An env that is truncated and not terminated (the adapter's ``TimeLimit.truncated``) bootstraps: its
    terminal observation goes to ``term_obs[s]``, ``term_slot[t, e] = s``, and ``gae`` adds
    ``gamma * term_val[s]`` to its reward.  Slots count such (t, env) pairs in order from 0 in every
    rollout.  ``term_cap`` defaults to ``2 * num_envs``: envs that were reset together reach the
    TimeLimit in the same step, so ``num_envs`` slots in one step is the normal case.  Overflow: a pair
    whose number is not below ``term_cap`` gets ``term_slot = -1`` and **no bootstrap** (its episode end
    is treated as a termination); ``counts()`` reports how many.

    ``reward_dtype`` is the dtype ``put_step`` will be given (float32: an f32 env or
    ``DeviceWrappers.norm_rew``; float64: an f64 env).  There is no CPU fallback.

    ``n_stack=k`` (frame mode; ``obs_width`` must be ``k * D``): ``obs`` is None and ``frames``
    [N, T + k - 1, D] holds one frame per (step, env): ``put_obs(0, ...)`` stores the whole window,
    ``put_obs(t > 0, ...)`` its newest ``D`` columns, and ``gather`` rebuilds the stacks from ``frames``
    and ``start``.  This needs the windows given to ``put_obs`` to evolve by the ``VecFrameStack`` rule
    between ``put_obs(0)`` and the last ``put_obs`` of a rollout, with exactly the dones given to
    ``put_step``: the fused loop of the module docstring does.  A manual ``wr.reset(obs, mask)`` inside a
    rollout is not supported in frame mode (between rollouts it is).  ``clear_keeps_sign`` must be the
    ``DeviceWrappers``' own setting: a slot behind an episode boundary is +0.0, or ``frame * 0.0``.
    ``term_obs`` stays full width."""

    def __init__(self, num_envs, n_steps, obs_width, act_dim, device, reward_dtype=torch.float32, term_cap=None,
                 lib_path=None, n_stack=None, clear_keeps_sign=False):
        n, T, W, A = int(num_envs), int(n_steps), int(obs_width), int(act_dim)
        if n <= 0 or T <= 0 or W <= 0 or A <= 0:
            raise ValueError("num_envs, n_steps, obs_width and act_dim must be > 0")
        if n_stack is not None:
            n_stack = int(n_stack)
            if not 1 <= n_stack <= 32 or W % n_stack != 0:
                raise ValueError("n_stack must be in [1, 32] and divide obs_width")
        cap = 2 * n if term_cap is None else int(term_cap)
        if cap < 0:
            raise ValueError("term_cap must be >= 0")
        if reward_dtype not in (torch.float32, torch.float64):
            raise ValueError("reward_dtype must be torch.float32 or torch.float64")
        device = _lib.cuda_device(device, "DeviceRollout")
        self.lib = _lib.load(lib_path)
        self.n, self.n_steps, self.w, self.a, self.term_cap = n, T, W, A, cap
        self.device, self.reward_dtype = device, reward_dtype
        f4 = dict(dtype=torch.float32, device=device)
        self.n_stack = n_stack
        self.clear_keeps_sign = bool(clear_keeps_sign)
        if n_stack is None:
            self.obs, self.frames = torch.zeros((T, n, W), **f4), None
        else:
            self.obs, self.frames = None, torch.zeros((n, T + n_stack - 1, W // n_stack), **f4)
        self.act = torch.zeros((T, n, A), **f4)
        self.rew, self.val, self.logp, self.adv, self.ret = (torch.zeros((T, n), **f4) for _ in range(5))
        self.start = torch.zeros((T + 1, n), dtype=torch.uint8, device=device)
        self.start[0] = 1                               # _last_episode_starts = np.ones
        self.term_slot = torch.full((T, n), -1, dtype=torch.int32, device=device)
        self.term_obs = torch.zeros((max(cap, 1), W), **f4)[:cap]
        self._count = torch.zeros(2, dtype=torch.int32, device=device)
        self._scratch = torch.zeros(self.lib.usv_rollout_scratch_bytes(n) // 8, dtype=torch.int64, device=device)
        self._bad = torch.zeros(1, dtype=torch.int32, device=device)
        self._bind()

    def _bind(self):
        """The C struct over the current buffers (again after a buffer was replaced)."""
        # frame mode: put_step and gae refuse a NULL obs and never touch it, so it names the frames
        k = self.n_stack
        self._ro = _lib.UsvRollout(self.n, self.n_steps, self.w, self.a, self.term_cap, 0, *(t.data_ptr() for t in (
            self.obs if k is None else self.frames, self.act, self.rew, self.val, self.logp, self.adv, self.ret,
            self.start, self.term_slot, self.term_obs, self._count, self._scratch)))
        self._rp = ctypes.byref(self._ro)
        flags = _lib.ROLLOUT_FRAMES_CLEAR_KEEPS_SIGN if self.clear_keeps_sign else 0
        self._fr = _lib.UsvRolloutFrames(k or 1, self.w // (k or 1), flags, self.frames.data_ptr() if k else None,
                                         self._bad.data_ptr())
        self._fp = ctypes.byref(self._fr)

    def _check(self, name, t, dtype, shape):
        _lib.check_tensor(name, t, dtype, shape, self.device)

    def _check_t(self, t):
        if not 0 <= int(t) < self.n_steps:
            raise ValueError(f"t must be in [0, {self.n_steps})")
        return int(t)

    def _stream(self):
        return _lib.stream_ptr(self.device)

    def put_obs(self, t, obs, act, val, logp):
        """Row ``t`` of ``obs`` / ``act`` / ``val`` / ``logp``: the observation the action was computed
        from, the unclipped action, V(obs) and the log-probability.  ``obs`` is [N, W] with inner stride 1
        and any row stride >= W (``DeviceWrappers.stacked`` is read in place); call it before the env
        step, whose wrapper push overwrites that window's oldest frame."""
        t = self._check_t(t)
        n, W = self.n, self.w
        if (obs.dtype != torch.float32 or tuple(obs.shape) != (n, W) or obs.device != self.device or
                (W > 1 and obs.stride(1) != 1) or (n > 1 and obs.stride(0) < W)):
            raise ValueError(f"obs must be a float32 tensor of shape {(n, W)} on {self.device} with inner stride 1 "
                             f"and a row stride >= {W}")
        self._check("act", act, torch.float32, (n, self.a))
        self._check("val", val, torch.float32, (n,))
        self._check("logp", logp, torch.float32, (n,))
        stride = obs.stride(0) if n > 1 else W
        if self.n_stack is not None:
            _lib.check(self.lib.usv_rollout_put_obs_frames(self._rp, self._fp, t, _ptr(obs), stride, _ptr(act),
                                                           _ptr(val), _ptr(logp), self._stream()), self.lib)
            return
        _lib.check(self.lib.usv_rollout_put_obs(self._rp, t, _ptr(obs), stride, _ptr(act), _ptr(val), _ptr(logp),
                                                self._stream()), self.lib)

    def put_step(self, t, rew, term, trunc, final_stack):
        """``rew[t]``, ``start[t + 1] = term | trunc`` and the terminal rows of the envs that bootstrap,
        taken from ``final_stack`` [N, W] (``DeviceWrappers.step``'s, or ``info["final_obs"]`` without a
        stack; only rows of done envs are read)."""
        t = self._check_t(t)
        n = self.n
        self._check("rew", rew, self.reward_dtype, (n,))
        for name, m in (("term", term), ("trunc", trunc)):
            if m.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"{name} must be a bool or uint8 tensor")
            self._check(name, m, m.dtype, (n,))
        if final_stack is not None or self.term_cap > 0:
            if final_stack is None:
                raise ValueError("final_stack is needed while term_cap > 0")
            self._check("final_stack", final_stack, torch.float32, (n, self.w))
        _lib.check(self.lib.usv_rollout_put_step(self._rp, t, _ptr(rew), 4 if self.reward_dtype == torch.float32 else 8,
                                                 _ptr(term), _ptr(trunc), _ptr(final_stack), self._stream()), self.lib)

    def gae(self, last_val, term_val, gamma, gae_lambda):
        """``compute_returns_and_advantage`` into ``adv`` / ``ret`` with ``last_val`` [N] = V of the
        observation after the last step and ``term_val`` [term_cap] = V(``term_obs``) (read only at the
        slots in use; None with ``term_cap == 0``).  Returns ``(adv, ret)``."""
        self._check("last_val", last_val, torch.float32, (self.n,))
        if term_val is not None or self.term_cap > 0:
            if term_val is None:
                raise ValueError("term_val is needed while term_cap > 0")
            self._check("term_val", term_val, torch.float32, (self.term_cap,))
        if not (0 <= float(gamma) <= 1 and 0 <= float(gae_lambda) <= 1):
            raise ValueError("gamma and gae_lambda must be in [0, 1]")
        _lib.check(self.lib.usv_rollout_gae(self._rp, _ptr(last_val), _ptr(term_val), float(gamma), float(gae_lambda),
                                            self._stream()), self.lib)
        return self.adv, self.ret

    def counts(self):
        """(terminal rows stored, pairs dropped for lack of a slot) of the current rollout as Python
        ints: one host copy, the only sync of this class."""
        c = self._count.tolist()
        return int(c[0]), int(c[1])

    def gather(self, idx, out=None):
        """SB3's ``RolloutBuffer._get_samples`` in one launch: the samples at the flat indices ``idx``
        (int64 [B] on the device, ``t * N + e``: the ``[T, N] -> [T * N]`` reshape) as a
        ``RolloutSamples`` of ``observations`` [B, W], ``actions`` [B, A] and ``old_values`` /
        ``old_log_prob`` / ``advantages`` / ``returns`` [B].  In frame mode the observations are rebuilt
        from ``frames`` and ``start``; they equal the rows full storage holds bit for bit.  The outputs
        are fresh tensors, or those of ``out`` (a ``RolloutSamples`` of contiguous float32 tensors of
        these shapes).  Runs on the current stream without a host sync.  An index outside [0, T * N) is
        not dereferenced: its outputs are NaN and ``bad_indices()`` counts it."""
        B = int(idx.shape[0]) if idx.dim() == 1 else 0
        if idx.dtype != torch.int64 or not 0 < B < 2 ** 31 or idx.device != self.device:
            raise ValueError(f"idx must be a non-empty 1-D int64 tensor (below 2^31 indices) on {self.device}")
        idx = idx.contiguous()
        out = self._out(B, out)
        _lib.check(self.lib.usv_rollout_gather(self._rp, self._fp, _ptr(idx), B, *(_ptr(t) for t in out),
                                               self._stream()), self.lib)
        return out

    def _out(self, B, out):
        """``gather``'s outputs for ``B`` samples: fresh tensors, or those of ``out`` checked."""
        shapes = ((B, self.w), (B, self.a), (B,), (B,), (B,), (B,))
        if out is None:
            return RolloutSamples(*(torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes))
        for name, t, s in zip(RolloutSamples._fields, out, shapes):
            self._check(f"out.{name}", t, torch.float32, s)
        return out if isinstance(out, RolloutSamples) else RolloutSamples(*out)

    def sampler(self, batch_size, seed=0):
        """A ``RolloutSampler`` over this rollout: minibatches of ``batch_size`` (it must divide ``T * N``:
        ``ValueError``) in the order that ``seed`` (a 64-bit integer) keys."""
        return RolloutSampler(self, batch_size, seed)

    def get(self, batch_size, generator=None):
        """SB3's ``RolloutBuffer.get``: one ``torch.randperm(T * N)`` on the device (``generator``: a
        device generator), then ``gather`` of consecutive slices of ``batch_size`` indices; the last
        slice may be shorter.  Call it after ``gae``."""
        batch_size = int(batch_size)
        if batch_size <= 0:
            raise ValueError("batch_size must be > 0")
        M = self.n_steps * self.n
        perm = torch.randperm(M, device=self.device, generator=generator)
        for s in range(0, M, batch_size):
            yield self.gather(perm[s:s + batch_size])

    def bad_indices(self):
        """How many indices ``gather`` has refused since this object was built, as a Python int (one
        host copy: a sync, like ``counts``)."""
        return int(self._bad.item())


class RolloutSampler:
    """SB3's ``RolloutBuffer.get`` as a sequence of ``next()`` calls that a HIP graph can replay.

    Epoch ``e`` visits the samples in the order ``perm_index(seed, e, T * N, 0 .. T * N - 1)``, a keyed bijection
    that the gather kernel evaluates itself; minibatch ``b`` of an epoch is positions ``b * batch_size ..``.  The
    cursor ``(epoch, batch)`` lives in a 16-byte device block that every ``next()`` advances on the device, so a
    recorded ``next()`` reads another minibatch at every replay, and ``n_epochs * batches_per_epoch`` calls are
    ``n_epochs`` passes over the rollout.  The sampler reads the rollout as it is when ``next()`` runs: one sampler
    serves every update.

    Reading ``epoch`` or ``batch`` copies the word to the host, **a host sync**; setting either is an ordinary
    stream-ordered write (a ``RuntimeError`` while capturing: the write would be recorded, not made).  Partial last
    minibatches are not supported: ``DeviceRollout.get`` keeps them."""

    def __init__(self, rollout, batch_size, seed=0):
        B, M = int(batch_size), rollout.n_steps * rollout.n
        if B <= 0 or B >= 2 ** 31 or M % B != 0:
            raise ValueError(f"batch_size must be in [1, 2^31) and divide n_steps * num_envs = {M}: a recorded "
                             f"minibatch has one shape")
        if M // B >= 2 ** 32:
            raise ValueError("more than 2^32 - 1 minibatches an epoch")
        self.rollout, self.batch_size, self.batches_per_epoch = rollout, B, M // B
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.lib, self.device = rollout.lib, rollout.device
        words = (int(self.lib.usv_rollout_cursor_bytes()) + 3) // 4
        self._cursor = torch.zeros(words, dtype=torch.int32, device=self.device)    # epoch, batch, reserved

    def _write(self, k, value, who):
        from .optim import refuse_capture
        refuse_capture(f"RolloutSampler.{who} was set", "set it between replays, outside the captured region")
        _lib.word_write(self._cursor[k:k + 1], value)

    @property
    def epoch(self):
        """The epoch of the next minibatch, a uint32 that wraps.  Reading it is a host sync."""
        return _lib.word_read(self._cursor[0:1])

    @epoch.setter
    def epoch(self, value):
        self._write(0, value, "epoch")

    @property
    def batch(self):
        """The number of the next minibatch within its epoch.  Reading it is a host sync."""
        return _lib.word_read(self._cursor[1:2])

    @batch.setter
    def batch(self, value):
        if not 0 <= int(value) < self.batches_per_epoch:
            raise ValueError(f"batch must be in [0, {self.batches_per_epoch})")
        self._write(1, value, "batch")

    def next(self, out=None, idx_out=None):
        """The next minibatch as a ``RolloutSamples``, then the cursor moves on: one C call, two launches on the
        current stream, no host sync, legal under capture.  ``out`` as ``DeviceRollout.gather``'s; ``idx_out``
        (contiguous int64 [batch_size] on the device) receives the flat indices ``t * N + e`` of the samples."""
        ro, B = self.rollout, self.batch_size
        if idx_out is not None:
            ro._check("idx_out", idx_out, torch.int64, (B,))
        out = ro._out(B, out)
        _lib.check(self.lib.usv_rollout_gather_perm(ro._rp, ro._fp, _ptr(self._cursor), self.seed, B, _ptr(idx_out),
                                                    *(_ptr(t) for t in out), ro._stream()), self.lib)
        return out

    def state_dict(self):
        """``{"seed", "epoch", "batch"}`` as Python ints (a host sync): what a checkpoint needs to go on with the
        same sequence."""
        e, b = (int(x) & 0xFFFFFFFF for x in self._cursor[:2].tolist())
        return {"seed": self.seed, "epoch": e, "batch": b}

    def load_state_dict(self, sd):
        seed, batch = int(sd["seed"]) & 0xFFFFFFFFFFFFFFFF, int(sd["batch"])
        if not 0 <= batch < self.batches_per_epoch:
            raise ValueError(f"batch must be in [0, {self.batches_per_epoch})")
        self.epoch, self.batch, self.seed = int(sd["epoch"]), batch, seed
