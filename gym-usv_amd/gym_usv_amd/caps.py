"""The CAPS smoothness regulariser for SAC's actor: *Conditioning for Action Policy Smoothness* (Mysore et al.,
"Regularizing Action Policies for Smooth Control with Reinforcement Learning", ICRA 2021), the ``lambda_t``,
``lambda_s`` and ``eps_s`` keys of the reference's ``config_sac`` (train_test/config.py:34-36).

With pi the actor's deterministic action (``tanh(mean)`` for a squashed policy, ``mean`` otherwise)::

    L_T = mean_i ||pi(s_i) - pi(s'_i)||_2          s' the next observation
    L_S = mean_i ||pi(s_i) - pi(s~_i)||_2          s~ = s + eps_s * z,  z ~ N(0, I)
    actor_loss + lambda_t * L_T + lambda_s * L_S

``DeviceCAPS`` is both pieces behind ``usv_caps_perturb`` / ``usv_caps_loss`` (include/usv_hip.h)::

    caps = DeviceCAPS(device, seed, lambda_t=10.0, lambda_s=5.0, eps_s=0.1, squash=True)
    caps.reset_noise()                          # once per gradient step
    near = caps.near(mb.observations)           # one launch, no noise tensor in memory
    m, m2, m3 = actor_mean(obs), actor_mean(mb.next_observations), actor_mean(near)    # pre-squash, [B, A]
    s = caps.loss(m, m2, m3)                    # SmoothLoss(loss, temporal, spatial), one launch
    (pl.actor_loss + s.loss).backward()         # one launch for the three gradients

The noise is counter-based: element ``j`` of row ``r`` is a function of (seed, r, epoch, j) through Philox4x32-10 and
Box-Muller (gym-usv_amd/csrc/usv_caps_math.hpp; tests/caps_ref.py restates it), so a row's noise does not depend on
the batch size.  The sums over the batch are taken in ``DeviceSACLoss``'s fixed order: the loss and its gradients are
bitwise reproducible.  All on the current stream, without a host sync.
"""
from __future__ import annotations

import collections
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .optim import refuse_capture

SmoothLoss = collections.namedtuple("SmoothLoss", "loss temporal spatial")
MAX_ACT_DIM = 8


def check_weight(name, v):
    """``v`` as a float that is finite and >= 0."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number") from None
    if not math.isfinite(f) or f < 0.0:
        raise ValueError(f"{name} must be finite and >= 0")
    return f


def check_means(mean, mean_next, mean_near, device):
    """The three [B, A] float32 means of ``DeviceCAPS.loss`` on ``device``, contiguous; returns (B, A)."""
    for name, t in (("mean", mean), ("mean_next", mean_next), ("mean_near", mean_near)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1:
            raise ValueError(f"{name} must be a float32 tensor of shape [B, A]")
        if t.shape != mean.shape:
            raise ValueError(f"{name} must have mean's shape {tuple(mean.shape)}")
        if t.device != device:
            raise ValueError(f"{name} must be on {device}")
    B, A = mean.shape
    if not 1 <= A <= MAX_ACT_DIM:
        raise ValueError(f"the action dimension must be in [1, {MAX_ACT_DIM}]")
    if B * A > 2 ** 31 - 1:
        raise ValueError("B * A must be below 2^31")
    return B, A


class _Smooth(torch.autograd.Function):
    """``DeviceCAPS.loss`` under autograd: the unit gradients saved, the backward is ``usv_sac_loss_backward``."""

    @staticmethod
    def forward(ctx, obj, mean, mean_next, mean_near):
        n = mean.numel()
        g = obj._fresh(3 * n)                               # g_mean, g_next, g_near [B, A] each
        at = g.data_ptr()
        out = obj._loss(mean, mean_next, mean_near, at, at + 4 * n, at + 8 * n)
        ctx.obj, ctx.shape = obj, mean.shape
        ctx.save_for_backward(g)
        ctx.mark_non_differentiable(out[1], out[2])
        ctx.set_materialize_grads(False)                    # an unused loss: its gradient stays None, zeros out
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, g_temporal, g_spatial):
        g, = ctx.saved_tensors
        n, at = g.numel() // 3, g.data_ptr()
        need = ctx.needs_input_grad[1:]
        if g_loss is None:
            return None, None, None, None
        o = [ctx.obj._fresh(ctx.shape) for _ in range(3)]
        up = g_loss if g_loss.dtype is torch.float32 else g_loss.float()
        _lib.check(ctx.obj.lib.usv_sac_loss_backward(n, up.data_ptr(), at, at + 4 * n, at + 8 * n, o[0].data_ptr(),
                                                     o[1].data_ptr(), o[2].data_ptr(), None, None, None,
                                                     _lib.stream_ptr(ctx.obj.device)), ctx.obj.lib)
        return (None,) + tuple(x if w else None for x, w in zip(o, need))


class DeviceCAPS:
    """CAPS on ``device`` (a ROCm GPU; there is no CPU fallback).  ``seed``: the key of the noise generator, in
    [0, 2^64); pass one different from the env's and from the gSDE heads'.  ``lambda_t``, ``lambda_s``, ``eps_s``:
    finite and >= 0 (``eps_s`` is a standard deviation).  ``squash``: pi = tanh(mean).  ``epoch`` (readable and
    settable, a uint32 that wraps): the noise epoch; save and restore it with a checkpoint.  The object owns a small
    scratch buffer that grows with the batch: calls of one object must be stream-ordered.

    ``capturable=True``: the epoch is a word in device memory that ``near``'s kernel reads (``usv_caps_perturb_dev``),
    so ``near`` is legal inside ``torch.cuda.graph`` and a replay draws the noise of the epoch the word then holds.
    ``reset_noise()`` is one launch of one thread (``usv_counter_add``), to be captured with the rest; setting ``epoch``
    is a stream-ordered write and reading it is **a host sync**.  In the default form ``near`` raises ``RuntimeError``
    while the stream is capturing: a graph would freeze its epoch.  ``loss`` draws no noise and is capturable in
    both forms, once a warm-up call has grown the scratch to the batch."""

    def __init__(self, device, seed, lambda_t=10.0, lambda_s=5.0, eps_s=0.1, squash=True, lib_path=None,
                 capturable=False):
        self.lambda_t, self.lambda_s = check_weight("lambda_t", lambda_t), check_weight("lambda_s", lambda_s)
        self.eps_s = check_weight("eps_s", eps_s)
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2^64)")
        self.seed, self.squash = seed, bool(squash)
        self.device = _lib.cuda_device(device, "DeviceCAPS")
        self.lib = _lib.load(lib_path)
        self.capturable = bool(capturable)
        self._epoch = 0
        self._word = torch.zeros(1, dtype=torch.int32, device=self.device) if self.capturable else None
        self._scratch, self._scratch_rows = None, 0

    @property
    def epoch(self):
        return self._epoch if self._word is None else _lib.word_read(self._word)

    @epoch.setter
    def epoch(self, v):
        if self._word is None:
            self._epoch = int(v) & 0xFFFFFFFF
        else:
            refuse_capture("DeviceCAPS.epoch was set", "set it outside the captured region")
            _lib.word_write(self._word, v)

    def reset_noise(self):
        """New noise for the next ``near``: the epoch moves on.  Nothing runs on the device; with ``capturable=True``
        one launch of one thread."""
        if self._word is None:
            self.epoch = self._epoch + 1
        else:
            _lib.check(self.lib.usv_counter_add(self._word.data_ptr(), 1, _lib.stream_ptr(self.device)), self.lib)

    def _fresh(self, n):
        return torch.empty(n, dtype=torch.float32, device=self.device)

    def _grown(self, B):
        """The scratch for ``B`` rows: zeroed when it is made, as the kernel's ticket word needs it."""
        if B > self._scratch_rows:
            self._scratch = torch.zeros(self.lib.usv_sac_scratch_floats(B), dtype=torch.float32, device=self.device)
            self._scratch_rows = B
        return self._scratch

    def near(self, obs, out=None):
        """``obs + eps_s * z`` for a contiguous float32 ``obs`` [B, W], z ~ N(0, I) of the current epoch: a fresh
        tensor, or ``out`` (which may be ``obs`` itself).  One launch; no gradient."""
        if not isinstance(obs, torch.Tensor) or obs.dtype != torch.float32 or obs.dim() != 2 or obs.numel() < 1 or \
                obs.device != self.device or not obs.is_contiguous():
            raise ValueError(f"obs must be a contiguous float32 tensor of shape [B, W] on {self.device}")
        B, W = obs.shape
        if B * W > 2 ** 31 - 1:
            raise ValueError("B * W must be below 2^31")
        if out is None:
            out = self._fresh(obs.shape)
        else:
            _lib.check_tensor("out", out, torch.float32, (B, W), self.device)
        if self._word is None:
            refuse_capture("DeviceCAPS.near() of a default (capturable=False) object was called",
                           "its noise epoch is a kernel argument that a graph would freeze; make it with capturable=True")
            fn, epoch = self.lib.usv_caps_perturb, self._epoch
        else:
            fn, epoch = self.lib.usv_caps_perturb_dev, self._word.data_ptr()
        _lib.check(fn(B, W, obs.data_ptr(), out.data_ptr(), self.eps_s, self.seed, epoch, _lib.stream_ptr(self.device)),
                   self.lib)
        return out

    def _loss(self, mean, mean_next, mean_near, g_mean, g_next, g_near):
        """One launch.  g_*: addresses or None.  Returns the three 0-dim outputs."""
        B, A = mean.shape
        out = self._fresh(3)
        _lib.check(self.lib.usv_caps_loss(B, A, int(self.squash), mean.data_ptr(), mean_next.data_ptr(),
                                          mean_near.data_ptr(), self.lambda_t, self.lambda_s, out.data_ptr(), g_mean,
                                          g_next, g_near, self._grown(B).data_ptr(), _lib.stream_ptr(self.device)),
                   self.lib)
        return out[0], out[1], out[2]

    def loss(self, mean, mean_next, mean_near):
        """``SmoothLoss(loss, temporal, spatial)``, all 0-dim, from the actor's pre-squash means [B, A] at the
        observations, the next observations and ``near(observations)``: ``temporal = ||pi(mean) - pi(mean_next)||_2``
        and ``spatial = ||pi(mean) - pi(mean_near)||_2`` averaged over the batch, ``loss = lambda_t * temporal +
        lambda_s * spatial``.  ``loss`` carries gradient to each of the three that requires one (a row at zero
        distance contributes none); ``temporal`` and ``spatial`` are for logging.  Under ``no_grad``, or when no input
        requires grad: one launch, nothing saved."""
        check_means(mean, mean_next, mean_near, self.device)
        ts = tuple(t if t.is_contiguous() else t.contiguous() for t in (mean, mean_next, mean_near))
        if torch.is_grad_enabled() and any(t.requires_grad for t in (mean, mean_next, mean_near)):
            return SmoothLoss(*_Smooth.apply(self, *ts))
        return SmoothLoss(*self._loss(*ts, None, None, None))
