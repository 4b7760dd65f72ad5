"""PPO's minibatch loss without its eager-torch glue: advantage normalisation, the clipped surrogate, the value loss
(with SB3's ``clip_range_vf``), the entropy term, the weighted sum, ``approx_kl`` and ``clip_fraction`` in one C call,
and ``explained_variance`` in another.

``DevicePPOLoss`` is the loss lines of SB3's ``PPO.train`` (stable_baselines3/ppo/ppo.py) behind ``usv_ppo_loss``
(include/usv_hip.h) and ``common/utils.py``'s ``explained_variance`` behind ``usv_ppo_explained_variance``::

    pl = DevicePPOLoss(device)
    logp = head.evaluate(mean, latent, std, actions).log_prob          # or any torch distribution's log_prob
    out = pl.loss(logp, mb.old_log_prob, mb.advantages, values, mb.returns, clip_range=0.2, vf_coef=0.5)
    out.loss.backward()                                    # one launch for log_prob, values and entropy
    kl, frac = out.approx_kl, out.clip_fraction            # 0-dim device tensors, no host sync
    ev = pl.explained_variance(rollout_values, rollout_returns)

The forward is one launch (three with advantage normalisation: the two moment passes go first, from the same C call)
that also writes the per-row gradients at unit upstream; the backward is one launch that multiplies them by the
upstream gradient on the device.  The sums over the batch are taken in a fixed order
(gym-usv_amd/csrc/usv_ppo_math.hpp; tests/ppo_loss_ref.py restates it): every output is bitwise reproducible,
whatever the grid or the stream.  All on the current stream, without a host sync.
"""
from __future__ import annotations

import collections
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .sac import _ptr, _rows

PPOLoss = collections.namedtuple("PPOLoss", "loss policy_loss value_loss entropy_loss approx_kl clip_fraction")


def _range(name, x):
    x = float(x)
    if not (math.isfinite(x) and x >= 0.0):
        raise ValueError(f"{name} must be finite and >= 0")
    return x


def check_loss_args(clip_range, vf_coef, ent_coef, old_values, clip_range_vf, data=()):
    """The argument rules of ``DevicePPOLoss.loss`` that need no device; returns ``(clip_range, clip_range_vf, vf_coef,
    ent_coef)`` as floats (``clip_range_vf`` 0.0 without one).  ``data``: the tensors that carry no gradient."""
    if (old_values is None) != (clip_range_vf is None):
        raise ValueError("old_values and clip_range_vf come together or not at all")
    for t in data:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError("old_log_prob, advantages, returns and old_values are data: detach them")
    return (_range("clip_range", clip_range), 0.0 if clip_range_vf is None else _range("clip_range_vf", clip_range_vf),
            float(vf_coef), float(ent_coef))


class _Loss(torch.autograd.Function):
    """``DevicePPOLoss.loss`` under autograd: fresh outputs, the unit gradients saved, the backward is
    ``usv_sac_loss_backward``.  Only ``loss`` is differentiable."""

    @staticmethod
    def forward(ctx, obj, logp, values, entropy, data, scalars):
        B = logp.numel()
        g = obj._fresh((3 if entropy is not None else 2) * B)   # g_logp, g_values [B] each, g_entropy with an entropy
        at = g.data_ptr()
        out = obj._loss(logp, values, entropy, data, scalars, at, at + 4 * B, at + 8 * B if entropy is not None else None)
        ctx.obj, ctx.shapes = obj, (logp.shape, values.shape, None if entropy is None else entropy.shape)
        ctx.save_for_backward(g)
        ctx.mark_non_differentiable(*out[1:])
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, *_):
        g, = ctx.saved_tensors
        s = ctx.shapes
        B, at = g.numel() // (3 if s[2] is not None else 2), g.data_ptr()
        ol, ov = ctx.obj._fresh(s[0]), ctx.obj._fresh(s[1])
        oe = ctx.obj._fresh(s[2]) if s[2] is not None else None
        ctx.obj._backward(B, g_loss, (at, at + 4 * B, at + 8 * B if oe is not None else None), (ol, ov, oe))
        need = ctx.needs_input_grad
        return None, ol if need[1] else None, ov if need[2] else None, oe if need[3] else None, None, None


class DevicePPOLoss:
    """PPO's loss lines on ``device`` (a ROCm GPU; there is no CPU fallback).  The object owns a small scratch buffer
    that grows with the batch: calls of one object must be stream-ordered.  It does not know the policy's head:
    ``log_prob`` may come from ``DeviceSDE.evaluate`` or from any torch distribution."""

    def __init__(self, device, lib_path=None):
        self.device = _lib.cuda_device(device, "DevicePPOLoss")
        self.lib = _lib.load(lib_path)
        self._scratch, self._scratch_rows = None, 0
        self.moments = None             # the last loss call's advantage (mean, std), a [2] device tensor; None: not normalised

    def _fresh(self, n):
        return torch.empty(n, dtype=torch.float32, device=self.device)

    def _grown(self, B):
        """The scratch for ``B`` rows: zeroed when it is made, as the kernels' ticket word needs it."""
        if B > self._scratch_rows:
            self._scratch = torch.zeros(self.lib.usv_ppo_scratch_floats(B), dtype=torch.float32, device=self.device)
            self._scratch_rows = B
        return self._scratch

    def _loss(self, logp, values, entropy, data, scalars, gl, gv, ge):
        """One C call; the device of every tensor is the C entry's to check.  gl, gv, ge: addresses or None.  Returns
        the six 0-dim outputs."""
        old_logp, adv, ret, old_values = data
        normalize, clip, clip_vf, vf_coef, ent_coef = scalars
        B = logp.numel()
        out = self._fresh(8)                                # the six outputs, then the two moments
        _lib.check(self.lib.usv_ppo_loss(
            B, _ptr(logp), _ptr(old_logp), _ptr(adv), _ptr(values), _ptr(old_values), _ptr(ret), _ptr(entropy),
            int(normalize), clip, clip_vf, ent_coef, vf_coef, out.data_ptr() + 24, out.data_ptr(), gl, gv, ge,
            self._grown(B).data_ptr(), _lib.stream_ptr(self.device)), self.lib)
        self.moments = out[6:] if normalize and B > 1 else None
        return tuple(out[k] for k in range(6))

    def _backward(self, B, up, g, o):
        up = None if up is None else up if up.dtype is torch.float32 else up.float()
        _lib.check(self.lib.usv_sac_loss_backward(B, _ptr(up), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(o[0]), _ptr(o[1]),
                                                  _ptr(o[2]), None, None, None, _lib.stream_ptr(self.device)), self.lib)

    def loss(self, log_prob, old_log_prob, advantages, values, returns, clip_range=0.2, vf_coef=0.5, ent_coef=0.0,
             normalize_advantage=True, old_values=None, clip_range_vf=None, entropy=None):
        """``PPOLoss(loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction)``, 0-dim device tensors, of
        one minibatch as SB3's ``PPO.train`` computes them: ``advantages`` normalised by their mean and unbiased std
        (``normalize_advantage``, and more than one row), ``policy_loss = -min(ratio a, clamp(ratio, 1 - clip_range,
        1 + clip_range) a).mean()`` with ``ratio = exp(log_prob - old_log_prob)``, ``value_loss =
        mse_loss(returns, values_pred)`` with ``values_pred = values`` or, with ``old_values`` and ``clip_range_vf``
        (they come together), ``old_values + clamp(values - old_values, -clip_range_vf, clip_range_vf)``,
        ``entropy_loss = -entropy.mean()`` or ``-(-log_prob).mean()`` without an ``entropy`` tensor (gSDE), ``loss =
        policy_loss + ent_coef * entropy_loss + vf_coef * value_loss``, ``approx_kl = ((ratio - 1) - (log_prob -
        old_log_prob)).mean()`` and ``clip_fraction = (|ratio - 1| > clip_range).float().mean()``.  Every row tensor
        is float32 of shape [B] or [B, 1].  The gradient of ``loss`` reaches ``log_prob``, ``values`` and ``entropy``;
        the five statistics carry none and everything else is data (one that requires grad is a ``ValueError``).
        Under ``no_grad``, or when no input requires grad: nothing is saved."""
        data = (old_log_prob, advantages, returns, old_values)
        clip, clip_vf, vf_coef, ent_coef = check_loss_args(clip_range, vf_coef, ent_coef, old_values, clip_range_vf, data)
        lp = _rows("log_prob", log_prob)
        B = lp.numel()
        v = _rows("values", values, B)
        ent = None if entropy is None else _rows("entropy", entropy, B)
        data = (_rows("old_log_prob", old_log_prob, B), _rows("advantages", advantages, B), _rows("returns", returns, B),
                None if old_values is None else _rows("old_values", old_values, B))         # read by address: data
        scalars = (bool(normalize_advantage), clip, clip_vf, vf_coef, ent_coef)
        if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (log_prob, values, entropy)):
            return PPOLoss(*_Loss.apply(self, lp, v, ent, data, scalars))
        return PPOLoss(*self._loss(lp, v, ent, data, scalars, None, None, None))

    def explained_variance(self, values, returns):
        """SB3's ``explained_variance(values, returns)``: ``1 - var(returns - values) / var(returns)`` as a 0-dim
        device tensor, NaN where ``var(returns) == 0``.  Float32 tensors of one shape, any shape (a rollout's
        [T, N] as it is stored).  Two launches, no host sync, no gradient."""
        if not (isinstance(values, torch.Tensor) and isinstance(returns, torch.Tensor)) or values.shape != returns.shape:
            raise ValueError("values and returns must be float32 tensors of one shape")
        v = _rows("values", values.detach().reshape(-1))
        r = _rows("returns", returns.detach().reshape(-1), v.numel())
        out = self._fresh(())
        _lib.check(self.lib.usv_ppo_explained_variance(v.numel(), v.data_ptr(), r.data_ptr(), out.data_ptr(),
                                                       self._grown(v.numel()).data_ptr(),
                                                       _lib.stream_ptr(self.device)), self.lib)
        return out
