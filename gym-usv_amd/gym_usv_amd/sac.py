"""SAC's gradient step without its eager-torch glue: the TD target, the twin-critic loss, the actor and
entropy-coefficient losses and ``polyak_update`` as one HIP launch each.

``DeviceSACLoss`` is the loss lines of SB3's ``SAC.train`` (stable_baselines3/sac/sac.py; TD3's target where no
entropy term is given) behind ``usv_sac_critic_loss`` / ``usv_sac_policy_loss`` (include/usv_hip.h), and
``DevicePolyak`` is ``common/utils.py``'s ``polyak_update`` over a whole parameter list behind ``usv_polyak_update``::

    sl, polyak = DeviceSACLoss(device), DevicePolyak(critic.parameters(), target.parameters())
    ent = log_ent.detach().exp()
    with torch.no_grad():
        q1n, q2n = target(next_obs, next_actions)
    c = sl.critic(*critic(obs, actions), q1n, q2n, rewards, dones, ent_coef=ent, logp_next=logp2, discounts=discounts)
    c.loss.backward()                                     # one launch; c.target is the TD target
    p = sl.policy(logp, *critic(obs, a_pi), ent, log_ent_coef=log_ent, target_entropy=-act_dim)
    (p.actor_loss + p.ent_coef_loss).backward()           # one launch for logp, both q's and log_ent
    polyak.step(tau)                                      # one launch for every tensor

Each loss is one launch forward (the per-row gradients at unit upstream are written by the same launch) and one
launch backward, which multiplies them by the upstream gradient on the device.  The sums over the batch are taken in
a fixed order (gym-usv_amd/csrc/usv_sac_math.hpp; tests/sac_loss_ref.py restates it): the losses and their gradients
are bitwise reproducible, whatever the grid or the stream.  All on the current stream, without a host sync.
"""
from __future__ import annotations

import collections
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib

CriticLoss = collections.namedtuple("CriticLoss", "loss target")
PolicyLoss = collections.namedtuple("PolicyLoss", "actor_loss ent_coef_loss")


def _ptr(t):
    """The address for a ``void*`` argument: a tensor's, or one already taken (ctypes converts the int; None is
    NULL)."""
    return t.data_ptr() if isinstance(t, torch.Tensor) else t


def _rows(name, t, B=None):
    """``t`` as a contiguous float32 tensor of ``B`` elements, [B] or [B, 1].  The test comes first that a tensor
    of the expected kind passes at once: these run on every gradient step."""
    if isinstance(t, torch.Tensor) and t.dtype is torch.float32 and t.is_contiguous():
        n, d = t.numel(), t.dim()
        if n >= 1 and (B is None or n == B) and (d == 1 or (d == 2 and t.shape[1] == 1)):
            return t
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in (1, 2) or \
            (t.dim() == 2 and t.shape[1] != 1) or t.numel() < 1 or (B is not None and t.numel() != B):
        raise ValueError(f"{name} must be a float32 tensor of shape [B] or [B, 1]" + ("" if B is None else f" with B = {B}"))
    return t.contiguous()


def _scalar(name, t):
    """``t`` as a one-element float32 tensor."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1:
        raise ValueError(f"{name} must be a float32 tensor with one element")
    return t if t.is_contiguous() else t.contiguous()


def check_critic_args(ent_coef, logp_next, discounts, gamma):
    """The argument rules of ``DeviceSACLoss.critic`` that need no device; returns ``gamma`` as a float (0.0 with
    ``discounts``)."""
    if (ent_coef is None) != (logp_next is None):
        raise ValueError("ent_coef and logp_next come together or not at all")
    if (discounts is None) == (gamma is None):
        raise ValueError("exactly one of discounts and gamma must be given")
    if ent_coef is not None and ent_coef.requires_grad:
        raise ValueError("ent_coef is data (SB3 detaches it): pass log_ent_coef.detach().exp()")
    return 0.0 if gamma is None else float(gamma)


def check_policy_args(ent_coef, log_ent_coef, target_entropy):
    """The argument rules of ``DeviceSACLoss.policy`` that need no device; returns ``target_entropy`` as a float."""
    if not isinstance(ent_coef, torch.Tensor):
        raise ValueError("ent_coef must be a one-element float32 tensor on the device")
    if ent_coef.requires_grad:
        raise ValueError("ent_coef is data (SB3 detaches it): pass log_ent_coef.detach().exp()")
    if (log_ent_coef is None) != (target_entropy is None):
        raise ValueError("log_ent_coef and target_entropy come together or not at all")
    return 0.0 if target_entropy is None else float(target_entropy)


class _Critic(torch.autograd.Function):
    """``DeviceSACLoss.critic`` under autograd: fresh outputs, the unit gradients saved, the backward is
    ``usv_sac_loss_backward``."""

    @staticmethod
    def forward(ctx, obj, q1, q2, data, gamma):
        B = q1.numel()
        g = obj._fresh(2 * B)                               # g_q1, g_q2 [B] each
        loss, target = obj._critic(q1, q2, data, gamma, g.data_ptr(), g.data_ptr() + 4 * B)
        ctx.obj, ctx.shapes = obj, (q1.shape, q2.shape)
        ctx.save_for_backward(g)
        ctx.mark_non_differentiable(target)
        ctx.set_materialize_grads(False)                    # an unused output's gradient stays None: NULL, zeros
        return loss, target

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, g_target):
        g, = ctx.saved_tensors
        B, at = g.numel() // 2, g.data_ptr()
        o1, o2 = ctx.obj._fresh(ctx.shapes[0]), ctx.obj._fresh(ctx.shapes[1])
        ctx.obj._backward(B, g_loss, (at, at + 4 * B, None), (o1, o2, None), None, None, None)
        need = ctx.needs_input_grad
        return None, o1 if need[1] else None, o2 if need[2] else None, None, None


class _Policy(torch.autograd.Function):
    """``DeviceSACLoss.policy`` under autograd; ``ent_coef_loss`` is None without ``log_ent``."""

    @staticmethod
    def forward(ctx, obj, logp, q1, q2, log_ent, ent, te):
        B = logp.numel()
        g = obj._fresh(3 * B + 1)                           # g_logp, g_q1, g_q2 [B] each, g_log_ent
        at = g.data_ptr()
        actor, ent_loss = obj._policy(logp, q1, q2, ent, log_ent, te, at, at + 4 * B, at + 8 * B,
                                      at + 12 * B if log_ent is not None else None)
        ctx.obj, ctx.shapes = obj, (logp.shape, q1.shape, q2.shape, None if log_ent is None else log_ent.shape)
        ctx.save_for_backward(g)
        ctx.set_materialize_grads(False)
        return actor, ent_loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_actor, g_ent):
        g, = ctx.saved_tensors
        s, B, at = ctx.shapes, g.numel() // 3, g.data_ptr()
        ol, o1, o2 = ctx.obj._fresh(s[0]), ctx.obj._fresh(s[1]), ctx.obj._fresh(s[2])
        oe = ctx.obj._fresh(s[3]) if s[3] is not None else None
        ctx.obj._backward(B, g_actor, (at, at + 4 * B, at + 8 * B), (ol, o1, o2), g_ent,
                          at + 12 * B if oe is not None else None, oe)
        need = ctx.needs_input_grad
        return (None, ol if need[1] else None, o1 if need[2] else None, o2 if need[3] else None,
                oe if need[4] else None, None, None)


class DeviceSACLoss:
    """SAC's loss lines on ``device`` (a ROCm GPU; there is no CPU fallback).  The object owns a small scratch buffer
    that grows with the batch: calls of one object must be stream-ordered."""

    def __init__(self, device, lib_path=None):
        self.device = _lib.cuda_device(device, "DeviceSACLoss")
        self.lib = _lib.load(lib_path)
        self._scratch, self._scratch_rows = None, 0

    def _fresh(self, n):
        return torch.empty(n, dtype=torch.float32, device=self.device)

    def _grown(self, B):
        """The scratch for ``B`` rows: zeroed when it is made, as the kernels' ticket word needs it."""
        if B > self._scratch_rows:
            self._scratch = torch.zeros(self.lib.usv_sac_scratch_floats(B), dtype=torch.float32, device=self.device)
            self._scratch_rows = B
        return self._scratch

    def _critic(self, q1, q2, data, gamma, g1, g2):
        """One launch; the device of every tensor is the C entry's to check.  g1, g2: addresses or None.  Returns
        (loss, target shaped like q1)."""
        q1n, q2n, rew, done, ent, logp_next, disc = data
        B = q1.numel()
        loss, target = self._fresh(()), self._fresh(q1.shape)
        _lib.check(self.lib.usv_sac_critic_loss(
            B, _ptr(q1), _ptr(q2), _ptr(q1n), _ptr(q2n), _ptr(rew), _ptr(done), _ptr(ent), _ptr(logp_next), _ptr(disc),
            gamma, target.data_ptr(), loss.data_ptr(), g1, g2, self._grown(B).data_ptr(),
            _lib.stream_ptr(self.device)), self.lib)
        return loss, target

    def _policy(self, logp, q1, q2, ent, log_ent, te, gl, g1, g2, ge):
        B = logp.numel()
        out = self._fresh(2)
        _lib.check(self.lib.usv_sac_policy_loss(
            B, _ptr(logp), _ptr(q1), _ptr(q2), _ptr(ent), _ptr(log_ent), te, out.data_ptr(),
            out.data_ptr() + 4 if log_ent is not None else None, gl, g1, g2, ge,
            self._grown(B).data_ptr(), _lib.stream_ptr(self.device)), self.lib)
        return out[0], out[1] if log_ent is not None else None

    def _backward(self, B, up, g, o, up_s, gs, os):
        up, up_s = (None if x is None else x if x.dtype is torch.float32 else x.float() for x in (up, up_s))
        _lib.check(self.lib.usv_sac_loss_backward(B, _ptr(up), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(o[0]), _ptr(o[1]),
                                                  _ptr(o[2]), _ptr(up_s), _ptr(gs), _ptr(os),
                                                  _lib.stream_ptr(self.device)), self.lib)

    def critic(self, q1, q2, q1_next, q2_next, rewards, dones, *, ent_coef=None, logp_next=None, discounts=None,
               gamma=None):
        """``CriticLoss(loss, target)``: ``target = rewards + (1 - dones) * disc * (min(q1_next, q2_next) - ent_coef *
        logp_next)`` (shaped like ``q1``, no gradient) and ``loss = 0.5 * (mse_loss(q1, target) + mse_loss(q2,
        target))`` (0-dim).  ``disc`` is the per-row ``discounts`` or the scalar ``gamma``: exactly one is given.
        Without ``ent_coef`` and ``logp_next`` (they come together) the target is TD3's.  Every row tensor is float32
        of shape [B] or [B, 1]; ``ent_coef`` is a one-element device tensor and data (one that requires grad is a
        ``ValueError``).  The gradient reaches ``q1`` and ``q2``; everything else is data.  Under ``no_grad``, or
        when neither requires grad: one launch, nothing saved."""
        gamma = check_critic_args(ent_coef, logp_next, discounts, gamma)
        q1c, q2c = _rows("q1", q1), _rows("q2", q2, q1.numel())
        B = q1c.numel()
        data = (_rows("q1_next", q1_next, B), _rows("q2_next", q2_next, B), _rows("rewards", rewards, B),
                _rows("dones", dones, B), None if ent_coef is None else _scalar("ent_coef", ent_coef),
                None if logp_next is None else _rows("logp_next", logp_next, B),
                None if discounts is None else _rows("discounts", discounts, B))      # read by address: data
        if torch.is_grad_enabled() and (q1.requires_grad or q2.requires_grad):
            return CriticLoss(*_Critic.apply(self, q1c, q2c, data, gamma))
        return CriticLoss(*self._critic(q1c, q2c, data, gamma, None, None))

    def policy(self, logp, q1_pi, q2_pi, ent_coef, *, log_ent_coef=None, target_entropy=None):
        """``PolicyLoss(actor_loss, ent_coef_loss)``: ``actor_loss = (ent_coef * logp - min(q1_pi, q2_pi)).mean()`` and,
        with ``log_ent_coef`` (one element) and ``target_entropy`` (a float), ``ent_coef_loss = -(log_ent_coef * (logp
        + target_entropy)).mean()`` with ``logp`` as data there, as SB3 detaches it; otherwise None.  Both 0-dim.
        ``actor_loss`` carries gradient to ``logp``, ``q1_pi`` and ``q2_pi`` (``torch.min``'s: a tie halves it) and
        ``ent_coef_loss`` to ``log_ent_coef``; ``(actor_loss + ent_coef_loss).backward()`` is one launch.  ``ent_coef`` is
        data: one that requires grad is a ``ValueError``."""
        te = check_policy_args(ent_coef, log_ent_coef, target_entropy)
        lp = _rows("logp", logp)
        B = lp.numel()
        q1c, q2c, ent = _rows("q1_pi", q1_pi, B), _rows("q2_pi", q2_pi, B), _scalar("ent_coef", ent_coef)
        le = None if log_ent_coef is None else _scalar("log_ent_coef", log_ent_coef)
        if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (logp, q1_pi, q2_pi, log_ent_coef)):
            return PolicyLoss(*_Policy.apply(self, lp, q1c, q2c, le, ent, te))
        return PolicyLoss(*self._policy(lp, q1c, q2c, ent, le, te, None, None, None, None))


class DevicePolyak:
    """SB3's ``polyak_update(params, target_params, tau)`` as one launch for the whole list: ``t = t * (1 - tau) +
    tau * p`` with three float32 roundings (the two-op ``t.mul_(1 - tau).add_(p, alpha=tau)`` without a fused
    multiply-add).  The tensors are float32, contiguous, on one ROCm device and pairwise of equal shape
    (``ValueError`` otherwise); zero-element tensors are skipped.  The device table of the pairs is built by the
    first ``step`` (or by ``prepare()``) and again whenever a ``data_ptr()`` has changed."""

    def __init__(self, params, target_params, lib_path=None):
        src, dst = list(params), list(target_params)         # the tensors themselves: a rebound .data is seen
        if len(src) != len(dst) or not src:
            raise ValueError("params and target_params must be two non-empty lists of equal length")
        for p, t in zip(src, dst):
            if p.dtype != torch.float32 or t.dtype != torch.float32 or not p.is_contiguous() or not t.is_contiguous():
                raise ValueError("every tensor must be float32 and contiguous")
            if p.shape != t.shape:
                raise ValueError("params and target_params must have pairwise equal shapes")
            if p.device != src[0].device or t.device != src[0].device:
                raise ValueError("every tensor must be on one device")
        self.device = _lib.cuda_device(src[0].device, "DevicePolyak")
        self.lib = _lib.load(lib_path)
        self._src, self._dst = src, dst
        self._ptrs = self._pairs = self._table = None

    def _current(self):
        return tuple(x.data_ptr() for x in self._src) + tuple(x.data_ptr() for x in self._dst)

    def _pending(self):
        """The current addresses, and whether the device table has to be built from them; (re)makes the host pairs and
        the table's memory where it has."""
        ptrs = self._current()
        if ptrs == self._ptrs:
            return ptrs, False
        n = len(self._src)
        self._pairs = (_lib.UsvPolyakPair * n)(*(_lib.UsvPolyakPair(p.data_ptr(), t.data_ptr(), p.numel())
                                                 for p, t in zip(self._src, self._dst)))
        nbytes = self.lib.usv_polyak_table_bytes(self._pairs, n)
        self._table = torch.zeros(max(1, (nbytes + 7) // 8), dtype=torch.int64, device=self.device)
        self._ptrs = None
        return ptrs, True

    def prepare(self):
        """Uploads the device table now, where it is not up to date (a device synchronise and a host copy; nothing is
        launched).  Call it before ``step`` is captured into a graph: an upload cannot be recorded."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DevicePolyak.prepare() synchronises the device: call it before the capture begins")
        ptrs, upload = self._pending()
        if upload:
            _lib.check(self.lib.usv_polyak_prepare(self._pairs, len(self._src), self._table.data_ptr(),
                                                   self._table.numel() * 8), self.lib)
            self._ptrs = ptrs

    def step(self, tau):
        """One launch on the current stream.  Legal inside ``torch.cuda.graph`` once the table is uploaded
        (``prepare()``, or an earlier ``step``): with an upload pending while the stream is capturing it raises
        ``RuntimeError``.  A captured step holds the table's address: the tensors must keep theirs."""
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and self._current() != self._ptrs:
            raise RuntimeError("DevicePolyak.step(): the table upload is pending (a first step, or a tensor has moved) "
                               "while the stream is capturing a graph; call prepare() before the capture begins")
        ptrs, upload = self._pending()
        _lib.check(self.lib.usv_polyak_update(self._pairs, len(self._src), self._table.data_ptr(), self._table.numel() * 8,
                                              int(upload), ctypes.c_double(float(tau)), _lib.stream_ptr(self.device)),
                   self.lib)
        self._ptrs = ptrs
