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
it in float64.  PPO's update-time ``log_prob`` never needed W; ``DeviceSDE.evaluate`` is SB3's
``evaluate_actions`` for stored actions with PPO's clipped surrogate on the same row and a HIP backward
(``usv_sde_eval_forward`` / ``_backward``): one launch forward, two backward, in place of some tens each way.

SAC differentiates through the sample, so ``DeviceSDE.squashed`` is the same head with ``squash_output=True``
and a HIP backward (``usv_sde_squash_forward`` / ``_backward``): the backward rebuilds the normals from the
same counters, so nothing of size [B, L, A] is saved between the two.
"""
from __future__ import annotations

import collections
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import ptr as _ptr
from .optim import refuse_capture

MAX_LATENT = 4096

SquashedSample = collections.namedtuple("SquashedSample", "actions env_actions log_prob gaussian_actions")
Evaluation = collections.namedtuple("Evaluation", "log_prob surrogate ratio")


def _fresh(head, *shapes, make=torch.empty):
    """Fresh float32 tensors of ``shapes`` on the head's device."""
    return tuple(make(s, dtype=torch.float32, device=head.device) for s in shapes)


def _contiguous(*tensors):
    """Each tensor contiguous; None (an unused output's gradient: NULL, zeros) stays None."""
    return tuple(None if t is None else t.contiguous() for t in tensors)


class _Squashed(torch.autograd.Function):
    """``DeviceSDE.squashed`` under autograd: the forward writes fresh tensors (the saved ``gauss`` / ``var`` must
    outlive the head's next call), the backward is ``usv_sde_squash_backward`` with the forward's epoch."""

    @staticmethod
    def forward(ctx, head, mean, latent, std):
        n, A = head.n, head.act_dim
        act, env, gauss, var, logp = _fresh(head, (n, A), (n, A), (n, A), (n, A), (n,))
        head._squash_forward(mean, latent, std, (act, env, logp, gauss, var))
        ctx.head, ctx.epoch, ctx.generation = head, head._epoch, head._generation
        ctx.save_for_backward(mean, latent, std, gauss, var)
        ctx.mark_non_differentiable(env, gauss)
        ctx.set_materialize_grads(False)                    # an unused output's gradient stays None: NULL, zeros
        return act, env, logp, gauss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_act, g_env, g_logp, g_gauss):
        head = ctx.head
        mean, latent, std, gauss, var = ctx.saved_tensors
        n, L, A = head.n, head.latent_dim, head.act_dim
        g_act, g_logp = _contiguous(g_act, g_logp)
        if head.capturable and head._generation != ctx.generation:
            raise RuntimeError("DeviceSDE(capturable=True): the noise epoch was changed (reset_noise() or .epoch) between "
                               "squashed() and its backward(), which reads the same device word: the backward would "
                               "rebuild another matrix than the forward used")
        g_mean, g_lat, g_std = _fresh(head, (n, A), (n, L), (L, A))
        head._squash_backward(ctx.epoch, mean, latent, std, gauss, var, g_act, g_logp, g_mean, g_lat, g_std)
        need = ctx.needs_input_grad
        return None, g_mean if need[1] else None, g_lat if need[2] else None, g_std if need[3] else None


class _Evaluate(torch.autograd.Function):
    """``DeviceSDE.evaluate`` under autograd: fresh outputs, ``var`` and ``ratio`` saved beside the inputs, the
    backward is ``usv_sde_eval_backward``.  Without the PPO arguments ``surrogate`` and ``ratio`` are None."""

    @staticmethod
    def forward(ctx, head, mean, latent, std, actions, old_log_prob, advantages, clip_range):
        B, A = mean.shape[0], head.act_dim
        ppo = old_log_prob is not None
        logp, var = _fresh(head, (B,), (B, A))
        sur, ratio = _fresh(head, (B,), (B,)) if ppo else (None, None)
        head._eval_forward(mean, latent, std, actions, old_log_prob, advantages, clip_range, logp, sur, ratio, var)
        ctx.head, ctx.clip = head, clip_range
        ctx.save_for_backward(mean, latent, std, actions, var, ratio, advantages)
        if ppo:
            ctx.mark_non_differentiable(ratio)
        ctx.set_materialize_grads(False)                    # an unused output's gradient stays None: NULL, zeros
        return logp, sur, ratio

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logp, g_sur, g_ratio):
        head = ctx.head
        mean, latent, std, actions, var, ratio, adv = ctx.saved_tensors
        B, L, A = mean.shape[0], head.latent_dim, head.act_dim
        need = ctx.needs_input_grad
        g_logp, g_sur = _contiguous(g_logp, g_sur)
        g_mean, g_std = _fresh(head, (B, A), (L, A))
        g_lat = _fresh(head, (B, L))[0] if need[2] else None
        head._eval_backward(mean, latent, std, actions, var, ratio, adv, ctx.clip, g_logp, g_sur, g_mean, g_lat, g_std)
        return None, g_mean if need[1] else None, g_lat, g_std if need[3] else None, None, None, None, None


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
    ``env.step`` do).  ``copy=True`` returns fresh tensors.  There is no CPU fallback.

    ``capturable=True``: the epoch is a word in device memory that the kernels read (the ``usv_sde_*_dev`` entries),
    so ``sample``, ``weights`` and ``squashed`` with its backward are legal inside ``torch.cuda.graph`` and a replay
    draws the noise of the epoch the word then holds.  ``reset_noise()`` is one launch of one thread
    (``usv_counter_add``), to be captured with the rest; setting ``epoch`` is a stream-ordered write and reading it is
    **a host sync**.  The backward of ``squashed`` reads the same word as its forward: a ``reset_noise()`` or an
    ``epoch`` assignment between the two is an error, which eager code meets as a ``RuntimeError`` from
    ``backward()`` (a host-side count of the changes; a replayed graph runs no host code and cannot be checked).
    In the default form the four calls raise ``RuntimeError`` while the stream is capturing: the epoch is a kernel
    argument there, and a graph would freeze it."""

    def __init__(self, num_envs, latent_dim, act_dim, device, seed, low, high, env_id_offset=0, copy=False,
                 lib_path=None, capturable=False):
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
        self.capturable = bool(capturable)
        self._epoch, self._generation = 0, 0               # the host's epoch; how often the epoch has been changed
        self._word = torch.zeros(1, dtype=torch.int32, device=device) if self.capturable else None
        self._s = _lib.UsvSde(n, L, A, 0, seed, gid0, (ctypes.c_float * 4)(*lo), (ctypes.c_float * 4)(*hi))
        self._sp = ctypes.byref(self._s)
        self._out = _fresh(self, (n, A), (n, A), (n,), make=torch.zeros)
        self._sq_out = self._scratch = None                # squashed's buffers, made by its first call
        self._eval_scratch = None                           # evaluate's backward scratch, grown with B

    @property
    def epoch(self):
        return self._epoch if self._word is None else _lib.word_read(self._word)

    @epoch.setter
    def epoch(self, v):
        self._generation += 1
        if self._word is None:
            self._epoch = int(v) & 0xFFFFFFFF
        else:
            refuse_capture("DeviceSDE.epoch was set", "set it outside the captured region")
            _lib.word_write(self._word, v)

    def reset_noise(self):
        """SB3's ``reset_noise`` / ``sample_weights``: a new matrix for every env from the next ``sample``
        on.  A host integer, nothing runs on the device; with ``capturable=True`` one launch of one thread."""
        if self._word is None:
            self.epoch = self._epoch + 1
        else:
            self._generation += 1
            _lib.check(self.lib.usv_counter_add(_ptr(self._word), 1, _lib.stream_ptr(self.device)), self.lib)

    def _noise_entry(self, name, who):
        """The C entry ``name`` and its epoch argument: the host integer, or ``name_dev`` and the device word."""
        if self._word is not None:
            return getattr(self.lib, name + "_dev"), _ptr(self._word)
        refuse_capture(f"DeviceSDE.{who}() of a default (capturable=False) head was called",
                       "its noise epoch is a kernel argument that a graph would freeze; make it with capturable=True")
        return getattr(self.lib, name), self._epoch

    def sample(self, mean, latent, std, out=None):
        """``(a, a_env, logp)`` in one launch: ``a = mean + latent @ W`` [N, A] (unclipped, the rollout
        buffer's), ``a_env = max(min(a, high), low)`` [N, A] and
        ``logp = Normal(mean, sqrt(latent^2 @ std^2 + 1e-6)).log_prob(a).sum(-1)`` [N].

        ``mean`` [N, A] and ``std`` [L, A] (``log_std.exp()``) are contiguous float32; ``latent`` is
        float32 [N, L] with inner stride 1, a row stride that is a multiple of 4 and >= L, and a 16-B
        aligned base.  ``out``: three contiguous float32 tensors of those shapes to write instead."""
        n, L, A = self.n, self.latent_dim, self.act_dim
        self._check(("mean", mean, (n, A)), ("std", std, (L, A)))
        stride = self._latent_stride("latent", latent)
        if out is None:
            out = self._out
        else:
            self._check(*zip(("out[0]", "out[1]", "out[2]"), out, ((n, A), (n, A), (n,))))
        a, a_env, logp = out
        fn, epoch = self._noise_entry("usv_sde_sample", "sample")
        _lib.check(fn(self._sp, epoch, _ptr(mean), _ptr(latent), stride, _ptr(std), _ptr(a),
                                           _ptr(a_env), _ptr(logp), _lib.stream_ptr(self.device)), self.lib)
        if self.copy and out is self._out:
            return a.clone(), a_env.clone(), logp.clone()
        return a, a_env, logp

    def weights(self, std, out=None):
        """SB3's ``exploration_mat`` of the current epoch for every env, [N, L, A]: a fresh tensor, or
        ``out``.  Off the hot path (``sample`` does not read it)."""
        n, L, A = self.n, self.latent_dim, self.act_dim
        self._check(("std", std, (L, A)))
        if out is None:
            out, = _fresh(self, (n, L, A))
        else:
            self._check(("out", out, (n, L, A)))
        fn, epoch = self._noise_entry("usv_sde_weights", "weights")
        _lib.check(fn(self._sp, epoch, _ptr(std), _ptr(out), _lib.stream_ptr(self.device)), self.lib)
        return out

    def _check(self, *table):
        """``check_tensor`` for every (name, tensor, shape) of ``table`` whose tensor is not None."""
        for name, t, shape in table:
            if t is not None:
                _lib.check_tensor(name, t, torch.float32, shape, self.device)

    def _latent_stride(self, name, t, n=None):
        # a single env's row has no stride of its own: the kernel is then given L
        return _lib.check_rows(name, t, torch.float32, (self.n if n is None else n, self.latent_dim), self.device,
                               stride_multiple=4, align=16)

    def _grown(self, attr, need):
        """The scratch buffer ``attr`` of this head, made anew where it holds fewer than ``need`` floats."""
        if getattr(self, attr) is None or getattr(self, attr).numel() < need:
            setattr(self, attr, _fresh(self, (need,))[0])
        return getattr(self, attr)

    def _squash_forward(self, mean, latent, std, out):
        n, L, A = self.n, self.latent_dim, self.act_dim
        self._check(("mean", mean, (n, A)), ("std", std, (L, A)))
        stride = self._latent_stride("latent", latent)
        act, env, logp, gauss, var = out
        fn, epoch = self._noise_entry("usv_sde_squash_forward", "squashed")
        _lib.check(fn(self._sp, epoch, _ptr(mean), _ptr(latent), stride, _ptr(std), _ptr(act), _ptr(env), _ptr(logp),
                      _ptr(gauss), _ptr(var), _lib.stream_ptr(self.device)), self.lib)

    def _squash_backward(self, epoch, mean, latent, std, gauss, var, g_act, g_logp, g_mean, g_lat, g_std):
        n, L, A = self.n, self.latent_dim, self.act_dim
        self._check(("g_act", g_act, (n, A)), ("g_logp", g_logp, (n,)), ("g_mean", g_mean, (n, A)),
                    ("g_std", g_std, (L, A)), ("gauss", gauss, (n, A)), ("var", var, (n, A)))
        scratch = self._grown("_scratch", self.lib.usv_sde_squash_scratch_floats(self._sp))
        fn, word = self._noise_entry("usv_sde_squash_backward", "squashed")
        _lib.check(fn(
            self._sp, epoch if self._word is None else word, _ptr(mean), _ptr(latent),
            self._latent_stride("latent", latent), _ptr(std), _ptr(gauss),
            _ptr(var), _ptr(g_act), _ptr(g_logp), _ptr(g_mean), _ptr(g_lat), self._latent_stride("g_lat", g_lat),
            _ptr(g_std), _ptr(scratch), _lib.stream_ptr(self.device)), self.lib)

    def squashed(self, mean, latent, std):
        """SAC's head (``squash_output=True``, ``learn_features=True``): ``SquashedSample(actions, env_actions,
        log_prob, gaussian_actions)`` with ``gaussian_actions = mean + latent @ W`` [N, A] (bit-equal to
        ``sample``'s unclipped action), ``actions = tanh(gaussian_actions)``, ``env_actions = low + (actions + 1)
        * 0.5 * (high - low)`` (SB3's ``unscale_action``) and ``log_prob`` [N] = the Gaussian log-probability of
        ``gaussian_actions`` minus ``sum(ln(1 - actions^2 + 1e-6))``, with ``1 - actions^2`` computed as
        ``4 t / (1 + t)^2``, ``t = exp(-2 |u|)``.  Arguments as ``sample``'s.

        No input requires grad, or under ``torch.no_grad()``: one launch into this object's persistent buffers
        (``copy`` as for ``sample``).  Otherwise the call is a ``torch.autograd.Function``: the forward writes
        fresh tensors, and ``backward`` (once differentiable; two launches on the current stream) returns the
        gradients of ``actions`` and ``log_prob`` with respect to ``mean``, ``latent`` (through the noise and
        the variance) and ``std`` (chain ``log_std.exp()`` in front and autograd carries it into ``log_std``).
        ``env_actions`` and ``gaussian_actions`` carry no gradient.  The epoch is the forward's: a
        ``reset_noise()`` before ``backward()`` does not change the backward's matrix (with ``capturable=True`` it is
        an error: see the class).  The backward's scratch
        belongs to the head: backward calls of one head must be stream-ordered.

        How SAC uses it.  One head of ``num_envs`` rows collects: rows are global env ids, and
        ``reset_noise()`` every ``sde_sample_freq`` steps.  A second head of ``batch_size`` rows, with another
        seed, serves the update: row = position in the minibatch, ``reset_noise()`` once per gradient step as
        ``SAC.train`` does, so the observations (with grad) and the next observations (without) of that step
        see the same matrices."""
        if torch.is_grad_enabled() and (mean.requires_grad or latent.requires_grad or std.requires_grad):
            return SquashedSample(*_Squashed.apply(self, mean, latent, std))
        if self._sq_out is None:
            n, A = self.n, self.act_dim
            self._sq_out = _fresh(self, (n, A), (n, A), (n,), (n, A), (n, A), make=torch.zeros)
        self._squash_forward(mean.detach(), latent.detach(), std.detach(), self._sq_out)
        act, env, logp, gauss, _ = self._sq_out
        if self.copy:
            return SquashedSample(act.clone(), env.clone(), logp.clone(), gauss.clone())
        return SquashedSample(act, env, logp, gauss)

    def _eval_forward(self, mean, latent, std, actions, old_log_prob, advantages, clip_range, logp, sur, ratio, var):
        B, L, A = mean.shape[0], self.latent_dim, self.act_dim
        self._check(("mean", mean, (B, A)), ("std", std, (L, A)), ("actions", actions, (B, A)),
                    ("old_log_prob", old_log_prob, (B,)), ("advantages", advantages, (B,)), ("log_prob", logp, (B,)),
                    ("surrogate", sur, (B,)), ("ratio", ratio, (B,)), ("var", var, (B, A)))
        _lib.check(self.lib.usv_sde_eval_forward(
            self._sp, B, _ptr(mean), _ptr(latent), self._latent_stride("latent", latent, B), _ptr(std), _ptr(actions),
            _ptr(old_log_prob), _ptr(advantages), 0.0 if clip_range is None else clip_range, _ptr(logp), _ptr(sur),
            _ptr(ratio), _ptr(var), _lib.stream_ptr(self.device)), self.lib)

    def _eval_backward(self, mean, latent, std, actions, var, ratio, advantages, clip_range, g_logp, g_sur, g_mean, g_lat,
                       g_std):
        B, L, A = mean.shape[0], self.latent_dim, self.act_dim
        self._check(("mean", mean, (B, A)), ("std", std, (L, A)), ("actions", actions, (B, A)), ("var", var, (B, A)),
                    ("ratio", ratio, (B,)), ("advantages", advantages, (B,)), ("g_logp", g_logp, (B,)),
                    ("g_sur", g_sur, (B,)), ("g_mean", g_mean, (B, A)), ("g_std", g_std, (L, A)))
        scratch = self._grown("_eval_scratch", self.lib.usv_sde_eval_scratch_floats(self._sp, B))
        _lib.check(self.lib.usv_sde_eval_backward(
            self._sp, B, _ptr(mean), _ptr(latent), self._latent_stride("latent", latent, B), _ptr(std), _ptr(actions),
            _ptr(var), _ptr(ratio), _ptr(advantages), 0.0 if clip_range is None else clip_range, _ptr(g_logp), _ptr(g_sur),
            _ptr(g_mean), _ptr(g_lat), 0 if g_lat is None else self._latent_stride("g_lat", g_lat, B), _ptr(g_std),
            _ptr(scratch), _lib.stream_ptr(self.device)), self.lib)

    def evaluate(self, mean, latent, std, actions, old_log_prob=None, advantages=None, clip_range=None):
        """PPO's update-time head, SB3's ``evaluate_actions`` for gSDE with the clipped surrogate on the same row:
        ``Evaluation(log_prob, surrogate, ratio)`` with ``log_prob = Normal(mean, sqrt(latent^2 @ std^2 +
        1e-6)).log_prob(actions).sum(-1)`` [B] (bit-equal to the ``logp`` that ``sample`` returned with these
        actions), ``ratio = exp(log_prob - old_log_prob)`` [B] and ``surrogate = min(ratio * advantages,
        clamp(ratio, 1 - clip_range, 1 + clip_range) * advantages)`` [B]: ``-surrogate.mean()`` is PPO's policy
        loss.  ``old_log_prob``, ``advantages`` [B] and ``clip_range`` (a float >= 0) come together; without them
        ``surrogate`` and ``ratio`` are None.

        No noise is drawn: the call does not depend on ``num_envs``, the seed or the epoch, and ``B`` (``mean``'s
        rows, >= 1) is the caller's: a short last minibatch is a smaller ``B``.  ``mean``, ``actions`` [B, A] and
        ``std`` [L, A] are contiguous float32; ``latent`` [B, L] as for ``sample``.  The outputs are fresh tensors.

        Under ``torch.no_grad()``, or when no input requires grad: one launch, nothing saved.  Otherwise a
        ``torch.autograd.Function`` whose backward (once differentiable; two launches on the current stream)
        returns the gradients of ``log_prob`` and ``surrogate`` with respect to ``mean``, ``std`` and, only where
        it requires grad, ``latent`` (PPO's ``learn_features=False`` passes ``latent.detach()``, and nothing of
        size [B, L] is then written).  ``ratio`` carries no gradient (it feeds ``approx_kl`` / ``clip_fraction``);
        ``actions``, ``old_log_prob`` and ``advantages`` are data.  The gradient of ``std`` is summed over rows in a
        fixed order without atomics: bitwise reproducible.  The backward's scratch belongs to the head and grows
        with ``B``: backward calls of one head must be stream-ordered."""
        given = [x is not None for x in (old_log_prob, advantages, clip_range)]
        if any(given) and not all(given):
            raise ValueError("old_log_prob, advantages and clip_range come together or not at all")
        if mean.dim() != 2 or mean.shape[0] < 1:
            raise ValueError("mean must be a [B, act_dim] tensor with B >= 1")
        if clip_range is not None:
            clip_range = float(clip_range)
            if not clip_range >= 0.0:
                raise ValueError("clip_range must be >= 0")
        data = tuple(None if x is None else x.detach() for x in (actions, old_log_prob, advantages))
        if torch.is_grad_enabled() and (mean.requires_grad or latent.requires_grad or std.requires_grad):
            return Evaluation(*_Evaluate.apply(self, mean, latent, std, *data, clip_range))
        B = mean.shape[0]
        logp, = _fresh(self, (B,))
        sur, ratio = _fresh(self, (B,), (B,)) if all(given) else (None, None)
        self._eval_forward(mean.detach(), latent.detach(), std.detach(), *data, clip_range, logp, sur, ratio, None)
        return Evaluation(logp, sur, ratio)
