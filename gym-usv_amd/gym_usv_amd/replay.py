"""SB3's ``ReplayBuffer`` on the device, behind ``UsvVectorEnv.step`` and ``DeviceWrappers.step``.

``DeviceReplay`` is ``ReplayBuffer.add``, ``sample`` and ``_get_samples``
(stable_baselines3/common/buffers.py, with ``optimize_memory_usage=False`` and
``handle_timeout_termination=True``) plus the terminal-observation substitution of
``OffPolicyAlgorithm._store_transition`` as HIP kernels (``usv_replay_*``, include/usv_hip.h) on the
current stream.  Nothing here waits for the device; the ring position and the fill count are host
integers, as SB3's ``pos`` and ``full`` are::

    wr = DeviceWrappers(env.num_envs, env.obs_dim, 5, env.device, env.reward.dtype)
    rb = DeviceReplay(env.num_envs, 400_000, 5 * env.obs_dim, env.act_dim, env.device, env.reward.dtype, n_stack=5)
    wr.reset(obs)
    for step in range(steps):
        a = actor(wr.stacked)                             # the ring's window, read in place
        rb.put_obs(wr.stacked, a)                         # before the step: the next push overwrites it
        obs, rew, term, trunc, info = env.step(clip(a))
        stacked, final_stack, _ = wr.step(obs, rew, info["_final_obs"], info["final_obs"])
        rb.put_step(rew, term, trunc, stacked, final_stack)
        mb = rb.sample(256)                               # one device randint, one launch
        mb.observations, mb.actions, mb.next_observations, mb.dones, mb.rewards

The stacked windows are not stored: the ring keeps the newest ``D`` columns of ``obs`` and of
``next_obs`` per transition (``2 D`` floats where SB3 keeps ``2 k D``) and one byte that says how many
slots of the window were live, and ``gather`` rebuilds both windows from the same ``k + 1`` frames, bit
for bit what full storage would hold (tests/replay_ref.py).

``DeviceReplay(..., n_steps=3, gamma=0.99)`` and ``rb.sample_nstep(256)`` are SB3 2.7's
``NStepReplayBuffer``: the discounted sum of up to ``n_steps`` rewards, the ``next_observations`` and
``dones`` at the end of that run and a per-sample ``discounts``, in the same single launch
(``gather_nstep``; tests/replay_nstep_ref.py).  Nothing stored changes.

The buffer stores what it is given: with ``DeviceWrappers(normalize={})`` that is the frame as normalised
at collection time.  Re-normalising stored observations with later statistics (SB3's
``_normalize_obs(..., env)`` in ``_get_samples``) is not done.
"""
from __future__ import annotations

import collections
import ctypes

import torch

from . import _lib
from ._lib import ptr as _ptr


# The fields of SB3's ReplayBufferSamples (common/type_aliases.py), in its order.
ReplaySamples = collections.namedtuple(
    "ReplaySamples", ("observations", "actions", "next_observations", "dones", "rewards"))
# ... and of its n-step samples (NStepReplayBuffer._get_samples): ``discounts`` multiplies the target Q.
NStepReplaySamples = collections.namedtuple("NStepReplaySamples", ReplaySamples._fields + ("discounts",))

MAX_N_STEPS = 32


def discount_table(gamma, n_steps):
    """``g[j] = float32(float(gamma) ** j)`` for ``j = 0 .. n_steps``: the power in double, rounded once."""
    return [ctypes.c_float(float(gamma) ** j).value for j in range(int(n_steps) + 1)]


class DeviceReplay:
    """A ring of ``R = max(buffer_size // num_envs, 1)`` transitions per env (SB3's
    ``self.buffer_size``) whose observations are ``obs_width = n_stack * D`` floats and whose actions are
    ``act_dim`` floats.

    Buffers (torch tensors on ``device``): ``frames`` [N, R + k - 1, D] (env-major: the frame of env step
    ``c`` is row ``c mod (R + k - 1)``), ``next_frame`` [R, N, D], ``act`` [R, N, A], ``rew`` [R, N]
    float32, ``done`` / ``timeout`` / ``age`` [R, N] uint8 and the per-env counter ``age_now`` [N].

    Preconditions: the windows given to ``put_obs`` evolve by the ``VecFrameStack`` rule with exactly the
    dones given to ``put_step`` (the loop of the module docstring does; the same precondition as
    ``DeviceRollout(n_stack=k)``).  A manual ``wr.reset(obs, mask)`` between stores is not supported:
    ``clear()`` starts over.  ``clear_keeps_sign`` must be the ``DeviceWrappers``' own setting: a slot
    behind an episode boundary is +0.0, or ``frame * 0.0``.  ``n_stack=1`` is plain full storage of an
    unstacked obs.  ``reward_dtype`` is the dtype ``put_step`` will be given.  There is no CPU fallback."""

    def __init__(self, num_envs, buffer_size, obs_width, act_dim, device, reward_dtype=torch.float32, n_stack=1,
                 clear_keeps_sign=False, lib_path=None, n_steps=1, gamma=0.99):
        n, size, W, A, k = int(num_envs), int(buffer_size), int(obs_width), int(act_dim), int(n_stack)
        if n <= 0 or size <= 0 or W <= 0 or A <= 0:
            raise ValueError("num_envs, buffer_size, obs_width and act_dim must be > 0")
        if not 1 <= k <= 32 or W % k != 0:
            raise ValueError("n_stack must be in [1, 32] and divide obs_width")
        if reward_dtype not in (torch.float32, torch.float64):
            raise ValueError("reward_dtype must be torch.float32 or torch.float64")
        self.set_n_steps(n_steps, gamma)
        device = _lib.cuda_device(device, "DeviceReplay")
        self.lib = _lib.load(lib_path)
        R = max(size // n, 1)
        self.n, self.rows, self.w, self.a, self.n_stack, self.d = n, R, W, A, k, W // k
        self.device, self.reward_dtype = device, reward_dtype
        self.clear_keeps_sign = bool(clear_keeps_sign)
        f4, u1 = dict(dtype=torch.float32, device=device), dict(dtype=torch.uint8, device=device)
        self.frames = torch.zeros((n, R + k - 1, self.d), **f4)
        self.next_frame = torch.zeros((R, n, self.d), **f4)
        self.act = torch.zeros((R, n, A), **f4)
        self.rew = torch.zeros((R, n), **f4)
        self.done, self.timeout, self.age = (torch.zeros((R, n), **u1) for _ in range(3))
        self.age_now = torch.full((n,), k - 1, **u1)
        self._bad = torch.zeros(1, dtype=torch.int32, device=device)
        self._puts = self._count = 0                    # put_obs calls; completed transitions
        self._bind()

    def set_n_steps(self, n_steps, gamma):
        """The constructor's ``n_steps`` and ``gamma`` (what ``gather_nstep`` uses), checked, and the
        discount table built from them; nothing stored depends on either."""
        if int(n_steps) != n_steps or not 1 <= n_steps <= MAX_N_STEPS:
            raise ValueError(f"n_steps must be an integer in [1, {MAX_N_STEPS}]")
        if not 0.0 <= float(gamma) <= 1.0:              # (refuses NaN as well)
            raise ValueError("gamma must be in [0, 1]")
        self.n_steps, self.gamma = int(n_steps), float(gamma)
        self._table = (ctypes.c_float * (self.n_steps + 1))(*discount_table(self.gamma, self.n_steps))

    def _bind(self):
        """The C struct over the current buffers (again after a buffer was replaced)."""
        flags = _lib.REPLAY_CLEAR_KEEPS_SIGN if self.clear_keeps_sign else 0
        self._rb = _lib.UsvReplay(self.n, self.rows, self.w, self.a, self.n_stack, self.d, flags, 0, *(t.data_ptr() for t in (
            self.frames, self.next_frame, self.act, self.rew, self.done, self.timeout, self.age, self.age_now, self._bad)))
        self._rp = ctypes.byref(self._rb)

    # ---- SB3's names for the ring position
    @property
    def size(self):
        """Valid transitions per env: ``buffer_size if full else pos``."""
        return min(self._count, self.rows)

    @property
    def pos(self):
        return self._count % self.rows

    @property
    def full(self):
        return self._count >= self.rows

    def _stream(self):
        return _lib.stream_ptr(self.device)

    def _rows(self, name, t):
        """A [N, W] window read in place: its row stride in floats."""
        n, W = self.n, self.w
        if (t.dtype != torch.float32 or tuple(t.shape) != (n, W) or t.device != self.device or
                (W > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < W)):
            raise ValueError(f"{name} must be a float32 tensor of shape {(n, W)} on {self.device} with inner stride 1 "
                             f"and a row stride >= {W}")
        return t.stride(0) if n > 1 else W

    def put_obs(self, stacked, action):
        """The observation the action was computed from and the action (``add``'s ``obs`` and ``action``;
        SB3 stores the action as the policy gave it, scaled to [-1, 1]).  ``stacked`` is [N, W] with
        inner stride 1 and any row stride >= W (``DeviceWrappers.stacked`` is read in place); call it
        before the env step, whose wrapper push overwrites that window's oldest frame."""
        if self._puts != self._count:
            raise RuntimeError("put_obs twice without a put_step in between")
        stride = self._rows("stacked", stacked)
        _lib.check_tensor("action", action, torch.float32, (self.n, self.a), self.device)
        _lib.check(self.lib.usv_replay_put_obs(self._rp, self._puts, _ptr(stacked), stride, _ptr(action), self._stream()),
                   self.lib)
        self._puts += 1

    def put_step(self, rew, term, trunc, next_stack, final_stack):
        """The rest of ``add`` after the env step: reward, ``done = term | trunc``, ``timeout = trunc &
        ~term`` and ``next_obs``: ``final_stack`` [N, W] (``DeviceWrappers.step``'s, SB3's
        ``terminal_observation``) in the rows of done envs, ``next_stack`` (the window after the step,
        e.g. ``wr.stacked``, read in place) elsewhere."""
        if self._puts != self._count + 1:
            raise RuntimeError("put_step needs the put_obs of its step first")
        n = self.n
        _lib.check_tensor("rew", rew, self.reward_dtype, (n,), self.device)
        for name, m in (("term", term), ("trunc", trunc)):
            if m.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"{name} must be a bool or uint8 tensor")
            _lib.check_tensor(name, m, m.dtype, (n,), self.device)
        stride = self._rows("next_stack", next_stack)
        _lib.check_tensor("final_stack", final_stack, torch.float32, (n, self.w), self.device)
        _lib.check(self.lib.usv_replay_put_step(self._rp, self._count, _ptr(rew), 4 if self.reward_dtype == torch.float32 else 8,
                                                _ptr(term), _ptr(trunc), _ptr(next_stack), stride, _ptr(final_stack),
                                                self._stream()), self.lib)
        self._count += 1

    def gather(self, idx, out=None):
        """SB3's ``ReplayBuffer._get_samples`` in one launch: the transitions at the flat indices ``idx``
        (int64 [B] on the device, ``slot * N + e`` with ``slot`` in ``[0, size)``) as a ``ReplaySamples``
        of ``observations`` [B, W], ``actions`` [B, A], ``next_observations`` [B, W], ``dones`` [B, 1]
        (``done * (1 - timeout)``) and ``rewards`` [B, 1].  The outputs are fresh tensors, or those of
        ``out`` (contiguous float32 tensors of these shapes).  Runs on the current stream without a host
        sync.  An index outside ``[0, size * N)`` is not dereferenced: its outputs are NaN and
        ``bad_indices()`` counts it.  Refused between a ``put_obs`` and its ``put_step``: the frame row
        just written is the one the oldest valid window still needs."""
        if self._puts != self._count:
            raise RuntimeError("gather between put_obs and put_step: finish the step first")
        B = int(idx.shape[0]) if idx.dim() == 1 else 0
        if idx.dtype != torch.int64 or not 0 < B < 2 ** 31 or idx.device != self.device:
            raise ValueError(f"idx must be a non-empty 1-D int64 tensor (below 2^31 indices) on {self.device}")
        idx = idx.contiguous()
        shapes = ((B, self.w), (B, self.a), (B, self.w), (B, 1), (B, 1))
        if out is None:
            out = ReplaySamples(*(torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes))
        else:
            for name, t, s in zip(ReplaySamples._fields, out, shapes):
                _lib.check_tensor(f"out.{name}", t, torch.float32, s, self.device)
        _lib.check(self.lib.usv_replay_gather(self._rp, self._count, _ptr(idx), B, *(_ptr(t) for t in out),
                                              self._stream()), self.lib)
        return out if isinstance(out, ReplaySamples) else ReplaySamples(*out)

    def sample(self, batch_size, generator=None):
        """SB3's ``ReplayBuffer.sample``: one ``torch.randint(0, size * N)`` on the device (``generator``:
        a device generator), uniform over (row, env) pairs as SB3's two ``randint``s are, then
        ``gather``."""
        batch_size = int(batch_size)
        if batch_size <= 0:
            raise ValueError("batch_size must be > 0")
        if self.size == 0:
            raise RuntimeError("sample from an empty buffer")
        idx = torch.randint(0, self.size * self.n, (batch_size,), device=self.device, generator=generator)
        return self.gather(idx)

    def gather_nstep(self, idx, out=None):
        """SB3's ``NStepReplayBuffer._get_samples`` (2.7: ``n_steps`` of SAC / TD3 / DQN) in one launch, with
        the constructor's ``n_steps`` and ``gamma``: an ``NStepReplaySamples`` whose ``observations`` and
        ``actions`` are those of ``gather(idx)``.  The run of a sample walks up to ``n_steps`` transitions
        of its env and ends at the first that is done or timed out, or at the newest one stored (it crosses
        neither the write position nor unwritten rows).  ``rewards`` [B, 1] is the discounted sum of the
        run's rewards, ``next_observations`` and ``dones`` are those of its last transition (the window
        rebuilt from the frame ring under that transition's own liveness), and ``discounts`` [B, 1] is
        ``gamma ** (transitions in the run)``: the target is ``rewards + (1 - dones) * discounts * q_next``.
        tests/replay_nstep_ref.py is the definition, met bit for bit: the table ``float32(gamma ** j)`` is
        built once on the host with the power taken in double, and the sum is float32 in the order of the
        steps, each product and each sum rounded on its own; a run of one transition returns the stored
        reward's bits.  Two differences from SB3: it takes ``gamma ** float32`` in float32 (within 1 ulp of
        the table: about 6e-8 on ``discounts``, at most 4.8e-7 observed on returns of unit-normal rewards),
        and it adds the terms behind the run's end as ``+0.0``, which shows only for a return of ``-0.0``
        (NumPy's own order of summation also differs from ``n_steps = 8`` on).  ``out``, bad indices, the
        stream and the call order are as in ``gather``; there is no host sync."""
        if self._puts != self._count:
            raise RuntimeError("gather_nstep between put_obs and put_step: finish the step first")
        B = int(idx.shape[0]) if idx.dim() == 1 else 0
        if idx.dtype != torch.int64 or not 0 < B < 2 ** 31 or idx.device != self.device:
            raise ValueError(f"idx must be a non-empty 1-D int64 tensor (below 2^31 indices) on {self.device}")
        idx = idx.contiguous()
        shapes = ((B, self.w), (B, self.a), (B, self.w), (B, 1), (B, 1), (B, 1))
        if out is None:
            out = NStepReplaySamples(*(torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes))
        else:
            for name, t, s in zip(NStepReplaySamples._fields, out, shapes):
                _lib.check_tensor(f"out.{name}", t, torch.float32, s, self.device)
        _lib.check(self.lib.usv_replay_gather_nstep(self._rp, self._count, _ptr(idx), B, self.n_steps, self._table,
                                                    *(_ptr(t) for t in out), self._stream()), self.lib)
        return out if isinstance(out, NStepReplaySamples) else NStepReplaySamples(*out)

    def sample_nstep(self, batch_size, generator=None):
        """``sample`` for n-step returns: the same one device ``randint``, then ``gather_nstep``."""
        batch_size = int(batch_size)
        if batch_size <= 0:
            raise ValueError("batch_size must be > 0")
        if self.size == 0:
            raise RuntimeError("sample from an empty buffer")
        idx = torch.randint(0, self.size * self.n, (batch_size,), device=self.device, generator=generator)
        return self.gather_nstep(idx)

    def clear(self):
        """Start over: the next ``put_obs`` is step 0 and stores its whole window.  ``bad_indices`` keeps
        counting."""
        self.age_now.fill_(self.n_stack - 1)
        self._puts = self._count = 0

    def nbytes(self):
        """Bytes of the ring's device buffers."""
        return sum(t.numel() * t.element_size() for t in (self.frames, self.next_frame, self.act, self.rew, self.done,
                                                          self.timeout, self.age, self.age_now))

    def bad_indices(self):
        """How many indices ``gather`` has refused since this object was built, as a Python int (one
        host copy: the only sync of this class)."""
        return int(self._bad.item())
