"""Torch-native SAC on the HIP vector env with the device replay buffer: the reference's off-policy
trainer without stable-baselines3.

The reference trains ``SAC("MlpPolicy", VecFrameStack(env, 5), **config_sac)``
(train_test/sb3_train_vec.py:58-72, train_test/config.py:17-37).  SB3 is absent from this image, so this
is a compact SAC with config_sac's hyper-parameters where they carry over:

* twin Q networks and a tanh-Gaussian actor, ``net_arch=[400, 300]``, ReLU; Polyak-averaged target
  critics (SB3's tau 0.005); ``gamma=0.99``, ``learning_rate=1e-4``, ``batch_size=256``,
  ``train_freq=8``, ``gradient_steps=8``, ``buffer_size=400000``, ``ent_coef='auto'`` (log-coefficient
  learned towards the target entropy ``-act_dim``, initial value 1);
* the frame stack and the episode statistics are ``DeviceWrappers`` (one HIP launch behind the step);
* ``device_replay=True``: the replay buffer is ``gym_usv_amd.DeviceReplay``: one 143-float frame of obs
  and of next_obs per transition where full storage keeps two 715-float stacks, and one launch per
  minibatch that rebuilds both windows (``sample`` = one device ``randint`` + ``gather``);
  ``device_replay=False``: a torch full-storage buffer (two ``[R, N, W]`` tensors, row copies to store,
  indexed reads to sample);
* ``check_replay=True`` keeps both and asserts that every minibatch of the two is bitwise equal (the
  assertion reads one flag per minibatch back to the host: a test mode);
* ``n_steps=N`` (``--n-steps N``): SB3 2.7's n-step returns.  A minibatch is ``gather_nstep``'s: the
  discounted sum of up to ``N`` rewards, the ``next_observations`` and ``dones`` at the end of that run and a
  per-sample ``discounts``, and the target is ``rewards + (1 - dones) * discounts * q_next``.  With the
  default 1 that is the one-step target (``discounts`` is ``float32(gamma)`` everywhere).  The torch buffer
  computes the same with three indexed reads per step of the run and six more per minibatch.

* ``sde_kernel=True`` (``--sde-kernel``): config_sac's ``use_sde=True``, ``sde_sample_freq=4``,
  ``log_std_init=-3`` through ``gym_usv_amd.DeviceSDE.squashed`` (one HIP launch forward, two backward, no
  exploration matrix in memory): the actor's ``log_std`` is a ``[300, 2]`` parameter, ``mu`` passes through
  ``hardtanh(+-2)`` (SB3's ``clip_mean``), one head of ``envs`` rows collects with a new noise epoch every
  fourth step and its ``env_actions`` feed ``env.step``, and a second head of ``batch_size`` rows with another
  seed serves both actor calls of a gradient step under one epoch, as ``SAC.train``'s ``reset_noise`` does.
  Without it the actor's noise is torch's (a state-independent tanh-Gaussian) and nothing here changes.
* ``loss_kernel=True`` (``--loss-kernel``): the TD target with the twin-critic loss, the actor loss with the
  entropy-coefficient loss, and ``polyak_update`` through ``gym_usv_amd.DeviceSACLoss`` / ``DevicePolyak``: one HIP
  launch each forward, one each backward, in place of torch's op-by-op graphs and the 24 launches of the two-op
  Polyak loop.  The entropy optimizer then steps after the actor loss's backward (one backward serves both
  losses); ``ent`` is read before it either way, so the algorithm is SB3's.
* ``check_loss=True`` (``--check-loss``, with ``loss_kernel``) also evaluates the torch lines on every gradient step
  and records the largest differences of the three losses, each over the sum of the magnitudes of its terms, and
  of Polyak against the torch two-op update of a cloned target (read back once per round: a test mode).
* ``caps=True`` (``--caps``): config_sac's ``lambda_t=10``, ``lambda_s=5``, ``eps_s=0.1``, the CAPS regulariser of the
  SB3 fork the reference trains with (Mysore et al., ICRA 2021): the actor loss gains ``lambda_t * L_T + lambda_s *
  L_S`` with ``L_T = ||pi(s) - pi(s')||_2`` and ``L_S = ||pi(s) - pi(s + eps_s * z)||_2``, ``z ~ N(0, I)``, averaged over
  the minibatch; pi is the deterministic action, ``tanh(hardtanh(mu))`` with ``sde_kernel`` and ``tanh(mu)`` without.
  The mean at ``s`` is the one the actor forward behind ``a_pi`` computes; one more forward takes the ``2 B`` rows of
  ``s'`` and the perturbed ``s``.  In torch lines (``randn_like``, ``linalg.vector_norm``) unless
* ``caps_kernel=True`` (``--caps-kernel``, with ``caps``) routes it through ``gym_usv_amd.DeviceCAPS``: one launch for
  the perturbed observations (counter-based noise, a new epoch every gradient step), one for both terms with their
  gradients, one backward.  ``check_caps=True`` (``--check-caps``, with ``caps_kernel``) also evaluates the torch lines
  on the kernel's own perturbed observations and records the largest difference of the loss over the loss (read back
  once per round: a test mode).  The temporal term needs the one-step successor: ``caps`` with ``n_steps`` other than 1
  is a ``ValueError``.
* ``adam_kernel=True`` (``--adam-kernel``): the three optimizers (critic, actor, the one-element ``log_ent``) are
  ``gym_usv_amd.DeviceAdam``, one HIP launch per ``step()`` over the whole parameter list in place of torch's Adam ops,
  with torch's arithmetic up to rounding.  Nothing else changes.

* ``graph=True`` (``--graph``; needs ``device_replay``, ``sde_kernel``, ``loss_kernel`` and ``adam_kernel``, with ``caps`` also
  ``caps_kernel``, and neither ``check_loss`` nor ``check_caps``; anything else is a ``ValueError`` at start): a gradient
  step is recorded once as a HIP graph (``gym_usv_amd.capture_step``) and replayed.  Per gradient step the ``randint`` and
  the one replay gather launch stay eager, the gather writing straight into static minibatch tensors; one ``replay()``
  covers the rest: both ``reset_noise()`` calls, the critic step, the actor and entropy-coefficient step with CAPS, three
  ``DeviceAdam.step()`` calls and ``DevicePolyak.step()``.  The trainer objects are then made with ``capturable=True`` (their
  step and noise counters live in device memory).  The warm-up and capture calls run on the first minibatch and are
  undone (parameters, optimizer state and noise epochs are put back), so the run takes the gradient steps of the run
  without ``graph``; the logged losses are read from the graph's static outputs after each replay.

``learning_starts`` counts vector steps here (SB3 counts transitions: 50 000 of them are 12 steps of 4096 envs).  The loop
collects ``train_freq`` steps, then takes ``gradient_steps`` gradient steps, as SB3's ``learn`` does.
Whole runs of the two buffer modes are two samples of one algorithm: torch's own kernels need not be
bitwise reproducible.

    python examples/sac_torch.py --envs 4096 --steps 400 --device-replay
    python examples/sac_torch.py --envs 4096 --steps 400 --device-replay --sde-kernel
    python examples/sac_torch.py --envs 4096 --steps 400 --device-replay --sde-kernel --loss-kernel
    python examples/sac_torch.py --envs 4096 --steps 400 --device-replay --sde-kernel --loss-kernel --caps --caps-kernel
    python examples/sac_torch.py --envs 4096 --steps 400 --device-replay --sde-kernel --loss-kernel --caps --caps-kernel \
        --adam-kernel --graph
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gym-usv_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CONFIG_SAC = {"n_stack": 5, "net_arch": (400, 300), "lr": 1e-4, "gamma": 0.99, "tau": 0.005, "buffer_size": 400000,
              "batch_size": 256, "train_freq": 8, "gradient_steps": 8, "learning_starts": 12,
              "n_steps": 1,                                         # SB3 2.7's n_steps (config_sac has none: 1)
              "sde_sample_freq": 4, "log_std_init": -3.0,             # these two: sde_kernel=True only
              "lambda_t": 10.0, "lambda_s": 5.0, "eps_s": 0.1}        # CAPS (config.py:34-36): caps=True only
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0   # SB3 sac/policies.py
CLIP_MEAN = 2.0                         # SB3 sac/policies.py, with use_sde


def mlp(inp, hidden, out):
    layers, d = [], inp
    for h in hidden:
        layers += [nn.Linear(d, h), nn.ReLU()]
        d = h
    return nn.Sequential(*layers, nn.Linear(d, out))


class Actor(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden, sde_log_std_init=None):
        super().__init__()
        self.body = mlp(obs_dim, hidden[:-1], hidden[-1])
        if sde_log_std_init is None:
            self.mu, self.log_std = nn.Linear(hidden[-1], act_dim), nn.Linear(hidden[-1], act_dim)
        else:                                               # gSDE: log_std [latent, act_dim] is a parameter
            self.mu = nn.Linear(hidden[-1], act_dim)
            self.log_std = nn.Parameter(torch.full((hidden[-1], act_dim), float(sde_log_std_init)))

    def sde(self, obs, head):
        """gSDE through ``head.squashed``: its ``SquashedSample`` (actions in [-1, 1], Box actions,
        log-probability, Gaussian actions) and the mean.  StateDependentNoiseDistribution, squash_output,
        learn_features."""
        h = F.relu(self.body(obs))
        mean = F.hardtanh(self.mu(h), -CLIP_MEAN, CLIP_MEAN)
        return head.squashed(mean, h, self.log_std.exp()), mean

    def forward(self, obs):
        """(action in [-1, 1], its log-probability, the mean): SquashedDiagGaussianDistribution, epsilon 1e-6."""
        h = F.relu(self.body(obs))
        mu, log_std = self.mu(h), self.log_std(h).clamp(LOG_STD_MIN, LOG_STD_MAX)
        std = log_std.exp()
        u = mu + std * torch.randn_like(mu)
        a = torch.tanh(u)
        logp = (-0.5 * ((u - mu) / std) ** 2 - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
        return a, logp - torch.log(1 - a * a + 1e-6).sum(-1), mu

    def mean(self, obs):
        """The pre-squash mean of the deterministic action ``tanh(mean)``, as ``sde`` / ``forward`` compute it."""
        mu = self.mu(F.relu(self.body(obs)))
        return F.hardtanh(mu, -CLIP_MEAN, CLIP_MEAN) if isinstance(self.log_std, nn.Parameter) else mu


class Critic(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden):
        super().__init__()
        self.q1, self.q2 = mlp(obs_dim + act_dim, hidden, 1), mlp(obs_dim + act_dim, hidden, 1)

    def forward(self, obs, act):
        x = torch.cat((obs, act), -1)
        return self.q1(x), self.q2(x)


class TorchReplay:
    """Full storage in torch: what a trainer writes without ``DeviceReplay``."""

    def __init__(self, n, buffer_size, W, A, device):
        self.n, self.rows = n, max(buffer_size // n, 1)
        z = lambda *s: torch.zeros(s, device=device)    # noqa: E731
        R = self.rows
        self.obs, self.next_obs, self.act = z(R, n, W), z(R, n, W), z(R, n, A)
        self.rew, self.done, self.timeout = z(R, n), z(R, n), z(R, n)
        self.count, self._tables = 0, {}

    @property
    def size(self):
        return min(self.count, self.rows)

    def put_obs(self, stacked, action):
        p = self.count % self.rows
        self.obs[p], self.act[p] = stacked, action

    def put_step(self, rew, term, trunc, next_stack, final_stack):
        p = self.count % self.rows
        done = term.bool() | trunc.bool()
        self.next_obs[p] = torch.where(done[:, None], final_stack, next_stack)
        self.rew[p], self.done[p] = rew.float(), done.float()
        self.timeout[p] = (trunc.bool() & ~term.bool()).float()
        self.count += 1

    def gather(self, idx):
        from gym_usv_amd.replay import ReplaySamples
        W, A = self.obs.shape[-1], self.act.shape[-1]
        dones = (self.done.reshape(-1)[idx] * (1 - self.timeout.reshape(-1)[idx])).reshape(-1, 1)
        return ReplaySamples(self.obs.reshape(-1, W)[idx], self.act.reshape(-1, A)[idx], self.next_obs.reshape(-1, W)[idx],
                             dones, self.rew.reshape(-1)[idx].reshape(-1, 1))

    def gather_nstep(self, idx, n_steps, table):
        """SB3's ``NStepReplayBuffer._get_samples`` as ``DeviceReplay.gather_nstep`` defines it: ``table`` is
        its ``discount_table(gamma, n_steps)``, the return the float32 sum in the order of the steps (one
        multiply and one add per step: eager torch fuses neither), a run of one step the stored reward."""
        from gym_usv_amd.replay import NStepReplaySamples
        n, R, W, A = self.n, self.rows, self.obs.shape[-1], self.act.shape[-1]
        slot, e = idx // n, idx % n
        last = (self.count - 1) % R
        rew, done, timeout = self.rew.reshape(-1), self.done.reshape(-1), self.timeout.reshape(-1)
        is_open = torch.ones_like(idx, dtype=torch.bool)
        ret, end = torch.zeros_like(idx, dtype=torch.float32), idx.clone()      # `end`: the run's last transition
        m = torch.zeros_like(idx)
        for j in range(n_steps):
            s = (slot + j) % R
            f = s * n + e
            ret = torch.where(is_open, rew[f] if j == 0 else ret + rew[f] * table[j], ret)
            end, m = torch.where(is_open, f, end), torch.where(is_open, j, m)
            is_open = is_open & (done[f] == 0) & (timeout[f] == 0) & (s != last)
        dones = (done[end] * (1 - timeout[end])).reshape(-1, 1)
        key = tuple(table)
        if key not in self._tables:                         # uploaded once per table
            self._tables[key] = torch.tensor(table, dtype=torch.float32, device=idx.device)
        discounts = self._tables[key][m + 1].reshape(-1, 1)
        return NStepReplaySamples(self.obs.reshape(-1, W)[idx], self.act.reshape(-1, A)[idx],
                                  self.next_obs.reshape(-1, W)[end], dones, ret.reshape(-1, 1), discounts)


class SAC:
    def __init__(self, env, seed=0, device_replay=True, check_replay=False, sde_kernel=False, loss_kernel=False,
                 check_loss=False, caps=False, caps_kernel=False, check_caps=False, adam_kernel=False, graph=False, **cfg):
        from gym_usv_amd import DeviceAdam, DeviceCAPS, DevicePolyak, DeviceReplay, DeviceSACLoss, DeviceSDE
        from gym_usv_amd.replay import discount_table
        from gym_usv_amd.wrappers import DeviceWrappers
        self.cfg = c = dict(CONFIG_SAC, **cfg)
        self.env, self.device = env, env.device
        self.N, D, A, k = env.num_envs, env.obs_dim, env.act_dim, c["n_stack"]
        W = k * D
        torch.manual_seed(seed)
        d = self.device
        self.actor = Actor(W, A, c["net_arch"], c["log_std_init"] if sde_kernel else None).to(d)
        self.critic, self.target = Critic(W, A, c["net_arch"]).to(d), Critic(W, A, c["net_arch"]).to(d)
        self.target.load_state_dict(self.critic.state_dict())
        self.log_ent = torch.zeros(1, device=d, requires_grad=True)      # ent_coef 'auto': initial value 1
        self.target_entropy = -float(A)
        check_graph_args(graph, device_replay, sde_kernel, loss_kernel, adam_kernel, caps, caps_kernel, check_loss,
                         check_caps)
        self.graph, self.captured, self.static_mb = graph, None, None
        cap = {"capturable": True} if graph else {}         # counters in device memory: a replayed step counts
        adam = DeviceAdam if adam_kernel else torch.optim.Adam      # the same calls either way: zero_grad, step
        self.opt_a = adam(self.actor.parameters(), lr=c["lr"], **cap)
        self.opt_c = adam(self.critic.parameters(), lr=c["lr"], **cap)
        self.opt_e = adam([self.log_ent], lr=c["lr"], **cap)
        lo, hi = env.single_action_space.low, env.single_action_space.high
        self.a_lo = torch.as_tensor(lo, device=d, dtype=torch.float32)
        self.a_hi = torch.as_tensor(hi, device=d, dtype=torch.float32)
        self.head_env = self.head_mb = None
        if sde_kernel:      # rows = global env ids / positions in the minibatch; seeds other than the env's
            self.head_env = DeviceSDE(self.N, c["net_arch"][-1], A, d, seed + 1, lo, hi)
            self.head_mb = DeviceSDE(c["batch_size"], c["net_arch"][-1], A, d, seed + 2, lo, hi, **cap)
        self.sde_steps = 0
        if check_loss and not loss_kernel:
            raise ValueError("check_loss compares the loss kernels with torch: it needs loss_kernel=True")
        self.loss = self.polyak = None
        if loss_kernel:
            self.loss = DeviceSACLoss(d)
            self.polyak = DevicePolyak(list(self.critic.parameters()), list(self.target.parameters()))
        self.check_loss, self.losses_checked = check_loss, 0
        self.loss_diff = torch.zeros(5, device=d)           # critic, actor, ent_coef, Polyak |diff|, Polyak ratio
        check_caps_args(caps, caps_kernel, check_caps, c["n_steps"])
        self.caps, self.caps_dev, self.check_caps, self.caps_checked = caps, None, check_caps, 0
        if caps_kernel:                                     # rows = positions in the minibatch; its own seed
            self.caps_dev = DeviceCAPS(d, seed + 3, c["lambda_t"], c["lambda_s"], c["eps_s"], squash=True, **cap)
        self.caps_diff = torch.zeros((), device=d)
        self.wr = DeviceWrappers(self.N, D, k, d, env.reward.dtype)
        self.rb = self.shadow = None
        if device_replay or check_replay:
            self.rb = DeviceReplay(self.N, c["buffer_size"], W, A, d, env.reward.dtype, n_stack=k, n_steps=c["n_steps"],
                                   gamma=c["gamma"])
        if not device_replay or check_replay:
            self.shadow = TorchReplay(self.N, c["buffer_size"], W, A, d)
        self.device_replay = device_replay
        self.table = discount_table(c["gamma"], c["n_steps"])
        obs, _ = env.reset(seed=seed)
        self.wr.reset(obs)
        self.env_steps = self.checked = 0
        self._totals = (0.0, 0, 0)

    @torch.no_grad()
    def collect(self, steps, random_actions):
        for _ in range(steps):
            obs = self.wr.stacked                           # the ring's window, no clone
            a_env = None
            if random_actions:                              # SB3: uniform actions before learning_starts
                a = torch.rand((self.N, self.a_lo.numel()), device=self.device) * 2 - 1
            elif self.head_env is not None:
                if self.sde_steps % self.cfg["sde_sample_freq"] == 0:
                    self.head_env.reset_noise()
                self.sde_steps += 1
                s, _ = self.actor.sde(obs, self.head_env)   # the head's buffers: consumed before its next call
                a, a_env = s.actions, s.env_actions
            else:
                a, _, _ = self.actor(obs)
            for buf in (self.rb, self.shadow):
                if buf is not None:
                    buf.put_obs(obs, a)
            if a_env is None:
                a_env = self.a_lo + (a + 1) * 0.5 * (self.a_hi - self.a_lo)   # unscale_action
            o, rew, term, trunc, info = self.env.step(a_env)
            stacked, final_stack, _ = self.wr.step(o, rew, info["_final_obs"], info["final_obs"])
            for buf in (self.rb, self.shadow):
                if buf is not None:
                    buf.put_step(rew, term, trunc, stacked, final_stack)
            self.env_steps += self.N

    def minibatch(self):
        c = self.cfg
        size = self.rb.size if self.rb is not None else self.shadow.size
        idx = torch.randint(0, size * self.N, (c["batch_size"],), device=self.device)
        legs = (lambda: self.rb.gather_nstep(idx, out=self.static_mb), lambda: self.shadow.gather_nstep(idx, c["n_steps"], self.table))
        mb = legs[0 if self.device_replay else 1]()
        if self.rb is not None and self.shadow is not None:
            other = legs[1 if self.device_replay else 0]()
            for name, x, y in zip(mb._fields, mb, other):
                assert x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), \
                    f"minibatch field {name} differs between DeviceReplay and the torch buffer"
            self.checked += 1
        return mb

    def policy(self, obs):
        """(action, log-probability, mean) of the update's actor calls."""
        if self.head_mb is None:
            return self.actor(obs)
        s, mean = self.actor.sde(obs, self.head_mb)
        return s.actions, s.log_prob, mean

    @staticmethod
    def smooth_lines(m, m2, m3, lambda_t, lambda_s):
        """CAPS in torch lines from the three pre-squash means: (loss, temporal, spatial)."""
        a = torch.tanh(m)
        temporal = torch.linalg.vector_norm(a - torch.tanh(m2), dim=-1).mean()
        spatial = torch.linalg.vector_norm(a - torch.tanh(m3), dim=-1).mean()
        return lambda_t * temporal + lambda_s * spatial, temporal.detach(), spatial.detach()

    def smooth(self, mb, m):
        """The CAPS term of a gradient step, (loss, temporal, spatial), from the mean ``m`` at ``mb.observations``:
        one actor forward over the 2 B rows of the next and the perturbed observations."""
        c = self.cfg
        if self.caps_dev is not None:
            self.caps_dev.reset_noise()
            near = self.caps_dev.near(mb.observations)
        else:
            near = mb.observations + c["eps_s"] * torch.randn_like(mb.observations)
        m2, m3 = self.actor.mean(torch.cat((mb.next_observations, near))).chunk(2)
        if self.caps_dev is None:
            return self.smooth_lines(m, m2, m3, c["lambda_t"], c["lambda_s"])
        s = self.caps_dev.loss(m, m2, m3)
        if self.check_caps:
            with torch.no_grad():
                ref = self.smooth_lines(m, m2, m3, c["lambda_t"], c["lambda_s"])[0]
                diff = (s.loss - ref).abs()
                r = torch.where(ref > 0, diff / ref, diff * float("inf")).nan_to_num(nan=0.0)   # as _worst
                self.caps_diff = torch.maximum(self.caps_diff, r)
            self.caps_checked += 1
        return s.loss, s.temporal, s.spatial

    def kernel_step(self, mb, a_pi, logp, ent, smooth=None):
        """The rest of a gradient step through the loss kernels: (actor_loss, critic_loss, ent_coef_loss)."""
        c = self.cfg
        with torch.no_grad():
            a2, logp2, _ = self.policy(mb.next_observations)
            q1n, q2n = self.target(mb.next_observations, a2)
        q1, q2 = self.critic(mb.observations, mb.actions)
        cl = self.loss.critic(q1, q2, q1n, q2n, mb.rewards, mb.dones, ent_coef=ent, logp_next=logp2,
                              discounts=mb.discounts)
        if self.check_loss:
            self.compare_critic(cl, q1, q2, q1n, q2n, logp2, mb, ent)
        self.opt_c.zero_grad(set_to_none=True)
        cl.loss.backward()
        self.opt_c.step()
        q1p, q2p = self.critic(mb.observations, a_pi)
        pl = self.loss.policy(logp, q1p, q2p, ent, log_ent_coef=self.log_ent, target_entropy=self.target_entropy)
        if self.check_loss:
            self.compare_policy(pl, logp, q1p, q2p, ent)
        self.opt_a.zero_grad(set_to_none=True)
        self.opt_e.zero_grad(set_to_none=True)
        total = pl.actor_loss + pl.ent_coef_loss
        if smooth is not None:
            total = total + smooth
        total.backward()                                    # one backward launch for logp, both q's and log_ent
        self.opt_a.step()
        self.opt_e.step()
        ref = None
        if self.check_loss:                                 # the torch two-op update of a cloned target
            with torch.no_grad():
                ref = [(t.clone(), t * (1 - c["tau"]), c["tau"] * p) for p, t in zip(self.critic.parameters(),
                                                                                     self.target.parameters())]
                for (t, _, _), p in zip(ref, self.critic.parameters()):
                    t.mul_(1 - c["tau"]).add_(p, alpha=c["tau"])
        self.polyak.step(c["tau"])
        if ref is not None:
            with torch.no_grad():
                diff = torch.cat([(t - r).abs().flatten() for t, (r, _, _) in zip(self.target.parameters(), ref)])
                size = torch.cat([(a.abs() + b.abs()).flatten() for _, a, b in ref])
                self._worst(3, diff.max(), 1.0)
                self._worst(4, torch.where(size > 0, diff / size, diff * float("inf")).nan_to_num(nan=0.0).max(), 1.0)
            self.losses_checked += 1
        return pl.actor_loss.detach(), cl.loss.detach(), pl.ent_coef_loss.detach()

    def _worst(self, at, diff, scale):
        scale = torch.as_tensor(scale, device=diff.device, dtype=diff.dtype)
        r = torch.where(scale > 0, diff / scale, diff * float("inf")).nan_to_num(nan=0.0)   # a zero scale wants a zero diff
        self.loss_diff[at] = torch.maximum(self.loss_diff[at], r.detach())

    @torch.no_grad()
    def compare_critic(self, cl, q1, q2, q1n, q2n, logp2, mb, ent):
        """The torch lines of the critic loss on the same tensors; the difference over the sum of magnitudes."""
        q_next = torch.min(q1n, q2n) - ent * logp2[:, None]
        target = mb.rewards + (1 - mb.dones) * mb.discounts * q_next
        loss = 0.5 * (F.mse_loss(q1, target) + F.mse_loss(q2, target))
        n = mb.rewards.abs() + ((1 - mb.dones) * mb.discounts).abs() * (torch.min(q1n, q2n).abs() + (ent * logp2[:, None]).abs())
        scale = 0.5 * (((q1.abs() + n) ** 2).mean() + ((q2.abs() + n) ** 2).mean())
        self._worst(0, (cl.loss - loss).abs(), scale)

    @torch.no_grad()
    def compare_policy(self, pl, logp, q1p, q2p, ent):
        q_pi = torch.min(q1p, q2p)
        actor = (ent * logp[:, None] - q_pi).mean()
        ent_loss = -(self.log_ent * (logp + self.target_entropy)).mean()
        self._worst(1, (pl.actor_loss - actor).abs(), ((ent * logp[:, None]).abs() + q_pi.abs()).mean())
        self._worst(2, (pl.ent_coef_loss - ent_loss).abs(),
                    self.log_ent.abs().squeeze() * (logp.abs() + abs(self.target_entropy)).mean())

    def gradient_step(self, mb):
        """One gradient step on ``mb`` behind the minibatch; with the loss kernels its statistics, one tensor (what
        ``graph=True`` records and replays), otherwise what the torch lines of ``train`` go on from."""
        if self.head_mb is not None:
            self.head_mb.reset_noise()                      # SAC.train: one matrix per gradient step
        a_pi, logp, mean = self.policy(mb.observations)
        ent = self.log_ent.detach().exp()
        smooth, extra = None, ()
        if self.caps:
            smooth, *extra = self.smooth(mb, mean)
        if self.loss is None:
            return a_pi, logp, ent, smooth, extra
        actor_loss, critic_loss, ent_loss = self.kernel_step(mb, a_pi, logp, ent, smooth)
        return torch.stack((actor_loss, critic_loss, ent.squeeze(), ent_loss, *extra))

    def capture(self, mb):
        """Records ``gradient_step`` on the static minibatch ``mb``.  The warm-up and capture calls train on it: what
        they changed is put back, so the first replay is the run's first gradient step."""
        from gym_usv_amd import capture_step
        opts = (self.opt_a, self.opt_c, self.opt_e)
        nets = [p for m in (self.actor, self.critic, self.target) for p in m.parameters()] + [self.log_ent]
        kept = [p.detach().clone() for p in nets]
        states = [o.state_dict() for o in opts]
        epochs = [x.epoch for x in (self.head_mb, self.caps_dev) if x is not None]
        self.static_mb = mb
        self.captured = capture_step(lambda: self.gradient_step(mb))
        with torch.no_grad():
            for p, k in zip(nets, kept):
                p.copy_(k)                                  # in place: the graph holds the addresses
        for o, sd in zip(opts, states):
            o.load_state_dict(sd)
        for x, e in zip([x for x in (self.head_mb, self.caps_dev) if x is not None], epochs):
            x.epoch = e

    def train(self, gradient_steps):
        c, stats = self.cfg, []
        for _ in range(gradient_steps):
            mb = self.minibatch()
            if self.graph:
                if self.captured is None:
                    self.capture(mb)                        # from here on minibatch() gathers into mb's tensors
                stats.append(self.captured.replay().clone())    # the static output, before the next replay rewrites it
                continue
            out = self.gradient_step(mb)
            if self.loss is not None:
                stats.append(out)
                continue
            a_pi, logp, ent, smooth, extra = out
            ent_loss = -(self.log_ent * (logp.detach() + self.target_entropy)).mean()
            self.opt_e.zero_grad(set_to_none=True)
            ent_loss.backward()
            self.opt_e.step()
            with torch.no_grad():
                a2, logp2, _ = self.policy(mb.next_observations)
                q_next = torch.min(*self.target(mb.next_observations, a2)) - ent * logp2[:, None]
                target = mb.rewards + (1 - mb.dones) * mb.discounts * q_next
            q1, q2 = self.critic(mb.observations, mb.actions)
            critic_loss = 0.5 * (F.mse_loss(q1, target) + F.mse_loss(q2, target))
            self.opt_c.zero_grad(set_to_none=True)
            critic_loss.backward()
            self.opt_c.step()
            q_pi = torch.min(*self.critic(mb.observations, a_pi))
            actor_loss = (ent * logp[:, None] - q_pi).mean()
            self.opt_a.zero_grad(set_to_none=True)
            (actor_loss if smooth is None else actor_loss + smooth).backward()
            self.opt_a.step()
            with torch.no_grad():                           # polyak_update
                for p, t in zip(self.critic.parameters(), self.target.parameters()):
                    t.mul_(1 - c["tau"]).add_(p, alpha=c["tau"])
            stats.append(torch.stack((actor_loss.detach(), critic_loss.detach(), ent.squeeze(), ent_loss.detach(), *extra)))
        s = torch.stack(stats).mean(0).tolist()
        out = {"actor_loss": s[0], "critic_loss": s[1], "ent_coef": s[2], "ent_coef_loss": s[3]}
        if self.caps:                                       # the regulariser's two terms, unweighted
            out["caps_temporal"], out["caps_spatial"] = s[4], s[5]
        if self.check_caps:
            out["caps_diff"], out["caps_checked"] = self.caps_diff.item(), self.caps_checked
        if self.check_loss:                                 # the largest so far, one read per round
            out["loss_diff"] = dict(zip(("critic", "actor", "ent_coef", "polyak_abs", "polyak_ratio"), self.loss_diff.tolist()))
            out["losses_checked"] = self.losses_checked
        if self.head_mb is not None:                        # of the round's last gradient step
            ls = self.actor.log_std
            out["log_std_mean"], out["log_std_move_abs_max"], out["log_std_grad_abs_max"] = torch.stack(
                (ls.detach().mean(), (ls.detach() - c["log_std_init"]).abs().max(), ls.grad.abs().max())).tolist()
        return out

    def episode_stats(self):
        now, was = self.wr.totals(), self._totals
        self._totals = now
        eps = now[1] - was[1]
        if eps == 0:
            return {"episodes": 0}
        return {"episodes": eps, "ep_rew_mean": (now[0] - was[0]) / eps, "ep_len_mean": (now[2] - was[2]) / eps}


def check_caps_args(caps, caps_kernel, check_caps, n_steps):
    if caps_kernel and not caps:
        raise ValueError("caps_kernel routes the CAPS regulariser through DeviceCAPS: it needs caps=True")
    if check_caps and not caps_kernel:
        raise ValueError("check_caps compares DeviceCAPS with torch: it needs caps_kernel=True")
    if caps and n_steps != 1:
        raise ValueError("caps needs n_steps=1: the temporal term takes the one-step successor, which an n-step "
                         "sample does not carry")


def check_graph_args(graph, device_replay, sde_kernel, loss_kernel, adam_kernel, caps, caps_kernel, check_loss, check_caps):
    if not graph:
        return
    missing = [name for name, on in (("--device-replay", device_replay), ("--sde-kernel", sde_kernel),
                                     ("--loss-kernel", loss_kernel), ("--adam-kernel", adam_kernel),
                                     ("--caps-kernel", caps_kernel or not caps)) if not on]
    if missing:
        raise ValueError("--graph records the gradient step of the HIP kernels: it also needs " + " ".join(missing) +
                         " (a step with torch's own noise, losses or optimizers is not recorded)")
    if check_loss or check_caps:
        raise ValueError("--graph does not go with --check-loss or --check-caps: the test modes run outside a graph")


def train(env_id="usv-simple", envs=4096, steps=400, seed=0, log=print, device_replay=True, check_replay=False,
          max_episode_steps=None, sde_kernel=False, loss_kernel=False, check_loss=False, caps=False, caps_kernel=False,
          check_caps=False, adam_kernel=False, graph=False, keep=None, **cfg):
    """``steps`` vector steps of ``envs`` envs.  Returns one record per training round (``train_freq``
    steps, then ``gradient_steps`` gradient steps once ``learning_starts`` steps are in the buffer)."""
    import gym_usv_amd
    if check_loss and not loss_kernel:
        raise ValueError("check_loss compares the loss kernels with torch: it needs loss_kernel=True")
    check_caps_args(caps, caps_kernel, check_caps, dict(CONFIG_SAC, **cfg)["n_steps"])
    check_graph_args(graph, device_replay, sde_kernel, loss_kernel, adam_kernel, caps, caps_kernel, check_loss, check_caps)
    kw = {} if max_episode_steps is None else {"max_episode_steps": max_episode_steps}
    env = gym_usv_amd.make_vec(env_id, envs, seed=seed, copy=False, **kw)
    sac = SAC(env, seed=seed, device_replay=device_replay, check_replay=check_replay, sde_kernel=sde_kernel,
              loss_kernel=loss_kernel, check_loss=check_loss, caps=caps, caps_kernel=caps_kernel, check_caps=check_caps,
              adam_kernel=adam_kernel, graph=graph, **cfg)
    if keep is not None:                                    # the caller's list: the trainer, for what it wants to read
        keep.append(sac)
    c, hist, done_steps = sac.cfg, [], 0
    t0 = time.perf_counter()
    while done_steps < steps:
        block = min(c["train_freq"], steps - done_steps)
        sac.collect(block, random_actions=done_steps < c["learning_starts"])
        done_steps += block
        if done_steps <= c["learning_starts"]:
            continue
        rec = {"step": done_steps, **sac.train(c["gradient_steps"]), "gradient_steps": c["gradient_steps"],
               **sac.episode_stats(), "env_steps": sac.env_steps, "minibatches_checked": sac.checked}
        torch.cuda.synchronize()
        rec["wall_s"] = round(time.perf_counter() - t0, 3)
        hist.append(rec)
        log(json.dumps(rec))
    env.close()
    return hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env-id", default="usv-simple")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--buffer-size", type=int, default=CONFIG_SAC["buffer_size"])
    ap.add_argument("--batch-size", type=int, default=CONFIG_SAC["batch_size"])
    ap.add_argument("--device-replay", action="store_true", help="DeviceReplay instead of the torch full-storage buffer")
    ap.add_argument("--check-replay", action="store_true", help="keep both buffers and compare every minibatch bitwise")
    ap.add_argument("--sde-kernel", action="store_true", help="gSDE (config_sac's use_sde) through DeviceSDE.squashed")
    ap.add_argument("--n-steps", type=int, default=CONFIG_SAC["n_steps"],
                    help="n-step returns (SB3 2.7's n_steps) through sample_nstep; 1: the one-step target")
    ap.add_argument("--loss-kernel", action="store_true",
                    help="critic, actor and entropy-coefficient losses and Polyak through DeviceSACLoss / DevicePolyak")
    ap.add_argument("--check-loss", action="store_true", help="with --loss-kernel: also run the torch lines and compare")
    ap.add_argument("--caps", action="store_true", help="the CAPS regulariser (config_sac's lambda_t, lambda_s, eps_s)")
    ap.add_argument("--caps-kernel", action="store_true", help="with --caps: through DeviceCAPS instead of torch lines")
    ap.add_argument("--check-caps", action="store_true", help="with --caps-kernel: also run the torch lines and compare")
    ap.add_argument("--adam-kernel", action="store_true", help="the three Adam optimizers through DeviceAdam")
    ap.add_argument("--graph", action="store_true",
                    help="record a gradient step as a HIP graph and replay it (needs the four kernel flags above)")
    ap.add_argument("--lambda-t", type=float, default=CONFIG_SAC["lambda_t"])
    ap.add_argument("--lambda-s", type=float, default=CONFIG_SAC["lambda_s"])
    ap.add_argument("--eps-s", type=float, default=CONFIG_SAC["eps_s"])
    a = ap.parse_args()
    train(a.env_id, a.envs, a.steps, a.seed, device_replay=a.device_replay, check_replay=a.check_replay,
          sde_kernel=a.sde_kernel, loss_kernel=a.loss_kernel, check_loss=a.check_loss, caps=a.caps, caps_kernel=a.caps_kernel,
          check_caps=a.check_caps, adam_kernel=a.adam_kernel, graph=a.graph, buffer_size=a.buffer_size, batch_size=a.batch_size,
          n_steps=a.n_steps, lambda_t=a.lambda_t, lambda_s=a.lambda_s, eps_s=a.eps_s)


if __name__ == "__main__":
    main()
