"""Torch-native PPO with gSDE on the HIP vector env: config C5 without stable-baselines3.

The reference trains SB3 PPO on ``VecFrameStack(make_vec_env("usv-simple", n_envs), 5)`` with
``config_ppo`` (train_test/sb3_train_vec.py:67-81, train_test/config.py:3-15).  SB3 is absent from
this image, so this is a compact PPO with the same hyper-parameters where they carry over:

* policy / value: separate MLPs, ``net_arch=dict(pi=[256, 256], vf=[256, 256])``, ReLU,
  ``ortho_init=False`` (torch default init);
* gSDE (``use_sde=True``, ``sde_sample_freq=4``, ``log_std_init=-2``), as SB3's
  ``StateDependentNoiseDistribution`` (full_std, no expln, latent not learned through the noise):
  a per-env exploration matrix W ~ N(0, exp(log_std)^2) of shape [256, act_dim] is drawn at the
  start of every rollout and every 4 steps; the action is mean(s) + latent(s) @ W, where latent(s)
  is the policy's last hidden layer (detached); its log-probability is under
  N(mean(s), sqrt(latent(s)^2 @ exp(log_std)^2 + 1e-6)).  SB3 reports no entropy for gSDE and uses
  -mean(log_prob) in its place; with ent_coef 0 it does not enter the loss;
* SB3 PPO defaults for the rest: lr 3e-4, gamma 0.99, GAE lambda 0.95, clip 0.2, 10 epochs,
  vf_coef 0.5, ent_coef 0, max_grad_norm 0.5, per-minibatch advantage normalisation, Box-action
  clipping;
* TimeLimit truncation bootstrapped from the terminal observation's value for envs that were
  truncated and not terminated (SB3: ``infos[i]["terminal_observation"]`` and
  ``TimeLimit.truncated``); VecFrameStack(5) via ``DeviceFrameStack``;
* ``--fused`` (``train(fused=True)``): the frame stack and the episode statistics are
  ``DeviceWrappers`` and the rollout buffer, the truncation bootstrap and the GAE are
  ``DeviceRollout`` (HIP kernels behind the step, gym_usv_amd/rollout.py).  The policy reads the ring's
  window in place, the terminal observations are valued in one batch after the rollout, and a rollout
  makes no host sync: no ``.any()``, ``.nonzero()`` or ``bool()`` on a device tensor.  The buffer
  arithmetic is then SB3's float32 RolloutBuffer bit for bit; the default path is unchanged.
* ``--frames`` (with ``--fused``; ``train(fused=True, frames=True)``): the rollout keeps one 143-float
  frame per step and env instead of the 715-float stack (``DeviceRollout(n_stack=5)``) and the update
  reads each minibatch through ``DeviceRollout.gather``, one launch that rebuilds the stacked rows and
  fetches the five other fields.  The minibatches hold the same bits as without the flag.
* ``--sde-kernel`` (with ``--fused`` and gSDE; ``train(fused=True, sde_kernel=True)``): the rollout's gSDE
  head is ``gym_usv_amd.DeviceSDE``, one HIP launch per step that rebuilds each env's exploration matrix
  from a counter-based generator instead of storing it: no ``sample_weights`` tensor, no ``bmm``, no
  ``Normal.log_prob``.  ``reset_noise`` is then a host integer.  The update is unchanged: it only ever
  needed the variance.  The noise differs from torch's generator, so runs with and without the flag are
  two samples of the same algorithm, not the same numbers.
* ``--eval-kernel`` (with ``--sde-kernel``; ``train(..., eval_kernel=True)``): the update's head is
  ``DeviceSDE.evaluate``: the log-probability of the stored actions, the ratio and the clipped surrogate in one
  HIP launch and their gradients in two, in place of the torch ops of ``ActorCritic.dist``, ``log_prob``, ``exp``,
  ``clamp`` and ``min`` and their autograd.  Advantage normalisation, the value loss and ``-logp.mean()`` stay
  torch (``--loss-kernel`` below fuses them).  ``--check-eval`` (a test mode) evaluates both heads on every minibatch and records
  ``eval_logp_diff_max``, the largest ``|logp_kernel - logp_torch| / (1 + sum_k (d^2 / s2 + |ln s2|))`` of the
  update, read back once per update.
* ``--adam-kernel`` (``train(..., adam_kernel=True)``): ``clip_grad_norm_``, ``Adam.step()`` and ``zero_grad`` of every
  minibatch are ``gym_usv_amd.DeviceAdam``: two HIP launches over the whole parameter list (the norm in a fixed
  summation order, then clip and Adam in one pass) in place of torch's ops per tensor, with torch's arithmetic up to
  rounding.  Nothing else changes.
* ``--loss-kernel`` (``train(..., loss_kernel=True)``, in every mode): the minibatch loss is
  ``gym_usv_amd.DevicePPOLoss.loss``: advantage normalisation, the ratio, clamp and min, the value loss, the entropy
  term and the weighted sum in one C call (three launches with normalisation) and their gradients in one launch, in
  place of some twenty torch ops each way.  With ``--eval-kernel`` the head is then called without the PPO
  arguments and only gives the log-probability; with ``--no-sde`` the distribution's entropy goes in as a tensor.
  The update's record gains ``approx_kl`` and ``clip_fraction`` (means over the update) and ``explained_variance``
  (one call per update on the rollout's values and returns), read back with the other statistics once per update.
  ``--check-loss`` (a test mode) also evaluates the torch lines on every minibatch and records ``loss_diff``, the
  largest difference of each of the three losses over the sum of the magnitudes of its terms.
* ``--perm-kernel`` (with ``--fused``, with or without ``--frames``; ``train(fused=True, perm_kernel=True)``): the
  update draws its minibatches from ``DeviceRollout.sampler``: one C call per minibatch in place of ``randperm`` and
  ``gather`` (or fancy indexing), no index tensor.  The order is a keyed bijection of the rollout's samples that the
  gather kernel computes itself, with a device cursor that the call advances; every epoch still visits every sample
  once.  ``batch_size`` must divide ``envs * n_steps``.  The order differs from ``randperm``'s, so runs with and
  without the flag are two samples of the same algorithm.
* ``--graph`` (``train(..., graph=True)``; needs ``--fused --sde-kernel --eval-kernel --adam-kernel --loss-kernel
  --perm-kernel``, refuses ``--check-eval`` and ``--check-loss``): one minibatch step -- ``sampler.next`` into static
  tensors, the forward, ``DevicePPOLoss.loss``, ``zero_grad``, the backward, ``DeviceAdam(capturable=True).step()``
  and the statistics' running sum -- is recorded once as a HIP graph (``gym_usv_amd.capture_step``) and an update is
  ``n_epochs * envs * n_steps / batch_size`` replays with nothing launched in between.  The warm-up and capture
  calls train on the first minibatches: parameters, optimizer state and the sampler's cursor are put back behind
  them, so the run takes exactly the gradient steps of the run without ``--graph``.  ``clip``, ``vf_coef``,
  ``ent_coef`` and ``clip_range_vf`` are kernel arguments and frozen in the graph.
* ``--clip-range-vf X`` (SB3's ``clip_range_vf``, default none) and ``--no-normalize-advantage`` (SB3's
  ``normalize_advantage=False``) apply with and without ``--loss-kernel``.

Rollout size at 4096 envs.  config_ppo's ``n_steps=2048, batch_size=64`` are for the reference's 4
envs: 8 192 samples per update in 128 minibatches.  With 4096 envs the same n_steps would put 8.4 M
samples (24 GB of stacked obs) into every update, so this scales the other way, as massively
parallel PPO does: ``n_steps=32`` (131 072 samples per update, 16x config_ppo's) in minibatches of
4096 (64x config_ppo's, 32 per epoch): updates stay frequent in env-steps and each gradient step
averages over many envs.  Both stay configurable (``--n-steps``, ``--batch-size``).

Parity with SB3 itself is unpinned (SB3 is not installed).  Everything stays on the device:
observations, actions, rewards and dones are the env's HBM tensors; the host reads back only the
per-update statistics.

    python examples/ppo_torch.py --envs 4096 --updates 80 --log profiles/r03_ppo_4096.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gym-usv_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

CONFIG_PPO = {"n_stack": 5, "hidden": (256, 256), "log_std_init": -2.0, "use_sde": True, "sde_sample_freq": 4,
              "lr": 3e-4, "gamma": 0.99, "gae_lambda": 0.95, "clip": 0.2, "n_epochs": 10, "vf_coef": 0.5,
              "ent_coef": 0.0, "max_grad_norm": 0.5, "clip_range_vf": None, "normalize_advantage": True}
SDE_EPS = 1e-6        # StateDependentNoiseDistribution.epsilon


def mlp(inp, hidden, out=None):
    layers, d = [], inp
    for h in hidden:
        layers += [nn.Linear(d, h), nn.ReLU()]
        d = h
    if out is not None:
        layers.append(nn.Linear(d, out))
    return nn.Sequential(*layers)


class ActorCritic(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden, log_std_init, use_sde=True):
        super().__init__()
        self.use_sde = use_sde
        self.pi_body = mlp(obs_dim, hidden)                 # latent_pi (gSDE's latent_sde, detached)
        self.mu = nn.Linear(hidden[-1], act_dim)
        self.vf = mlp(obs_dim, hidden, 1)
        shape = (hidden[-1], act_dim) if use_sde else (act_dim,)
        self.log_std = nn.Parameter(torch.full(shape, float(log_std_init)))

    def dist(self, obs, validate=None):
        """(Normal over actions, latent_sde).  ``validate=False`` skips torch.distributions' argument
        checks, each of which asks the host ``bool(valid.all())``: a stream drain."""
        lat = self.pi_body(obs)
        mean = self.mu(lat)
        if not self.use_sde:
            return torch.distributions.Normal(mean, self.log_std.exp().expand_as(mean), validate_args=validate), None
        lat_sde = lat.detach()
        var = (lat_sde * lat_sde) @ (self.log_std.exp() ** 2)
        return torch.distributions.Normal(mean, torch.sqrt(var + SDE_EPS), validate_args=validate), lat_sde

    def sample_weights(self, n):
        """gSDE exploration matrices, one per env: [n, latent, act] ~ N(0, exp(log_std)^2)."""
        std = self.log_std.exp().detach()
        return torch.randn((n,) + tuple(std.shape), device=std.device) * std

    def value(self, obs):
        return self.vf(obs).squeeze(-1)


class PPO:
    """Rollout + update over a ``UsvVectorEnv`` (any registered id with a Box action space)."""

    def __init__(self, env, n_steps=32, batch_size=4096, seed=0, fused=False, frames=False, sde_kernel=False,
                 eval_kernel=False, check_eval=False, adam_kernel=False, loss_kernel=False, check_loss=False,
                 perm_kernel=False, graph=False, **cfg):
        from gym_usv_amd.sb3 import DeviceFrameStack
        self.cfg = dict(CONFIG_PPO, **cfg)
        self.env, self.n_steps, self.batch_size = env, n_steps, batch_size
        self.device = env.device
        self.N, D, A = env.num_envs, env.obs_dim, env.act_dim
        self.D = D
        self.fused = fused
        if frames and not fused:
            raise ValueError("frames=True needs fused=True")
        self.frames = frames
        check_graph_args(graph, fused, sde_kernel, eval_kernel, adam_kernel, loss_kernel, perm_kernel, check_eval, check_loss)
        if perm_kernel and not fused:
            raise ValueError("perm_kernel=True needs fused=True: the sampler reads a DeviceRollout")
        self.perm_kernel, self.graph, self.captured, self.sampler = perm_kernel, graph, None, None
        if sde_kernel and not (fused and self.cfg["use_sde"]):
            raise ValueError("sde_kernel=True needs fused=True and use_sde=True")
        if (eval_kernel or check_eval) and not (fused and sde_kernel):
            raise ValueError("eval_kernel=True and check_eval=True need fused=True and sde_kernel=True")
        self.eval_kernel, self.check_eval = eval_kernel, check_eval
        self._eval_diff = None                          # check_eval: the update's largest normalised |dlogp|
        if check_loss and not loss_kernel:
            raise ValueError("check_loss compares the loss kernel with torch: it needs loss_kernel=True")
        self.loss_kernel, self.check_loss, self.losses_checked = loss_kernel, check_loss, 0
        self.ppo_loss = self._ev = None
        if loss_kernel:
            from gym_usv_amd import DevicePPOLoss
            self.ppo_loss = DevicePPOLoss(self.device)
            self.loss_diff = torch.zeros(3, device=self.device)     # policy, value, entropy: the largest so far
        self.head = None
        if not fused:
            self.stack = DeviceFrameStack(self.N, D, self.cfg["n_stack"], self.device)
        torch.manual_seed(seed)
        self.model = ActorCritic(D * self.cfg["n_stack"], A, self.cfg["hidden"], self.cfg["log_std_init"],
                                 self.cfg["use_sde"]).to(self.device)
        self.adam_kernel = adam_kernel
        if adam_kernel:
            from gym_usv_amd import DeviceAdam
            self.opt = DeviceAdam(self.model.parameters(), lr=self.cfg["lr"], max_grad_norm=self.cfg["max_grad_norm"],
                                  capturable=graph)          # the step number in device memory: a replayed step counts
        else:
            self.opt = torch.optim.Adam(self.model.parameters(), lr=self.cfg["lr"])
        lo, hi = env.single_action_space.low, env.single_action_space.high
        self.a_lo = torch.as_tensor(lo, device=self.device, dtype=torch.float32)
        self.a_hi = torch.as_tensor(hi, device=self.device, dtype=torch.float32)
        obs, _ = env.reset(seed=seed)
        self.abs_ye = []                                # mean |ye| (m) of every step's obs
        self.env_steps = 0
        self.W = None
        if fused:
            from gym_usv_amd.rollout import DeviceRollout
            from gym_usv_amd.wrappers import DeviceWrappers
            k = self.cfg["n_stack"]
            self.wr = DeviceWrappers(self.N, D, k, self.device, env.reward.dtype)
            self.ro = DeviceRollout(self.N, n_steps, k * D, A, self.device, env.reward.dtype,
                                    n_stack=k if frames else None)
            self.wr.reset(obs)
            if perm_kernel:                             # a key of its own, as the head's below
                self.sampler = self.ro.sampler(batch_size, seed ^ 0x9E3779B97F4A7C15)
            if sde_kernel:
                from gym_usv_amd import DeviceSDE
                # a key of its own: the env's resets draw from the same generator keyed by `seed`
                self.head = DeviceSDE(self.N, self.cfg["hidden"][-1], A, self.device, seed ^ 0x5DE5DE5DE5DE5DE5, lo, hi,
                                      env_id_offset=int(env.cfg.env_id_offset))
            # the update reads the rollout's own buffers
            self.b_obs, self.b_act, self.b_logp, self.b_val = self.ro.obs, self.ro.act, self.ro.logp, self.ro.val
            self._totals = (0.0, 0, 0)
            return
        self.obs = self.stack.reset(obs).clone()
        T, N = n_steps, self.N
        z = lambda *s: torch.zeros(s, device=self.device)   # noqa: E731
        self.b_obs = z(T, N, D * self.cfg["n_stack"])
        self.b_act, self.b_logp, self.b_val = z(T, N, A), z(T, N), z(T, N)
        self.b_rew, self.b_done = z(T, N), z(T, N)
        self.ep_ret, self.ep_len = z(N), z(N)
        self.finished = []                              # (return, length) of completed episodes

    @torch.no_grad()
    def rollout_fused(self):
        """The rollout on DeviceWrappers + DeviceRollout: nothing here waits for the device."""
        sde, freq = self.cfg["use_sde"], self.cfg["sde_sample_freq"]
        wr, ro = self.wr, self.ro
        for t in range(self.n_steps):
            new_noise = sde and (t == 0 or (freq > 0 and t % freq == 0))   # reset_noise (SB3 collect_rollouts)
            obs = wr.stacked                                        # the ring's window, no clone
            if self.head is not None:
                if new_noise:
                    self.head.reset_noise()
                lat = self.model.pi_body(obs)
                a, a_env, logp = self.head.sample(self.model.mu(lat), lat, self.model.log_std.exp())
                ro.put_obs(t, obs, a, self.model.value(obs), logp)
                self._step_fused(t, a_env)
                continue
            if new_noise:
                self.W = self.model.sample_weights(self.N)
            dist, lat = self.model.dist(obs, validate=False)
            if sde:
                a = dist.mean + torch.bmm(lat.unsqueeze(1), self.W).squeeze(1)
            else:
                a = dist.sample()
            ro.put_obs(t, obs, a.contiguous(), self.model.value(obs), dist.log_prob(a).sum(-1))
            a_env = torch.max(torch.min(a, self.a_hi), self.a_lo)          # SB3 clips Box actions
            self._step_fused(t, a_env)

    def _step_fused(self, t, a_env):
        """The env step behind the fused wrappers and the rollout's row t of rewards and dones."""
        o, rew, term, trunc, info = self.env.step(a_env)
        self.abs_ye.append(o[:, 5].abs().mean() * 10.0)   # obs[5] = ye / 10 (simple_env.py:79-80)
        _, final_stack, _ = self.wr.step(o, rew, info["_final_obs"], info["final_obs"])
        self.ro.put_step(t, rew, term, trunc, final_stack)
        self.env_steps += self.N

    @torch.no_grad()
    def rollout(self):
        if self.fused:
            return self.rollout_fused()
        g, sde, freq = self.cfg["gamma"], self.cfg["use_sde"], self.cfg["sde_sample_freq"]
        for t in range(self.n_steps):
            if sde and (t == 0 or (freq > 0 and t % freq == 0)):   # reset_noise (SB3 collect_rollouts)
                self.W = self.model.sample_weights(self.N)
            dist, lat = self.model.dist(self.obs)
            if sde:
                a = dist.mean + torch.bmm(lat.unsqueeze(1), self.W).squeeze(1)
            else:
                a = dist.sample()
            self.b_obs[t] = self.obs
            self.b_act[t] = a
            self.b_logp[t] = dist.log_prob(a).sum(-1)
            self.b_val[t] = self.model.value(self.obs)
            a_env = torch.max(torch.min(a, self.a_hi), self.a_lo)          # SB3 clips Box actions
            obs, rew, term, trunc, info = self.env.step(a_env)
            done = info["_final_obs"]                                     # terminated | truncated
            self.abs_ye.append(obs[:, 5].abs().mean() * 10.0)   # obs[5] = ye / 10 (simple_env.py:79-80)
            nxt, term_rows = self.stack.step(obs, done, info["final_obs"])
            r = rew.float().clone()
            if bool(trunc.any()):
                # bootstrap envs truncated (TimeLimit / out of the field) and not terminated (SB3:
                # TimeLimit.truncated and not done-by-termination)
                idx = done.nonzero().flatten()
                tr = (trunc & ~term)[idx]
                if bool(tr.any()):
                    r[idx[tr]] += g * self.model.value(term_rows[tr])
            self.b_rew[t] = r
            self.b_done[t] = done.float()
            self.ep_ret += rew.float()
            self.ep_len += 1
            if bool(done.any()):
                d = done.nonzero().flatten()
                self.finished.append(torch.stack((self.ep_ret[d], self.ep_len[d]), 1))
                self.ep_ret[d] = 0
                self.ep_len[d] = 0
            self.obs = nxt.clone()
            self.env_steps += self.N

    def advantages(self):
        g, lam = self.cfg["gamma"], self.cfg["gae_lambda"]
        if self.fused:
            with torch.no_grad():                       # one forward pass over the terminal rows
                return self.ro.gae(self.model.value(self.wr.stacked), self.model.value(self.ro.term_obs), g, lam)
        with torch.no_grad():
            last_v = self.model.value(self.obs)
        adv = torch.zeros_like(self.b_rew)
        gae = torch.zeros(self.N, device=self.device)
        for t in reversed(range(self.n_steps)):
            nv = last_v if t == self.n_steps - 1 else self.b_val[t + 1]
            nonterm = 1.0 - self.b_done[t]
            delta = self.b_rew[t] + g * nv * nonterm - self.b_val[t]
            gae = delta + g * lam * nonterm * gae
            adv[t] = gae
        return adv, adv + self.b_val

    def policy_terms(self, obs, actions, old_logp, a_):
        """(log_prob [B], policy loss, the torch distribution or None) of one minibatch.  ``eval_kernel``: the
        three come from ``DeviceSDE.evaluate`` on the policy's mean and detached latent; ``check_eval``: both heads
        run and the largest normalised difference of their log-probabilities is kept on the device.  ``a_`` None
        (``loss_kernel``): the log-probability alone, no policy loss."""
        clip = self.cfg["clip"]
        if not (self.eval_kernel or self.check_eval):
            dist, _ = self.model.dist(obs)
            logp = dist.log_prob(actions).sum(-1)
            if a_ is None:
                return logp, None, dist
            ratio = (logp - old_logp).exp()
            return logp, -torch.min(ratio * a_, ratio.clamp(1 - clip, 1 + clip) * a_).mean(), dist
        lat = self.model.pi_body(obs)
        mean, std = self.model.mu(lat), self.model.log_std.exp()
        lat = lat.detach()
        if self.eval_kernel and a_ is None:
            logp, pg = self.head.evaluate(mean, lat, std, actions).log_prob, None
        elif self.eval_kernel:
            ev = self.head.evaluate(mean, lat, std, actions, old_logp, a_, clip)
            logp, pg = ev.log_prob, -ev.surrogate.mean()
        if self.check_eval or not self.eval_kernel:
            s2 = (lat * lat) @ (std ** 2) + SDE_EPS
            t_logp = torch.distributions.Normal(mean, torch.sqrt(s2), validate_args=False).log_prob(actions).sum(-1)
        if not self.eval_kernel and a_ is None:
            logp, pg = t_logp, None
        elif not self.eval_kernel:
            ratio = (t_logp - old_logp).exp()
            logp, pg = t_logp, -torch.min(ratio * a_, ratio.clamp(1 - clip, 1 + clip) * a_).mean()
        if self.check_eval:
            with torch.no_grad():
                k_logp = logp if self.eval_kernel else self.head.evaluate(mean, lat, std, actions).log_prob
                d = actions - mean
                scale = 1.0 + (d * d / s2 + s2.log().abs()).sum(-1)
                worst = ((k_logp - t_logp).abs() / scale).max()
                self._eval_diff = worst if self._eval_diff is None else torch.maximum(self._eval_diff, worst)
        return logp, pg, None

    def update_record(self, s):
        """The update's record from ``s``, the mean of its minibatches' statistics."""
        if self.loss_kernel:                            # one read for the update's means and explained_variance
            s = torch.cat((s, self._ev.reshape(1)))
        s = s.tolist()
        rec = {"policy_loss": s[0], "value_loss": s[1], "entropy": s[2],
               "std_mean": float(self.model.log_std.detach().exp().mean())}
        if self.loss_kernel:
            rec["approx_kl"], rec["clip_fraction"], rec["explained_variance"] = s[3], s[4], s[5]
        if self.check_loss:                             # the largest so far
            rec["loss_diff"] = dict(zip(("policy", "value", "entropy"), self.loss_diff.tolist()))
            rec["losses_checked"] = self.losses_checked
        if self.check_eval:
            rec["eval_logp_diff_max"], self._eval_diff = float(self._eval_diff), None
        return rec

    def gradient_step(self, loss):
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        if not self.adam_kernel:                        # DeviceAdam.step clips by its max_grad_norm itself
            nn.utils.clip_grad_norm_(self.model.parameters(), self.cfg["max_grad_norm"])
        self.opt.step()

    def minibatch_loss(self, obs, act, old_logp, adv, ret, old_val):
        """(loss, the minibatch's statistics) of SB3's ``PPO.train`` lines: (policy loss, value loss, entropy) and,
        with ``loss_kernel``, approx_kl and clip_fraction behind them."""
        c = self.cfg
        if self.loss_kernel:
            return self.kernel_loss(obs, act, old_logp, adv, ret, old_val)
        a_ = adv
        if c["normalize_advantage"] and len(a_) > 1:
            a_ = (a_ - a_.mean()) / (a_.std() + 1e-8)
        logp, pg, dist = self.policy_terms(obs, act, old_logp, a_)
        if c["clip_range_vf"] is None:
            vl = ((self.model.value(obs) - ret) ** 2).mean()
        else:
            vp = old_val + (self.model.value(obs) - old_val).clamp(-c["clip_range_vf"], c["clip_range_vf"])
            vl = ((vp - ret) ** 2).mean()
        ent = -logp.mean() if c["use_sde"] else dist.entropy().sum(-1).mean()
        loss = pg + c["vf_coef"] * vl - c["ent_coef"] * ent
        return loss, torch.stack((pg.detach(), vl.detach(), ent.detach()))

    def kernel_loss(self, obs, act, old_logp, adv, ret, old_val):
        """``minibatch_loss`` through ``DevicePPOLoss.loss``: the head gives the log-probability alone."""
        c = self.cfg
        logp, _, dist = self.policy_terms(obs, act, old_logp, None)
        values = self.model.value(obs)
        entropy = None if c["use_sde"] else dist.entropy().sum(-1)
        cvf = c["clip_range_vf"]
        out = self.ppo_loss.loss(logp, old_logp, adv, values, ret, clip_range=c["clip"], vf_coef=c["vf_coef"],
                                 ent_coef=c["ent_coef"], normalize_advantage=c["normalize_advantage"],
                                 old_values=None if cvf is None else old_val, clip_range_vf=cvf, entropy=entropy)
        if self.check_loss:
            self.compare_loss(out, logp, values, entropy, old_logp, adv, ret, old_val)
        return out.loss, torch.stack((out.policy_loss, out.value_loss, -out.entropy_loss, out.approx_kl,
                                      out.clip_fraction))

    @torch.no_grad()
    def compare_loss(self, out, logp, values, entropy, old_logp, adv, ret, old_val):
        """``check_loss``: the torch lines on the same tensors; each loss's difference over the sum of the magnitudes
        of its terms (a normalised advantage's terms are |adv| and |mean| over the std)."""
        c = self.cfg
        clip, cvf = c["clip"], c["clip_range_vf"]
        a_, mag = adv, adv.abs()
        if c["normalize_advantage"] and len(a_) > 1:
            mean, std = a_.mean(), a_.std()
            a_, mag = (a_ - mean) / (std + 1e-8), (mag + mean.abs()) / (std + 1e-8)
        ratio = (logp - old_logp).exp()
        pg = -torch.min(ratio * a_, ratio.clamp(1 - clip, 1 + clip) * a_).mean()
        vp = values if cvf is None else old_val + (values - old_val).clamp(-cvf, cvf)
        vl = ((vp - ret) ** 2).mean()
        term = -logp if entropy is None else entropy
        ours = torch.stack((out.policy_loss, out.value_loss, -out.entropy_loss))
        diff = (ours - torch.stack((pg, vl, term.mean()))).abs()
        scale = torch.stack(((ratio * mag).mean(), ((vp.abs() + ret.abs()) ** 2).mean(), term.abs().mean()))
        r = torch.where(scale > 0, diff / scale, diff * float("inf")).nan_to_num(nan=0.0)   # a zero scale wants a zero diff
        self.loss_diff = torch.maximum(self.loss_diff, r)
        self.losses_checked += 1

    def update(self):
        c = self.cfg
        adv, ret = self.advantages()
        M = self.n_steps * self.N
        if self.loss_kernel:
            self._ev = self.ppo_loss.explained_variance(self.b_val, ret)
        if self.perm_kernel:
            return self.update_perm()
        if self.frames:
            return self.update_frames(M)
        obs = self.b_obs.reshape(M, -1)
        act = self.b_act.reshape(M, -1)
        logp0, val0, adv, ret = self.b_logp.reshape(M), self.b_val.reshape(M), adv.reshape(M), ret.reshape(M)
        stats = []
        for _ in range(c["n_epochs"]):
            perm = torch.randperm(M, device=self.device)
            for k in range(0, M, self.batch_size):
                i = perm[k:k + self.batch_size]
                loss, stat = self.minibatch_loss(obs[i], act[i], logp0[i], adv[i], ret[i], val0[i])
                self.gradient_step(loss)
                stats.append(stat)
        return self.update_record(torch.stack(stats).mean(0))

    def update_frames(self, M):
        """``update``'s loop with every minibatch read by ``DeviceRollout.gather`` (frame storage has no
        ``[T * N, W]`` view to index)."""
        c = self.cfg
        stats = []
        for _ in range(c["n_epochs"]):
            perm = torch.randperm(M, device=self.device)
            for k in range(0, M, self.batch_size):
                mb = self.ro.gather(perm[k:k + self.batch_size])
                loss, stat = self.minibatch_loss(mb.observations, mb.actions, mb.old_log_prob, mb.advantages, mb.returns,
                                                 mb.old_values)
                self.gradient_step(loss)
                stats.append(stat)
        return self.update_record(torch.stack(stats).mean(0))

    def update_perm(self):
        """``update``'s loop on ``DeviceRollout.sampler``: no permutation tensor, one C call per minibatch; with
        ``graph`` the whole minibatch step is a replay."""
        steps = self.cfg["n_epochs"] * self.sampler.batches_per_epoch
        if self.graph:
            if self.captured is None:
                self.capture()
            self.acc.zero_()
            for _ in range(steps):
                self.captured.replay()                  # nothing else is launched in between
            return self.update_record(self.acc / steps)
        stats = []
        for _ in range(steps):
            stats.append(self.sampled_step(None))
        return self.update_record(torch.stack(stats).mean(0))

    def sampled_step(self, out):
        """One minibatch step behind ``sampler.next`` (into ``out``, or fresh tensors); returns its statistics."""
        mb = self.sampler.next(out=out)
        loss, stat = self.minibatch_loss(mb.observations, mb.actions, mb.old_log_prob, mb.advantages, mb.returns,
                                         mb.old_values)
        self.gradient_step(loss)
        return stat

    def graph_step(self):
        self.acc += self.sampled_step(self.static_mb)
        return self.acc

    def capture(self):
        """Records ``graph_step``.  The warm-up and capture calls train on the update's first minibatches: what they
        changed (parameters, optimizer state, the sampler's cursor) is put back, so the first replay is the run's
        first gradient step."""
        from gym_usv_amd import RolloutSamples, capture_step
        B, W, A = self.batch_size, self.ro.w, self.ro.a
        z = lambda *shape: torch.zeros(shape, device=self.device)   # noqa: E731
        self.static_mb = RolloutSamples(z(B, W), z(B, A), z(B), z(B), z(B), z(B))
        self.acc = z(5)
        nets = list(self.model.parameters())
        kept = [p.detach().clone() for p in nets]
        opt_state, cursor = self.opt.state_dict(), self.sampler.state_dict()
        self.captured = capture_step(self.graph_step)
        with torch.no_grad():
            for p, k in zip(nets, kept):
                p.copy_(k)                              # in place: the graph holds the addresses
        self.opt.load_state_dict(opt_state)
        self.sampler.load_state_dict(cursor)

    def episode_stats(self):
        out = {"mean_abs_ye": float(torch.stack(self.abs_ye).mean())} if self.abs_ye else {}
        self.abs_ye = []
        if self.fused:                                  # DeviceWrappers' cumulative counters, once per update
            now, was = self.wr.totals(), self._totals
            self._totals = now
            eps = now[1] - was[1]
            if eps == 0:
                return {"episodes": 0, **out}
            return {"episodes": eps, "ep_rew_mean": (now[0] - was[0]) / eps, "ep_len_mean": (now[2] - was[2]) / eps,
                    **out}
        if not self.finished:
            return {"episodes": 0, **out}
        f = torch.cat(self.finished)
        self.finished = []
        return {"episodes": int(f.shape[0]), "ep_rew_mean": float(f[:, 0].mean()),
                "ep_len_mean": float(f[:, 1].mean()), **out}


def check_graph_args(graph, fused, sde_kernel, eval_kernel, adam_kernel, loss_kernel, perm_kernel, check_eval, check_loss):
    if not graph:
        return
    missing = [name for name, on in (("--fused", fused), ("--sde-kernel", sde_kernel), ("--eval-kernel", eval_kernel),
                                     ("--adam-kernel", adam_kernel), ("--loss-kernel", loss_kernel),
                                     ("--perm-kernel", perm_kernel)) if not on]
    if missing:
        raise ValueError("--graph records the minibatch step of the HIP kernels: it also needs " + " ".join(missing) +
                         " (a step with torch's own head, loss, optimizer or permutation is not recorded)")
    if check_eval or check_loss:
        raise ValueError("--graph does not go with --check-eval or --check-loss: the test modes run outside a graph")


def train(env_id="usv-simple", envs=4096, updates=10, n_steps=32, batch_size=4096, seed=0, log=print, fused=False,
          frames=False, sde_kernel=False, eval_kernel=False, check_eval=False, adam_kernel=False, loss_kernel=False,
          check_loss=False, perm_kernel=False, graph=False, keep=None, **cfg):
    """``keep``: a dict that receives the ``PPO`` object under "ppo" (tests read its parameters and counters)."""
    import gym_usv_amd
    if check_loss and not loss_kernel:
        raise ValueError("check_loss compares the loss kernel with torch: it needs loss_kernel=True")
    check_graph_args(graph, fused, sde_kernel, eval_kernel, adam_kernel, loss_kernel, perm_kernel, check_eval, check_loss)
    if perm_kernel and not fused:
        raise ValueError("perm_kernel=True needs fused=True: the sampler reads a DeviceRollout")
    if perm_kernel and (int(envs) * int(n_steps)) % int(batch_size) != 0:
        raise ValueError("perm_kernel=True needs a batch_size that divides envs * n_steps")
    env = gym_usv_amd.make_vec(env_id, envs, seed=seed, copy=False)   # each step is consumed at once
    ppo = PPO(env, n_steps=n_steps, batch_size=batch_size, seed=seed, fused=fused, frames=frames,
              sde_kernel=sde_kernel, eval_kernel=eval_kernel, check_eval=check_eval, adam_kernel=adam_kernel,
              loss_kernel=loss_kernel, check_loss=check_loss, perm_kernel=perm_kernel, graph=graph, **cfg)
    if keep is not None:
        keep["ppo"] = ppo
    hist = []
    t0 = time.perf_counter()
    for u in range(updates):
        ppo.rollout()
        rec = {"update": u + 1, **ppo.update(), **ppo.episode_stats(), "env_steps": ppo.env_steps}
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
    ap.add_argument("--updates", type=int, default=80)
    ap.add_argument("--n-steps", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-sde", action="store_true", help="state-independent log-std instead of gSDE")
    ap.add_argument("--fused", action="store_true", help="DeviceWrappers + DeviceRollout: a sync-free rollout")
    ap.add_argument("--frames", action="store_true",
                    help="with --fused: one frame per step in the rollout, minibatches by DeviceRollout.gather")
    ap.add_argument("--sde-kernel", action="store_true",
                    help="with --fused and gSDE: the rollout's action head is one DeviceSDE launch per step")
    ap.add_argument("--eval-kernel", action="store_true",
                    help="with --sde-kernel: the update's log_prob, ratio and clipped surrogate are DeviceSDE.evaluate")
    ap.add_argument("--check-eval", action="store_true",
                    help="with --sde-kernel: evaluate both heads on every minibatch and record eval_logp_diff_max")
    ap.add_argument("--adam-kernel", action="store_true",
                    help="clip_grad_norm_ and Adam.step() of every minibatch through DeviceAdam")
    ap.add_argument("--loss-kernel", action="store_true",
                    help="the minibatch loss, approx_kl and clip_fraction through DevicePPOLoss; explained_variance per update")
    ap.add_argument("--check-loss", action="store_true",
                    help="with --loss-kernel: also evaluate the torch lines on every minibatch and record loss_diff")
    ap.add_argument("--perm-kernel", action="store_true",
                    help="with --fused: minibatches from DeviceRollout.sampler (an in-kernel permutation, a device cursor)")
    ap.add_argument("--graph", action="store_true",
                    help="record a minibatch step as a HIP graph and replay it (needs --fused and the five kernel flags)")
    ap.add_argument("--clip-range-vf", type=float, default=None, help="SB3's clip_range_vf (default: none)")
    ap.add_argument("--no-normalize-advantage", action="store_true", help="SB3's normalize_advantage=False")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.frames and not a.fused:
        ap.error("--frames needs --fused")
    if a.sde_kernel and (not a.fused or a.no_sde):
        ap.error("--sde-kernel needs --fused and gSDE (no --no-sde)")
    if (a.eval_kernel or a.check_eval) and not a.sde_kernel:
        ap.error("--eval-kernel and --check-eval need --sde-kernel")
    if a.check_loss and not a.loss_kernel:
        ap.error("--check-loss needs --loss-kernel")
    if a.perm_kernel and not a.fused:
        ap.error("--perm-kernel needs --fused")
    if a.perm_kernel and (a.envs * a.n_steps) % a.batch_size != 0:
        ap.error("--perm-kernel needs a --batch-size that divides --envs * --n-steps")
    try:
        check_graph_args(a.graph, a.fused, a.sde_kernel, a.eval_kernel, a.adam_kernel, a.loss_kernel, a.perm_kernel,
                         a.check_eval, a.check_loss)
    except ValueError as e:
        ap.error(str(e))
    f = open(a.log, "a") if a.log else None

    def log(s):
        print(s, flush=True)
        if f:
            f.write(s + "\n")
            f.flush()
    if f:
        log(json.dumps({"config": {**CONFIG_PPO, "use_sde": not a.no_sde, "env_id": a.env_id, "envs": a.envs,
                                   "n_steps": a.n_steps, "batch_size": a.batch_size, "seed": a.seed,
                                   "fused": a.fused, "frames": a.frames, "sde_kernel": a.sde_kernel,
                                   "eval_kernel": a.eval_kernel, "check_eval": a.check_eval,
                                   "adam_kernel": a.adam_kernel, "loss_kernel": a.loss_kernel,
                                   "check_loss": a.check_loss, "perm_kernel": a.perm_kernel, "graph": a.graph,
                                   "clip_range_vf": a.clip_range_vf,
                                   "normalize_advantage": not a.no_normalize_advantage}}))
    train(a.env_id, a.envs, a.updates, a.n_steps, a.batch_size, a.seed, log=log, fused=a.fused, frames=a.frames,
          sde_kernel=a.sde_kernel, eval_kernel=a.eval_kernel, check_eval=a.check_eval, adam_kernel=a.adam_kernel,
          loss_kernel=a.loss_kernel, check_loss=a.check_loss, perm_kernel=a.perm_kernel, graph=a.graph,
          use_sde=not a.no_sde, clip_range_vf=a.clip_range_vf,
          normalize_advantage=not a.no_normalize_advantage)


if __name__ == "__main__":
    main()
