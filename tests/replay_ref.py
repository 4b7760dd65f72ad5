"""SB3's ReplayBuffer (stable_baselines3/common/buffers.py, optimize_memory_usage=False,
handle_timeout_termination=True) and the terminal-observation substitution of
OffPolicyAlgorithm._store_transition (common/off_policy_algorithm.py) restated in NumPy (SB3 is not
installed), for tests/test_replay_math.py and tests/test_gpu_replay.py.  This file is the definition the
device replay buffer (gym-usv_amd/csrc/usv_replay.hpp, gym_usv_amd.replay.DeviceReplay) is compared with,
bit for bit: full storage, two stacked windows per transition.

The lines restated:

  ReplayBuffer.__init__      self.buffer_size = max(buffer_size // n_envs, 1)
                             observations / next_observations (buffer_size, n_envs, *obs_shape),
                             actions (buffer_size, n_envs, action_dim), rewards / dones / timeouts
                             (buffer_size, n_envs) float32
  ReplayBuffer.add           self.observations[self.pos] = np.array(obs)
                             self.next_observations[self.pos] = np.array(next_obs)
                             self.actions[self.pos] = np.array(action)
                             self.rewards[self.pos] = np.array(reward)
                             self.dones[self.pos] = np.array(done)
                             self.timeouts[self.pos] = np.array([info.get("TimeLimit.truncated", False) ...])
                             self.pos += 1
                             if self.pos == self.buffer_size: self.full = True; self.pos = 0
  BaseBuffer.sample          upper_bound = self.buffer_size if self.full else self.pos
                             batch_inds = np.random.randint(0, upper_bound, size=batch_size)
  ReplayBuffer._get_samples  env_indices = np.random.randint(0, high=self.n_envs, size=(len(batch_inds),))
                             next_obs = self.next_observations[batch_inds, env_indices, :]
                             (self.observations[batch_inds, env_indices, :], self.actions[batch_inds, env_indices, :],
                              next_obs,
                              (self.dones[batch_inds, env_indices] * (1 - self.timeouts[batch_inds, env_indices])).reshape(-1, 1),
                              self.rewards[batch_inds, env_indices].reshape(-1, 1))
  _store_transition          for i, done in enumerate(dones):
                                 if done and infos[i].get("terminal_observation") is not None:
                                     next_obs[i] = infos[i]["terminal_observation"]
  the adapter (sb3.py)       TimeLimit.truncated = truncated and not terminated; done = terminated | truncated

A flat index is i = slot * n + e: (batch_inds, env_indices) as one number.  `script` takes the consistent
windows and the done patterns of rollout_frames_ref.script and adds random terminal frames:
final_stack[t] = concat(window[t][:, D:], final[t]), what DeviceWrappers.step writes for a done env.
"""
import numpy as np

import rollout_frames_ref as F

PATTERNS = F.PATTERNS
bits = F.bits


class NpReplay:
    def __init__(self, n, buffer_size, obs_width, act_dim):
        self.n, self.W, self.A = n, obs_width, act_dim
        self.R = R = max(buffer_size // n, 1)
        self.obs = np.zeros((R, n, obs_width), np.float32)
        self.next_obs = np.zeros((R, n, obs_width), np.float32)
        self.act = np.zeros((R, n, act_dim), np.float32)
        self.rew = np.zeros((R, n), np.float32)
        self.done = np.zeros((R, n), np.float32)
        self.timeout = np.zeros((R, n), np.float32)
        self.pos, self.full = 0, False

    @property
    def size(self):
        return self.R if self.full else self.pos

    def add(self, obs, next_obs, act, rew, done, timeout):
        p = self.pos
        self.obs[p], self.next_obs[p], self.act[p] = obs, next_obs, act
        self.rew[p] = np.asarray(rew).astype(np.float32)
        self.done[p], self.timeout[p] = done, timeout
        self.pos += 1
        if self.pos == self.R:
            self.full, self.pos = True, 0

    def store(self, window, act, rew, term, trunc, next_window, final_stack):
        """One env step as the trainer sees it: _store_transition, then add."""
        term, trunc = np.asarray(term, bool), np.asarray(trunc, bool)
        done = term | trunc
        next_obs = np.where(done[:, None], final_stack, next_window)
        self.add(window, next_obs, act, rew, done, trunc & ~term)

    def get(self, idx):
        """_get_samples at flat indices slot * n + e, every one in [0, size * n)."""
        idx = np.asarray(idx, np.int64)
        assert ((idx >= 0) & (idx < self.size * self.n)).all()
        s, e = idx // self.n, idx % self.n
        one = np.float32(1.0)
        return (self.obs[s, e], self.act[s, e], self.next_obs[s, e],
                (self.done[s, e] * (one - self.timeout[s, e])).reshape(-1, 1), self.rew[s, e].reshape(-1, 1))


def script(n, T, k, D, A=2, pattern="random", keep_sign=False, seed=0, f64=False, live_prologue=True):
    """T scripted env steps: rollout_frames_ref.script's windows [T + 1, n, k D], actions, rewards and
    dones, plus `final` [T, n, D] random terminal frames and `final_stack` [T, n, k D]."""
    sc = F.script(n, T, k, D, A, pattern, keep_sign, seed, live_prologue)
    rng = np.random.default_rng(5100 + 131 * n + 7 * T + 1009 * k + D + seed)
    sc["final"] = F.frames(rng, (T, n, D))
    sc["final_stack"] = np.concatenate((sc["windows"][:T][:, :, D:], sc["final"]), axis=2)
    if f64:                                             # rewards that float32 cannot hold exactly
        sc["rew"] = sc["rew"].astype(np.float64) + rng.standard_normal((T, n)) * 1e-9
    return sc


def run(sc, n, R, k, D, A, counts):
    """The scripted steps through NpReplay; {count: NpReplay state copy} after each of `counts` stores."""
    import copy
    ref, out = NpReplay(n, R * n, k * D, A), {}
    for t in range(max(counts)):
        ref.store(sc["windows"][t], sc["act"][t], sc["rew"][t], sc["term"][t], sc["trunc"][t], sc["windows"][t + 1],
                  sc["final_stack"][t])
        if t + 1 in counts:
            out[t + 1] = copy.deepcopy(ref)
    return out


def counts_of(R):
    """The fill states every test checks: one store, just full, one past full, mid-way through the third lap."""
    return sorted({1, R, R + 1, 2 * R + (R + 1) // 2})
