"""SB3 2.7's NStepReplayBuffer._get_samples (stable_baselines3/common/buffers.py) restated in NumPy on the
full-storage buffer of tests/replay_ref.py (SB3 is not installed), for tests/test_replay_nstep_math.py and
tests/test_gpu_replay_nstep.py: the definition `DeviceReplay.gather_nstep` is compared with, bit for bit.

Two restatements of the same lines:

  * `get_nstep`: the loop.  With R rows, `count` stored transitions and last = (count - 1) mod R, the run of
    (slot, e) walks s_j = (slot + j) mod R, j = 0 .. n_steps - 1, and ends at m, the first j with done[s_j],
    timeout[s_j] or s_j == last, else n_steps - 1.  observations / actions are those of (slot, e);
    next_observations and dones = done * (1 - timeout) those of (s_m, e); rewards = rew[s_0] if m == 0,
    else the float32 sum in the order j = 0 .. m of fl(rew[s_j] g[j]); discounts = g[m + 1].
  * `get_nstep_sb3`: the vectorised code, line by line:
        last_valid_index = self.pos - 1
        original_timeout_values = self.timeouts[last_valid_index].copy()
        self.timeouts[last_valid_index] = np.logical_or(original_timeout_values,
                                                        np.logical_not(self.dones[last_valid_index]))
        steps = np.arange(self.n_steps).reshape(1, -1)
        indices = (batch_inds[:, None] + steps) % self.buffer_size
        rewards_seq = self._normalize_reward(self.rewards[indices, env_indices[:, None]], env)
        dones_seq = self.dones[indices, env_indices[:, None]]
        truncated_seq = self.timeouts[indices, env_indices[:, None]]
        done_or_truncated = np.logical_or(dones_seq, truncated_seq)
        done_idx = done_or_truncated.argmax(axis=1)
        has_done_or_truncated = done_or_truncated.any(axis=1)
        done_idx = np.where(has_done_or_truncated, done_idx, self.n_steps - 1)
        mask = np.arange(self.n_steps).reshape(1, -1) <= done_idx[:, None]
        target_q_discounts = self.gamma ** mask.sum(axis=1, keepdims=True).astype(np.float32)
        discounts = self.gamma ** np.arange(self.n_steps, dtype=np.float32).reshape(1, -1)
        discounted_rewards = rewards_seq * discounts * mask
        n_step_returns = discounted_rewards.sum(axis=1, keepdims=True)
        last_indices = (batch_inds + done_idx) % self.buffer_size
        next_obs = self.next_observations[last_indices, env_indices]
        self.timeouts[last_valid_index] = original_timeout_values
        final_dones = self.dones[last_indices, env_indices][:, None] *
                      (1 - self.timeouts[last_indices, env_indices][:, None])      (the temporary flag in force)
    with `table`'s entries substituted for the two `self.gamma ** float32` powers.

The table is g[j] = float32(float(gamma) ** j), j = 0 .. n_steps: the power in double, rounded once.  What
remains different from SB3: it takes the powers in float32 (within 1 ulp of the table), and it adds the
masked terms as +0.0 where the loop leaves them out (only a return of -0.0 shows that).  NumPy's sum(axis=1)
is sequential up to seven terms and an 8-way unrolled pairwise sum from eight on: the loop's order is the
definition for every n_steps.
"""
import numpy as np

import replay_ref as P

bits = P.bits
STOPS = ("done", "timeout", "last", "open")   # what ended a run: `kinds` of get_nstep


def table(gamma, n_steps):
    return np.array([np.float32(float(gamma) ** j) for j in range(n_steps + 1)], np.float32)


def get_nstep(ref, idx, n_steps, gamma, count=None):
    """The loop, on an NpReplay.  Returns (observations, actions, next_observations, dones, rewards,
    discounts) in SB3's order, then m [B], s_m [B] and the kind of stop per sample (an index of STOPS: a
    timeout is stored with done set and counts as a timeout; a stop at the last row counts as "last" only when
    that row stores neither)."""
    idx = np.asarray(idx, np.int64)
    n, R = ref.n, ref.R
    assert ((idx >= 0) & (idx < ref.size * n)).all()
    last = (ref.pos - 1) % R if count is None else (count - 1) % R
    g = table(gamma, n_steps)
    slot, e = idx // n, idx % n
    is_open = np.ones(len(idx), bool)                     # the loop over j, every sample at once
    acc = np.zeros(len(idx), np.float32)
    m, sm, kinds = (np.zeros(len(idx), np.int64) for _ in range(3))
    kinds += 3
    for j in range(n_steps):
        s = (slot + j) % R
        rew, done, timeout = ref.rew[s, e], ref.done[s, e] != 0, ref.timeout[s, e] != 0
        assert rew.dtype == np.float32 and g.dtype == np.float32          # float32 products, float32 sums
        acc = np.where(is_open, rew if j == 0 else acc + rew * g[j], acc)
        m, sm = np.where(is_open, j, m), np.where(is_open, s, sm)
        stop = done | timeout | (s == last)
        kinds = np.where(is_open & stop, np.where(timeout, 1, np.where(done, 0, 2)), kinds)
        is_open = is_open & ~stop
    dones = (ref.done[sm, e] * (np.float32(1.0) - ref.timeout[sm, e])).reshape(-1, 1)
    return (ref.obs[slot, e], ref.act[slot, e], ref.next_obs[sm, e], dones, acc.reshape(-1, 1),
            g[m + 1].reshape(-1, 1)), m, sm, kinds


def get_nstep_sb3(ref, idx, n_steps, gamma):
    """The vectorised code with the table substituted.  Returns (returns, discounts, dones, done_idx,
    last_indices)."""
    idx = np.asarray(idx, np.int64)
    n, R = ref.n, ref.R
    batch_inds, env_indices = idx // n, idx % n
    g = table(gamma, n_steps)
    timeouts = ref.timeout.copy()
    last_valid_index = ref.pos - 1
    timeouts[last_valid_index] = np.logical_or(timeouts[last_valid_index], np.logical_not(ref.done[last_valid_index]))
    steps = np.arange(n_steps).reshape(1, -1)
    indices = (batch_inds[:, None] + steps) % R
    rewards_seq = ref.rew[indices, env_indices[:, None]]
    dones_seq = ref.done[indices, env_indices[:, None]]
    truncated_seq = timeouts[indices, env_indices[:, None]]
    done_or_truncated = np.logical_or(dones_seq, truncated_seq)
    done_idx = done_or_truncated.argmax(axis=1)
    done_idx = np.where(done_or_truncated.any(axis=1), done_idx, n_steps - 1)
    mask = np.arange(n_steps).reshape(1, -1) <= done_idx[:, None]
    target_q_discounts = g[mask.sum(axis=1, keepdims=True)]
    discounts = g[:n_steps].reshape(1, -1)
    n_step_returns = (rewards_seq * discounts * mask).sum(axis=1, keepdims=True)
    last_indices = (batch_inds + done_idx) % R
    final_dones = ref.done[last_indices, env_indices][:, None] * (1 - timeouts[last_indices, env_indices][:, None])
    return n_step_returns, target_q_discounts, final_dones.astype(np.float32), done_idx, last_indices
