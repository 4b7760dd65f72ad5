"""SB3's RolloutBuffer.add / compute_returns_and_advantage (common/buffers.py) and the truncation
bootstrap of OnPolicyAlgorithm.collect_rollouts (common/on_policy_algorithm.py) restated in NumPy float32
(SB3 is not installed), for tests/test_rollout_math.py and tests/test_gpu_rollout.py.  This file is the
definition the device rollout buffer (gym-usv_amd/csrc/usv_rollout.hpp) is compared with, bit for bit.

Every buffer is a float32 array and every scalar a np.float32, so NumPy rounds each operation to float32
on its own, as SB3's float32 buffers do.  Two deviations from SB3, both the device buffer's:
  * `rew` keeps the raw reward; the bootstrapped value gamma * V(terminal_obs) is added inside `gae`
    only (SB3 adds it into buffer.rewards, which PPO never reads again), so `gae` is idempotent;
  * the terminal observations are kept in `term_obs` and valued by the caller in one batch after the
    rollout (`term_val`), where SB3 calls the value net inside the step loop.  At most `term_cap` rows
    are kept, in (t, env) order; a later pair gets no bootstrap and is counted as overflow.
"""
import numpy as np


class NpRollout:
    def __init__(self, n, n_steps, obs_width, act_dim, term_cap=None):
        self.n, self.T, self.W, self.A = n, n_steps, obs_width, act_dim
        self.cap = 2 * n if term_cap is None else term_cap
        T = n_steps
        self.obs = np.zeros((T, n, obs_width), np.float32)
        self.act = np.zeros((T, n, act_dim), np.float32)
        self.rew, self.val, self.logp = (np.zeros((T, n), np.float32) for _ in range(3))
        self.adv, self.ret = (np.zeros((T, n), np.float32) for _ in range(2))
        self.start = np.zeros((T + 1, n), np.uint8)
        self.start[0] = 1                                # _last_episode_starts = np.ones
        self.term_slot = np.full((T, n), -1, np.int32)
        self.term_obs = np.zeros((self.cap, obs_width), np.float32)
        self.stored = self.overflow = 0
        self._pairs = 0

    def put_obs(self, t, obs, act, val, logp):
        self.obs[t], self.act[t], self.val[t], self.logp[t] = obs, act, val, logp

    def put_step(self, t, rew, term, trunc, final_stack):
        if t == 0:
            self._pairs = 0
        self.rew[t] = np.asarray(rew).astype(np.float32)
        term, trunc = np.asarray(term, bool), np.asarray(trunc, bool)
        self.start[t + 1] = term | trunc
        self.term_slot[t] = -1
        for e in np.nonzero(trunc & ~term)[0]:           # TimeLimit.truncated, in env order
            if self._pairs < self.cap:
                self.term_slot[t, e] = self._pairs
                self.term_obs[self._pairs] = final_stack[e]
            self._pairs += 1
        self.stored = min(self._pairs, self.cap)
        self.overflow = self._pairs - self.stored

    def gae(self, last_val, term_val, gamma, gae_lambda, stats=None):
        """`stats` (a dict) counts the operations whose FMA-contracted result would differ from the
        two-rounding one computed here: a test that cannot see a contraction proves nothing."""
        g32, gl32, one = np.float32(gamma), np.float32(gamma * gae_lambda), np.float32(1.0)
        last_val = np.asarray(last_val, np.float32)
        gae = np.zeros(self.n, np.float32)
        for t in reversed(range(self.T)):
            r = self.rew[t].copy()
            m = self.term_slot[t] >= 0
            if m.any():
                tv = np.asarray(term_val, np.float32)[self.term_slot[t][m]]
                p = g32 * tv
                _count(stats, "bootstrap", r[m] + p, _fma(g32, tv, r[m]))
                r[m] = r[m] + p
            nnt = one - self.start[t + 1].astype(np.float32)
            nv = last_val if t == self.T - 1 else self.val[t + 1]
            delta = (r + ((g32 * nv) * nnt)) - self.val[t]
            d = gl32 * nnt
            new = delta + (d * gae)
            _count(stats, "gae", new, _fma(d, gae, delta))
            gae = new
            self.adv[t] = gae
            self.ret[t] = self.adv[t] + self.val[t]
        self.start[0] = self.start[self.T]
        return self.adv, self.ret


def _fma(a, b, c):
    """float32(a * b + c) rounded once (the product of two float32 is exact in float64; the float64 sum's
    own rounding is 2^-29 of a float32 ulp away from mattering)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _count(stats, key, two_roundings, fused):
    if stats is not None:
        stats[key] = stats.get(key, 0) + int((np.asarray(two_roundings).view(np.uint32) !=
                                              np.asarray(fused).view(np.uint32)).sum())


PATTERNS = ("none", "all_trunc", "both", "consecutive", "random")


def script(n, T, W, A, pattern="random", seed=0, f64=False):
    """Scripted [T][n] inputs: rewards around the collision term's -20 on a tenth of the pairs, values of
    the size a trained value net gives, and the done pattern:
      none         no env is ever done
      all_trunc    every env truncated in step min(1, T - 1) (n slots at once), none terminated
      both         every env terminated and truncated together in that step (no slot)
      consecutive  envs 0, 2, 4 .. truncated in two consecutive steps (one if T == 1)
      random       terminated and truncated each with probability 0.25, independently."""
    rng = np.random.default_rng(9000 + 131 * n + 7 * T + W + PATTERNS.index(pattern) * 17 + seed)
    rew = rng.standard_normal((T, n)) * 0.7
    hit = rng.random((T, n)) < 0.1
    rew = np.where(hit, rew - 20.0, rew)
    rew = rew.astype(np.float64 if f64 else np.float32)
    term, trunc = np.zeros((T, n), bool), np.zeros((T, n), bool)
    s = min(1, T - 1)
    if pattern == "all_trunc":
        trunc[s] = True
    elif pattern == "both":
        term[s] = trunc[s] = True
    elif pattern == "consecutive":
        trunc[s, ::2] = True
        trunc[min(s + 1, T - 1), ::2] = True
    elif pattern == "random":
        term, trunc = rng.random((T, n)) < 0.25, rng.random((T, n)) < 0.25
    return dict(obs=rng.standard_normal((T, n, W)).astype(np.float32),
                act=rng.standard_normal((T, n, A)).astype(np.float32),
                val=(rng.standard_normal((T, n)) * 15.0 - 30.0).astype(np.float32),
                logp=(rng.standard_normal((T, n)) - 2.0).astype(np.float32),
                rew=rew, term=term, trunc=trunc,
                final=rng.standard_normal((T, n, W)).astype(np.float32),
                last_val=(rng.standard_normal(n) * 15.0 - 30.0).astype(np.float32))


def value_of(rows):
    """The stand-in value function of the scripted tests: any deterministic float32 function of a row."""
    rows = np.asarray(rows, np.float32)
    return (rows.astype(np.float64).sum(axis=-1) * 3.0 - 25.0).astype(np.float32)


def run(sc, n, T, W, A, term_cap=None, gamma=0.99, gae_lambda=0.95, ro=None, term_val=None, stats=None):
    """One scripted rollout through NpRollout (a given `ro` continues with its start[0]).  `term_val`
    defaults to value_of(term_obs) with NaN at the slots no pair holds."""
    ro = ro or NpRollout(n, T, W, A, term_cap)
    for t in range(T):
        ro.put_obs(t, sc["obs"][t], sc["act"][t], sc["val"][t], sc["logp"][t])
        ro.put_step(t, sc["rew"][t], sc["term"][t], sc["trunc"][t], sc["final"][t])
    if term_val is None:
        term_val = value_of(ro.term_obs)
        term_val[ro.stored:] = np.nan
    ro.gae(sc["last_val"], term_val, gamma, gae_lambda, stats)
    return ro
