"""SB3's RunningMeanStd (common/running_mean_std.py), VecNormalize (common/vec_env/vec_normalize.py) and
StackedObservations restated in NumPy float64 (SB3 is not installed), for tests/test_norm_math.py and
tests/test_gpu_normalize.py.  Batch mean and variance are np.mean / np.var of the float64 cast.

Also the sizes at which the fused VecNormalize's reduction changes path, read from the constants of
gym-usv_amd/csrc/usv_norm_math.hpp, and the error bounds of its statistics.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "gym-usv_amd", "csrc", "usv_norm_math.hpp")
U = 2.0 ** -53


def header_constants():
    """kNormGroupRows and kNormBlockRows (envs of a wave group, of the smallest block chunk)."""
    src = open(HEADER).read()
    group = int(re.search(r"constexpr int kNormGroupRows = (\d+);", src).group(1))
    waves = int(re.search(r"constexpr int kNormWaves = (\d+);", src).group(1))
    assert "kNormBlockRows = kNormGroupRows * kNormWaves" in src
    return group, group * waves


def edge_sizes():
    """One fewer than, equal to and one more than a wave group and a block chunk, and an N that gives
    three partials with a ragged last one (a full group and a short one)."""
    try:
        g, b = header_constants()
    except OSError:                                      # no header: the tests that use these sizes fail on their own
        g, b = 16, 64
    return [g - 1, g, g + 1, b - 1, b, b + 1], 2 * b + g + 5


class RunningMeanStd:
    def __init__(self, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = 1e-4

    def update(self, arr):
        arr = np.asarray(arr, np.float64)
        self.update_from_moments(np.mean(arr, axis=0), np.var(arr, axis=0), arr.shape[0])

    def update_from_moments(self, bm, bv, n):
        delta = bm - self.mean
        tot = self.count + n
        new_mean = self.mean + delta * n / tot
        m2 = self.var * self.count + bv * n + np.square(delta) * self.count * n / tot
        self.mean, self.var, self.count = new_mean, m2 / tot, tot


class NpVecNormalize:
    """The statistics side of VecNormalize.step_wait / reset for [N, D] obs; the transform is `apply`
    below, given statistics."""

    def __init__(self, n, d, training=True, norm_obs=True, norm_reward=True, gamma=0.99, epsilon=1e-8):
        self.obs_rms, self.ret_rms = RunningMeanStd((d,)), RunningMeanStd(())
        self.returns = np.zeros(n, np.float64)
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        self.gamma, self.epsilon = gamma, epsilon

    def reset(self, obs):
        self.returns[:] = 0
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)

    def step(self, obs, rew, done):
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        if self.training and self.norm_reward:
            self.returns = self.returns * self.gamma + np.asarray(rew, np.float64)
            self.ret_rms.update(self.returns)
        after = self.returns.copy()                      # what ret_rms saw
        self.returns[np.asarray(done, bool)] = 0
        return after


def apply(x, mean, inv_std, clip):
    """The fused wrappers' transform, a bit-exact function of the published statistics."""
    return ((np.asarray(x).astype(np.float64) - mean) * inv_std).clip(-clip, clip).astype(np.float32)


class NpFrameStack:
    """StackedObservations (channels-last, 1-D obs)."""

    def __init__(self, n, d, k):
        self.s = np.zeros((n, k * d), np.float32)
        self.d = d

    def reset(self, obs):
        self.s[...] = 0
        self.s[:, -self.d:] = obs
        return self.s.copy()

    def update(self, obs, dones, final=None):
        """Returns (stack, terminal stacks [N, k d] whose rows of done envs are valid)."""
        self.s = np.roll(self.s, -self.d, axis=-1)
        term = self.s.copy()
        if final is not None:
            term[:, -self.d:] = final
        self.s[np.asarray(dones, bool)] = 0
        self.s[:, -self.d:] = obs
        return self.s.copy(), term


def mean_bound(n, t, xmax):
    """f64 mean of n terms combined in another order than NumPy's: 2 n u max|x|, t updates."""
    return t * 2 * n * U * xmax


def var_bound(n, t, xmax):
    return t * 8 * n * U * xmax * xmax
