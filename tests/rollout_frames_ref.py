"""The definition the frame-deduplicated rollout storage and the minibatch gather
(gym-usv_amd/csrc/usv_rollout_frames.hpp, gym_usv_amd.rollout.DeviceRollout(n_stack=k).gather) are held
to, for tests/test_rollout_frames_math.py and tests/test_gpu_rollout_frames.py.

The definition is full storage: a rollout that keeps every stacked window, `obs[t, e, :]`, and reads row
`idx` of its `[T * n, W]` view.  Frame storage must give the same bits.  So this file has two parts:

  * `script`: consistent inputs -- frames `f[t, e, :]`, dones, and the windows that SB3's
    `VecFrameStack` (StackedObservations.update, channels-last) builds from them in either clear mode:
        window[t + 1] = concat(cleared(window[t][D:]) if done[t] else window[t][D:], f[t + 1])
    with cleared(x) = +0.0, or x * 0.0 (-0.0 where x was negative) with `keep_sign`, which is what
    `DeviceWrappers(clear_keeps_sign=True)` leaves in its ring;
  * `gather`: `full_obs.reshape(T * n, W)[idx]`.
"""
import numpy as np

import rollout_ref as R

# rollout_ref's done patterns and two more:
#   double  env e is done in the two consecutive steps s, s + 1 with s = e mod max(T - 1, 1): a window
#           then holds two boundaries, at every position the rollout has
#   last    every env is done in step T - 1 (start[T], which no sample of this rollout may consult, and
#           which the next rollout inherits as its start[0])
PATTERNS = R.PATTERNS + ("double", "last")


def cleared(x, keep_sign):
    x = np.asarray(x, np.float32)
    return x * np.float32(0.0) if keep_sign else np.zeros_like(x)


def frames(rng, shape):
    """Random frames: about half negative, about 2 % exact +0.0 and 2 % exact -0.0."""
    f = rng.standard_normal(shape).astype(np.float32)
    z = rng.random(shape)
    f[z < 0.02] = np.float32(0.0)
    f[(z >= 0.02) & (z < 0.04)] = np.float32(-0.0)
    return f


def script(n, T, k, D, A=2, pattern="random", keep_sign=False, seed=0, live_prologue=True):
    """rollout_ref.script's inputs for T steps with `obs` replaced by consistent windows [T + 1, n, k D]
    (window[T] is the one after the last step: the next rollout's first) and the frames `f` [T + 1, n, D].
    `live_prologue`: window[0] is mid-episode (k random frames, the older ones of every third env
    cleared as after a done two steps before); otherwise it is the window after a reset, +0.0 in the
    older slots."""
    W = k * D
    base = pattern if pattern in R.PATTERNS else "none"
    sc = R.script(n, T, W, A, base, seed=seed)
    rng = np.random.default_rng(77000 + 131 * n + 7 * T + 1009 * k + D + 17 * PATTERNS.index(pattern) + seed)
    e = np.arange(n)
    if pattern == "double":
        s = e % max(T - 1, 1)
        sc["term"][s, e] = True
        sc["term"][np.minimum(s + 1, T - 1), e] = True
    elif pattern == "last":
        sc["trunc"][T - 1] = True
    f = frames(rng, (T + 1, n, D))
    win = np.zeros((T + 1, n, W), np.float32)
    if live_prologue:
        win[0] = frames(rng, (n, W))
        if k > 2:
            win[0, ::3, :(k - 2) * D] = cleared(win[0, ::3, :(k - 2) * D], keep_sign)
    win[0, :, (k - 1) * D:] = f[0]
    done = sc["term"] | sc["trunc"]
    for t in range(T):
        older = win[t][:, D:]
        win[t + 1, :, :(k - 1) * D] = np.where(done[t][:, None], cleared(older, keep_sign), older)
        win[t + 1, :, (k - 1) * D:] = f[t + 1]
    sc["obs"] = win[:T]
    sc["windows"] = win
    sc["frames"] = f
    return sc


def split(sc, T):
    """A script of 2 T steps as two scripts of T steps, the second beginning with the first's last window."""
    out = []
    for lo in (0, T):
        part = {}
        for key, v in sc.items():
            if key == "last_val":
                part[key] = v
            elif key in ("windows", "frames"):
                part[key] = v[lo:lo + T + 1]
            else:
                part[key] = v[lo:lo + T]
        out.append(part)
    return out


def gather(full_obs, idx):
    """The reference gather: row idx = t * n + e of the [T, n, W] full-storage buffer."""
    full_obs = np.asarray(full_obs)
    T, n, W = full_obs.shape
    return full_obs.reshape(T * n, W)[np.asarray(idx)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])
