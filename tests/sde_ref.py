"""The fused gSDE head restated in NumPy from its definition (not from the C++ header):

Philox4x32-10 in Python integers, key (seed lo, seed hi), counter (gid lo, gid hi, epoch, block); element
(j, k) of env e's [L][A] matrix is normal (j * A + k) % 4 of block (j * A + k) // 4; a block's words
(o0, o1, o2, o3) give z0 = r cos(2 pi u2), z1 = r sin(2 pi u2) with u1 = ((o0 >> 8) + 1) 2^-24,
u2 = (o1 >> 8) 2^-24, r = sqrt(-2 ln u1), and (o2, o3) give z2, z3.  The uniforms are exact float32
values; Box-Muller and every sum are float64."""
import functools
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
SDE_EPS = 1e-6


def philox(counter, key):
    """Philox4x32-10: counter (4 words), key (2 words) -> 4 words."""
    x0, x1, x2, x3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * x0, M1 * x2
        x0, x1, x2, x3 = (p1 >> 32) ^ x1 ^ k0, p1 & MASK, (p0 >> 32) ^ x3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return x0, x1, x2, x3


def block_words(seed, gid, epoch, b):
    gid &= (1 << 64) - 1
    return philox((gid & MASK, gid >> 32, epoch & MASK, b & MASK), (seed & MASK, (seed >> 32) & MASK))


def uniforms(words):
    """(u1, u2, u1', u2') of a block as float32 (exact: 24-bit integers times 2^-24)."""
    o0, o1, o2, o3 = words
    u = np.array([(o0 >> 8) + 1, o1 >> 8, (o2 >> 8) + 1, o3 >> 8], dtype=np.float64) * 2.0 ** -24
    u32 = u.astype(np.float32)
    assert (u32.astype(np.float64) == u).all()
    return u32


@functools.lru_cache(maxsize=None)
def _env_uniforms(seed, gid, epoch, blocks):
    return np.stack([uniforms(block_words(seed, gid, epoch, b)) for b in range(blocks)])


def uniform_table(seed, gid0, epoch, n, L, A):
    """[n, L * A // 4, 4] float32: (u1, u2, u1', u2') of every block of every env."""
    return np.stack([_env_uniforms(seed, (gid0 + e) & ((1 << 64) - 1), epoch, L * A // 4) for e in range(n)])


def normals(seed, gid0, epoch, n, L, A):
    """(z [n, L, A] float64, r [n, L, A] float64: the Box-Muller radius of each element's pair)."""
    u = uniform_table(seed, gid0, epoch, n, L, A).astype(np.float64)
    z = np.empty(u.shape, np.float64)
    rr = np.empty(u.shape, np.float64)
    for p in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[..., p]))
        t = 2.0 * math.pi * u[..., p + 1]
        z[..., p], z[..., p + 1] = r * np.cos(t), r * np.sin(t)
        rr[..., p] = rr[..., p + 1] = r
    return z.reshape(n, L, A), rr.reshape(n, L, A)


def clip(a, low, high):
    """max(min(a, high), low) in a's dtype."""
    return np.maximum(np.minimum(a, high), low)


def logp_of(a, mean, lat, std):
    """(logp [n], scale [n]) in float64 of actions `a` [n, A]; scale = 1 + sum_k (d^2 / s2 + |ln s2|)."""
    a, mean, lat, std = (np.asarray(x, np.float64) for x in (a, mean, lat, std))
    s2 = (lat * lat) @ (std * std) + SDE_EPS
    d = a - mean
    lp = (-d * d / (2.0 * s2) - 0.5 * np.log(s2) - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    return lp, 1.0 + (d * d / s2 + np.abs(np.log(s2))).sum(-1)


def sample(seed, gid0, epoch, mean, lat, std):
    """(a [n, A], a_scale [n, A], w [n, L, A]) in float64; a_scale = |mean| + sum_j |lat_j| std_jk |z_jk|.
    w_jk is the float32 product std_jk * z_jk of the definition taken in float64 (unrounded)."""
    mean, lat, std = (np.asarray(x, np.float64) for x in (mean, lat, std))
    n, L = lat.shape
    A = std.shape[1]
    z, _ = normals(seed, gid0, epoch, n, L, A)
    w = std[None] * z
    a = mean + np.einsum("ej,ejk->ek", lat, w)
    scale = np.abs(mean) + np.einsum("ej,ejk->ek", np.abs(lat), np.abs(w))
    return a, scale, w


def stats(z):
    """(mean z-score, variance z-score (s^2 - 1) sqrt(n / 2)) of a sample of would-be N(0, 1) values."""
    z = np.asarray(z, np.float64).ravel()
    n = z.size
    return float(z.mean() * math.sqrt(n)), float((z.var(ddof=1) - 1.0) * math.sqrt(n / 2.0))


def corr(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.corrcoef(x, y)[0, 1])
