"""A NumPy restatement of gym-usv_amd/csrc/usv_rollout_perm_math.hpp, written from its comment: the keyed bijection
of [0, M) behind ``usv_rollout_gather_perm`` (a six-round alternating unbalanced Feistel network with cycle walking,
keyed by Philox4x32-10) and the two-word minibatch cursor.  Vectorised over positions; nothing here calls the library."""
import numpy as np

ROUNDS = 6
TAG = 0x5045524D          # "PERM"
M32 = 0xFFFFFFFF


def philox(counter, key):
    """Philox4x32-10 on Python ints: the four output words."""
    x0, x1, x2, x3 = counter
    a, b = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * x0, 0xCD9E8D57 * x2
        x0, x1, x2, x3 = (p1 >> 32) ^ x1 ^ a, p1 & M32, (p0 >> 32) ^ x3 ^ b, p0 & M32
        a, b = (a + 0x9E3779B9) & M32, (b + 0xBB67AE85) & M32
    return x0, x1, x2, x3


def keys(seed, epoch):
    seed, epoch = int(seed) & (2 ** 64 - 1), int(epoch) & M32
    k = (seed & M32, seed >> 32)
    return philox((epoch, TAG, 0, 0), k) + philox((epoch, TAG, 1, 0), k)[:2]


def mix(v):
    """murmur3's 32-bit finaliser on a uint64 array of values below 2^32."""
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    v = v ^ (v >> np.uint64(13))
    v = (v * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    return v ^ (v >> np.uint64(16))


def split(M):
    bits = max(2, (int(M) - 1).bit_length())
    a = bits // 2
    return a, bits - a


def _mask(w):
    return np.uint64((1 << w) - 1)


def encrypt(key, a, b, x):
    L, R = x >> np.uint64(b), x & _mask(b)
    wl = a
    for r in range(ROUNDS):
        L, R = R, L ^ (mix(R ^ np.uint64(key[r])) & _mask(wl))
        wl = a + b - wl
    return (L << np.uint64(b)) | R


def decrypt(key, a, b, y):
    L, R = y >> np.uint64(b), y & _mask(b)
    wr = b
    for r in reversed(range(ROUNDS)):
        L, R = R ^ (mix(L ^ np.uint64(key[r])) & _mask(wr)), L
        wr = a + b - wr
    return (L << np.uint64(b)) | R


def _walk(fn, seed, epoch, M, p):
    p = np.atleast_1d(np.asarray(p)).astype(np.uint64)
    walks = np.zeros(p.shape, np.int64)
    if M <= 1:
        return np.zeros(p.shape, np.int64), walks
    key, (a, b) = keys(seed, epoch), split(M)
    x, todo = p.copy(), np.ones(p.shape, bool)
    while todo.any():
        x[todo] = fn(key, a, b, x[todo])
        walks[todo] += 1
        todo &= x >= np.uint64(M)
    return x.astype(np.int64), walks


def perm_index(seed, epoch, M, p, walks=False):
    """The sample indices of positions ``p`` (an int or an array) as an int64 array; with ``walks`` also the number
    of passes each took."""
    out, w = _walk(encrypt, seed, epoch, M, p)
    return (out, w) if walks else out


def perm_inverse(seed, epoch, M, i):
    return _walk(decrypt, seed, epoch, M, i)[0]


def permutation(seed, epoch, M):
    return perm_index(seed, epoch, M, np.arange(M))


def cursor_ticked(epoch, batch, n_batches):
    batch = batch if batch < n_batches else 0
    if batch + 1 == n_batches:
        return (epoch + 1) & M32, 0
    return epoch, batch + 1


def minibatch(seed, epoch, batch, M, B):
    """The indices of minibatch ``batch`` of epoch ``epoch``."""
    return perm_index(seed, epoch, M, batch * B + np.arange(B))
