"""The squashed gSDE head (usv_sde_squash_forward / _backward) restated from its definition in float64.

The normals are tests/sde_ref.py's.  Forward, per row and action k:

    u = mean + sum_j lat_j std_jk z_jk        var = sum_j lat_j^2 std_jk^2
    a = tanh(u)      om = 4 t / (1 + t)^2, t = exp(-2 |u|)      c = om + 1e-6
    env = low + (a + 1) * 0.5 * (high - low)
    logp = sum_k (-(u - mean)^2 / (2 s2) - 0.5 ln s2 - 0.5 ln 2 pi - ln c),  s2 = var + 1e-6

The backward is torch-CPU float64 autograd on exactly these lines (``grads``), not a second copy of the
gradient formulas.  It is taken at the program's own u and var (float32 values cast up): the graph is built
from the float64 u and var, whose values are then replaced by the program's without touching the graph, so the
comparison measures the backward and not the conditioning of the forward.

The backward's normals are the program's own too (float32 cast up), and they are compared with sde_ref.normals
on their own, as the existing head's are: "z" = |z - z_ref| / max(1, r).  A float32 Box-Muller normal is
accurate to a few 1e-7 of its radius r, not of itself: next to a zero of the cosine (|z| << r) its relative
error is unbounded, and the term gn std z of g_lat_j, with |W_jk| = std |z| in the scale below, inherits it where
lat_j = 0 leaves no other term.  Against sde_ref.normals' z the host replay's g_lat error is 7.4e-4 at
(65, 512, 1) (element z = -1.3e-4, r = 1.06) and 7.7e-6 at (257, 300, 2); at the program's z it is 1.9e-7 and
1.8e-7.  That error is the unchanged generator's, which "z" bounds; the gradient errors measure the backward.

Error scales (each error is divided by the sum of the absolute magnitudes of its terms):

    Sm_k  = |ga_k| + 2 |gl|                                              g_mean
    Sn_k  = Sm_k + |gl| |d_k| / s2_k        Sv_k = |gl| (d_k^2 / (2 s2_k^2) + 0.5 / s2_k)
    g_lat_j  : sum_k (Sn_k |std_jk z_jk| + Sv_k 2 |lat_j| std_jk^2)
    g_std_jk : sum_e (Sn_ek |lat_ej| |z_ejk| + Sv_ek 2 lat_ej^2 std_jk)
"""
import math

import numpy as np

import sde_ref as R

EPS = 1e-6
LOW, HIGH = (0.0, -1.0), (1.0, 1.0)
# (n, L, A): the last gives R = 2 rows per partial of g_std with a ragged final partial
SHAPES = ((1, 4, 1), (3, 64, 2), (5, 260, 2), (257, 300, 2), (65, 512, 1), (1027, 8, 2))
SEED, GID0, EPOCH = 11, 3, 2
CEILING = 1e-5


def inputs(n, L, A):
    """lat = relu(randn), log_std in -3 +- 1, mean in the action Box +- 1 (tests/test_gpu_sde.py's inputs with
    the SAC configuration's log_std); from two rows on, row 0 has an all-zero latent and the last row has
    mean = 12 (saturated: a = 1).  Upstream gradients ga [n, A] and gl [n] are standard normals."""
    rng = np.random.default_rng(1000 * n + 10 * L + A)
    lat = np.maximum(rng.standard_normal((n, L)), 0.0).astype(np.float32)
    std = np.exp(rng.uniform(-4.0, -2.0, (L, A))).astype(np.float32)
    lo, hi = np.float32(LOW[:A]), np.float32(HIGH[:A])
    mean = rng.uniform(lo - 1.0, hi + 1.0, (n, A)).astype(np.float32)
    ga = rng.standard_normal((n, A)).astype(np.float32)
    gl = rng.standard_normal((n,)).astype(np.float32)
    if n >= 2:
        lat[0] = 0.0
        mean[-1] = 12.0
    return mean, lat, std, ga, gl


def squash(u):
    t = np.exp(-2.0 * np.abs(u))
    return np.tanh(u), 4.0 * t / ((1.0 + t) * (1.0 + t))


def forward(seed, gid0, epoch, mean, lat, std):
    """dict of float64 u, u_scale (as sde_ref.sample's), var, z and r [n, L, A]."""
    u, scale, _ = R.sample(seed, gid0, epoch, mean, lat, std)
    lat, std = np.asarray(lat, np.float64), np.asarray(std, np.float64)
    z, r = R.normals(seed, gid0, epoch, lat.shape[0], lat.shape[1], std.shape[1])
    return {"u": u, "u_scale": scale, "var": (lat * lat) @ (std * std), "z": z, "r": r}


def logp_of(u, mean, var):
    """(logp [n], scale [n]) in float64 at the given u and var; scale = 1 + sum_k (d^2 / s2 + |ln s2| + |ln c|)."""
    u, mean, var = (np.asarray(x, np.float64) for x in (u, mean, var))
    s2, d = var + EPS, u - mean
    _, om = squash(u)
    lc = np.log(om + EPS)
    lp = (-d * d / (2.0 * s2) - 0.5 * np.log(s2) - 0.5 * math.log(2.0 * math.pi) - lc).sum(-1)
    return lp, 1.0 + (d * d / s2 + np.abs(np.log(s2)) + np.abs(lc)).sum(-1)


def unscale(a, low, high):
    """low + (a + 1) * 0.5 * (high - low) in a's dtype, in that order."""
    a = np.asarray(a)
    low, high = np.asarray(low, a.dtype), np.asarray(high, a.dtype)
    return low + ((a + a.dtype.type(1)) * a.dtype.type(0.5)) * (high - low)


def grads(z, mean, lat, std, u_at, var_at, ga, gl):
    """(g_mean, g_lat, g_std) of sum(ga * a) + sum(gl * logp) by torch float64 autograd, taken at u_at, var_at."""
    import torch
    t64 = lambda x, g=False: torch.tensor(np.asarray(x, np.float64), dtype=torch.float64, requires_grad=g)  # noqa: E731
    mean_t, lat_t, std_t = t64(mean, True), t64(lat, True), t64(std, True)
    u = mean_t + torch.einsum("ej,ejk->ek", lat_t, std_t[None] * t64(z))
    var = (lat_t * lat_t) @ (std_t * std_t)
    u = u + (t64(u_at) - u).detach()                      # the program's values on the definition's graph
    var = var + (t64(var_at) - var).detach()
    a = torch.tanh(u)
    t = torch.exp(-2.0 * u.abs())
    c = 4.0 * t / ((1.0 + t) * (1.0 + t)) + EPS
    s2, d = var + EPS, u - mean_t
    logp = (-(d * d) / (2.0 * s2) - 0.5 * torch.log(s2) - 0.5 * math.log(2.0 * math.pi) - torch.log(c)).sum(-1)
    ((t64(ga) * a).sum() + (t64(gl) * logp).sum()).backward()
    return mean_t.grad.numpy(), lat_t.grad.numpy(), std_t.grad.numpy()


def grad_scales(z, mean, lat, std, u_at, var_at, ga, gl):
    """(Sm [n, A], scale of g_lat [n, L], scale of g_std [L, A]) as in the module docstring."""
    z, mean, lat, std, u_at, var_at, ga, gl = (np.asarray(x, np.float64) for x in (z, mean, lat, std, u_at, var_at, ga, gl))
    s2, d, agl = var_at + EPS, u_at - mean, np.abs(gl)[:, None]
    Sm = np.abs(ga) + 2.0 * agl
    Sn = Sm + agl * np.abs(d) / s2
    Sv = agl * (d * d / (2.0 * s2 * s2) + 0.5 / s2)
    al = np.abs(lat)
    s_lat = np.einsum("ek,ejk->ej", Sn, np.abs(std[None] * z)) + 2.0 * al * (Sv @ (std * std).T)
    s_std = np.einsum("ek,ej,ejk->jk", Sn, al, np.abs(z)) + 2.0 * np.einsum("ek,ej->jk", Sv, lat * lat) * std
    return Sm, s_lat, s_std


def ratio(diff, scale):
    """diff / scale; where the scale is 0 the quantity has no non-zero term and must be exactly 0."""
    diff, scale = np.asarray(diff, np.float64), np.asarray(scale, np.float64)
    return np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(diff == 0, 0.0, np.inf))


def errors(got, case_inputs, seed=SEED, gid0=GID0, epoch=EPOCH):
    """The eight normalised maxima of a program's outputs `got` (dict of float32 arrays: z, gauss, act, var, logp,
    g_mean, g_lat, g_std) on inputs (mean, lat, std, ga, gl).  "a" is |act - tanh(gauss)|: tanh is bounded by 1."""
    mean, lat, std, ga, gl = case_inputs
    ref = forward(seed, gid0, epoch, mean, lat, std)
    u, var = got["gauss"].astype(np.float64), got["var"].astype(np.float64)
    vref = ref["var"]
    lp, lscale = logp_of(u, mean, vref)
    z = got["z"].astype(np.float64)
    gm, glat, gstd = grads(z, mean, lat, std, u, var, ga, gl)
    Sm, s_lat, s_std = grad_scales(z, mean, lat, std, u, var, ga, gl)
    mx = lambda x: float(np.max(x))                       # noqa: E731
    return {"z": mx(np.abs(z - ref["z"]) / np.maximum(1.0, ref["r"])),
            "u": mx(np.abs(u - ref["u"]) / ref["u_scale"]),
            "a": mx(np.abs(got["act"] - np.tanh(u))),
            "var": mx(np.abs(var - vref) / (vref + EPS)),
            "logp": mx(np.abs(got["logp"] - lp) / lscale),
            "g_mean": mx(ratio(np.abs(got["g_mean"] - gm), Sm)),
            "g_lat": mx(ratio(np.abs(got["g_lat"] - glat), s_lat)),
            "g_std": mx(ratio(np.abs(got["g_std"] - gstd), s_std))}
