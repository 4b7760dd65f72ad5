"""The gSDE evaluation head (usv_sde_eval_forward / _backward: PPO's evaluate_actions with the clipped surrogate)
restated from its definition in float64.

Forward, per row and action k, in NumPy:

    var = sum_j lat_j^2 std_jk^2        s2 = var + 1e-6        d = act - mean
    logp = sum_k (-d^2 / (2 s2) - 0.5 ln s2 - 0.5 ln 2 pi)
    ratio = exp(logp - old)             sur = min(ratio adv, clamp(ratio, 1 - c, 1 + c) adv)

The backward is torch-CPU float64 autograd on the ``Normal(mean, sqrt(var + 1e-6)).log_prob(act).sum(-1)``, ``exp``,
``clamp`` and ``torch.min`` lines (``grads``), not a second copy of the gradient formulas.  It is taken at the
program's own var, logp and ratio (float32 values cast up): the graph is built from the float64 values, which are
then replaced by the program's without touching the graph, as sde_squash_ref.grads does, so the comparison measures
the backward and not the conditioning of the forward.

Error scales (each error is divided by the sum of the absolute magnitudes of its terms):

    var      : var + 1e-6
    logp     : Sl = 1 + sum_k (d_k^2 / s2_k + |ln s2_k|)                         (sde_ref.logp_of's)
    ratio    : Sr = ratio (Sl + |old|)              the error of logp - old, carried through exp
    sur      : |adv| Sr                             adv = 0: the surrogate is exactly 0
    St       = |gl| + |gs| |ratio adv|              the row's gradient of logp
    g_mean_k : St |d_k| / s2_k                      d = 0: exactly 0
    Sv_k     = St (d_k^2 / (2 s2_k^2) + 0.5 / s2_k)
    g_lat_j  : sum_k Sv_k 2 |lat_j| std_jk^2
    g_std_jk : sum_e Sv_ek 2 lat_ej^2 std_jk
"""
import math

import numpy as np

import sde_ref as R
import sde_squash_ref as Q

EPS = 1e-6
CLIP = 0.2
SHAPES = Q.SHAPES
CEILING = Q.CEILING
ratio_of = Q.ratio                                       # diff / scale; a zero scale wants an exactly zero diff

# the directed rows: the ratio and the sign of the advantage.  0.79 and 1.21 are just past the clip bounds
# 0.8 and 1.2; every ratio meets a positive, a negative and a zero advantage.  The order lets the smallest shapes
# (n = 1, 3, 5) reach different ratios and signs with their few rows.
DIRECTED = ((0.5, 1.0), (0.79, -1.0), (1.0, 0.0), (1.21, 1.0), (1.5, -1.0),
            (0.5, -1.0), (0.79, 0.0), (1.0, 1.0), (1.21, -1.0), (1.5, 0.0),
            (0.5, 0.0), (0.79, 1.0), (1.0, -1.0), (1.21, 0.0), (1.5, 1.0))


def forward(mean, lat, std, act, old=None, adv=None, clip=CLIP):
    """dict of float64 var [n, A], logp, logp_scale [n] and, with old and adv, ratio and sur [n]."""
    mean, lat, std, act = (np.asarray(x, np.float64) for x in (mean, lat, std, act))
    lp, scale = R.logp_of(act, mean, lat, std)
    out = {"var": (lat * lat) @ (std * std), "logp": lp, "logp_scale": scale}
    if old is not None:
        old, adv = np.asarray(old, np.float64), np.asarray(adv, np.float64)
        ratio = np.exp(lp - old)
        out["ratio"] = ratio
        out["sur"] = np.minimum(ratio * adv, np.clip(ratio, 1.0 - clip, 1.0 + clip) * adv)
    return out


def inputs(n, L, A, clip=CLIP):
    """(mean, lat, std, act, old, adv, gl, gs) in float32.  lat = relu(randn), log_std in -3 +- 1 and mean as
    sde_squash_ref.inputs; actions = mean + N(0, 1) sqrt(var).  From two rows on, row 0 has an all-zero latent
    (s2 = 1e-6) and the last row has act == mean.  old is built from the float64 logp so that the first
    min(n, 15) rows have the DIRECTED ratios and advantages (|adv| drawn, its sign or zero directed) and the rest
    ratios log-uniform in [0.6, 1.6] (a draw within 5e-3 of 1 +- clip is moved to 5e-3 from it, no row is dropped)
    with normal advantages.  Asserted in float64: no ratio lies within 1e-3 of 1 +- clip: the
    gradient's discontinuity is away from every row.  Upstream gradients gl and gs [n] are standard normals."""
    rng = np.random.default_rng(7000 * n + 10 * L + A)
    lat = np.maximum(rng.standard_normal((n, L)), 0.0).astype(np.float32)
    std = np.exp(rng.uniform(-4.0, -2.0, (L, A))).astype(np.float32)
    lo, hi = np.float32(Q.LOW[:A]), np.float32(Q.HIGH[:A])
    mean = rng.uniform(lo - 1.0, hi + 1.0, (n, A)).astype(np.float32)
    if n >= 2:
        lat[0] = 0.0
    var = (lat.astype(np.float64) ** 2) @ (std.astype(np.float64) ** 2)
    act = (mean + rng.standard_normal((n, A)) * np.sqrt(var)).astype(np.float32)
    if n >= 2:
        act[-1] = mean[-1]
    target = np.exp(rng.uniform(math.log(0.6), math.log(1.6), n))
    for b in (1.0 - clip, 1.0 + clip):                   # a draw within 5e-3 of a bound moves to 5e-3 on its side
        near = np.abs(target - b) < 5e-3
        target[near] = b + np.where(target[near] < b, -5e-3, 5e-3)
    adv = rng.standard_normal(n)
    for i, (r, sign) in enumerate(DIRECTED[:n]):
        target[i], adv[i] = r, sign * (0.5 + abs(adv[i]))
    lp = forward(mean, lat, std, act)["logp"]
    old = (lp - np.log(target)).astype(np.float32)
    adv = adv.astype(np.float32)
    gl = rng.standard_normal(n).astype(np.float32)
    gs = rng.standard_normal(n).astype(np.float32)
    ratio = np.exp(lp - old.astype(np.float64))
    assert (np.abs(ratio - (1.0 - clip)) > 1e-3).all() and (np.abs(ratio - (1.0 + clip)) > 1e-3).all(), (n, L, A)
    return mean, lat, std, act, old, adv, gl, gs


def grads(mean, lat, std, act, old, adv, gl, gs, var_at, logp_at, ratio_at, clip=CLIP):
    """(g_mean, g_lat, g_std) of sum(gl * logp) + sum(gs * sur) by torch float64 autograd, taken at var_at, logp_at
    and ratio_at.  old = None: no surrogate."""
    import torch
    t64 = lambda x, g=False: torch.tensor(np.asarray(x, np.float64), dtype=torch.float64, requires_grad=g)  # noqa: E731
    mean_t, lat_t, std_t = t64(mean, True), t64(lat, True), t64(std, True)
    var = (lat_t * lat_t) @ (std_t * std_t)
    var = var + (t64(var_at) - var).detach()              # the program's values on the definition's graph
    logp = torch.distributions.Normal(mean_t, torch.sqrt(var + EPS), validate_args=False).log_prob(t64(act)).sum(-1)
    logp = logp + (t64(logp_at) - logp).detach()
    loss = (t64(gl) * logp).sum()
    if old is not None:
        ratio = torch.exp(logp - t64(old))
        ratio = ratio + (t64(ratio_at) - ratio).detach()
        a = t64(adv)
        loss = loss + (t64(gs) * torch.min(ratio * a, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a)).sum()
    loss.backward()
    return mean_t.grad.numpy(), lat_t.grad.numpy(), std_t.grad.numpy()


def grad_scales(mean, lat, std, act, adv, gl, gs, var_at, ratio_at):
    """(scale of g_mean [n, A], of g_lat [n, L], of g_std [L, A]) as in the module docstring; adv = None: no
    surrogate."""
    mean, lat, std, act, gl, var_at = (np.asarray(x, np.float64) for x in (mean, lat, std, act, gl, var_at))
    St = np.abs(gl)
    if adv is not None:
        St = St + np.abs(np.asarray(gs, np.float64)) * np.abs(np.asarray(ratio_at, np.float64) * np.asarray(adv, np.float64))
    s2, d = var_at + EPS, act - mean
    Sv = St[:, None] * (d * d / (2.0 * s2 * s2) + 0.5 / s2)
    return (St[:, None] * np.abs(d) / s2, 2.0 * np.abs(lat) * (Sv @ (std * std).T),
            2.0 * np.einsum("ek,ej->jk", Sv, lat * lat) * std)


def errors(got, case_inputs, clip=CLIP):
    """The seven normalised maxima of a program's outputs `got` (dict of float32 arrays: var, logp, ratio, sur,
    g_mean, g_lat, g_std) on `case_inputs` (inputs()'s tuple)."""
    mean, lat, std, act, old, adv, gl, gs = case_inputs
    ref = forward(mean, lat, std, act, old, adv, clip)
    var, logp, ratio = (got[k].astype(np.float64) for k in ("var", "logp", "ratio"))
    gm, glat, gstd = grads(mean, lat, std, act, old, adv, gl, gs, var, logp, ratio, clip)
    s_mean, s_lat, s_std = grad_scales(mean, lat, std, act, adv, gl, gs, var, ratio)
    Sr = ref["ratio"] * (ref["logp_scale"] + np.abs(old.astype(np.float64)))
    mx = lambda x: float(np.max(x))                       # noqa: E731
    return {"var": mx(np.abs(var - ref["var"]) / (ref["var"] + EPS)),
            "logp": mx(np.abs(logp - ref["logp"]) / ref["logp_scale"]),
            "ratio": mx(np.abs(ratio - ref["ratio"]) / Sr),
            "sur": mx(ratio_of(np.abs(got["sur"] - ref["sur"]), np.abs(adv.astype(np.float64)) * Sr)),
            "g_mean": mx(ratio_of(np.abs(got["g_mean"] - gm), s_mean)),
            "g_lat": mx(ratio_of(np.abs(got["g_lat"] - glat), s_lat)),
            "g_std": mx(ratio_of(np.abs(got["g_std"] - gstd), s_std))}
