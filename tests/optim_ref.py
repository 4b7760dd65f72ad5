"""The fused optimizer step (usv_adam_step: clip_grad_norm_ and Adam.step() over a tensor list) restated twice.

``step`` / ``total_norm``: NumPy float32 in the order gym-usv_amd/csrc/usv_optim_math.hpp fixes (every operation
rounded on its own; the sum of squares by chunks of C = 4096 elements, 256 strands of four groups of four consecutive
elements, a balanced tree over each 64 strands, (w0 + w1) + (w2 + w3), chunk sums ascending over the list).  Programs
are compared with it bit for bit.

``torch_step``: ``torch.nn.utils.clip_grad_norm_`` and ``torch.optim.Adam`` on CPU in float64, one step from the same
state cast up: the definition.  Errors against it are divided by the sum of the magnitudes of the terms of each
quantity (``scales``):

    p' : |p| + |step_size m' / denom|      m' : |m| + |g'|      v' : |v beta2| + |(1 - beta2) g'^2|      total : total
"""
import math

import numpy as np

from sac_loss_ref import bits, same, tree  # noqa: F401

C, STRANDS, LANES, GROUP, K = 4096, 256, 64, 4, 96
CEILING = 1e-5                                            # on every normalised error: a condition
CLIP_EPS = 1e-6
f32 = np.float32
NUMELS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
MANY = tuple(1 + (5 * i + i // 7) % 7 for i in range(130))  # 130 tensors of 1-7 elements: two launches per pass
BIG = 65 * C + 1                                          # 66 chunk sums: more than the 64 one wave adds at once
STEPS = (1, 2, 1000)
HYPER = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8)


def chunk_sqsum(g):
    """One chunk of <= C float32 elements.  A strand starts from +0.0 and adds squares, so it never holds -0.0: the
    elements that do not exist may be added as +0.0."""
    pad = np.zeros(C, f32)
    pad[:len(g)] = g
    sq = (pad * pad).reshape(C // (GROUP * STRANDS), STRANDS, GROUP)      # [j][strand][k]: element 4 (s + 256 j) + k
    acc = np.zeros(STRANDS, f32)
    for j in range(sq.shape[0]):
        for k in range(GROUP):
            acc = acc + sq[j, :, k]
    w = [tree(acc[LANES * v:LANES * (v + 1)]) for v in range(STRANDS // LANES)]
    return (w[0] + w[1]) + (w[2] + w[3])


def total_norm(grads):
    """sqrt of the chunk sums added in ascending order from +0.0, tensors in list order."""
    acc = f32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in grads:
            g = np.asarray(g, f32).reshape(-1)
            for at in range(0, len(g), C):
                acc = f32(acc + chunk_sqsum(g[at:at + C]))
        return f32(np.sqrt(acc))


def scalars(t, lr, beta1, beta2, eps):
    """The host's doubles, each cast once."""
    bc1 = 1.0 - beta1 ** t
    bc2 = 1.0 - beta2 ** t
    return {"om_b1": f32(1.0 - beta1), "b2": f32(beta2), "om_b2": f32(1.0 - beta2), "eps": f32(eps),
            "step_size": f32(lr / bc1), "bc2_sqrt": f32(math.sqrt(bc2))}


def clip_coef(total, max_norm):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = f32(max_norm) / (f32(total) + f32(CLIP_EPS))
    return f32(1.0) if c > 1.0 else f32(c)                # a NaN stays


def step(ps, gs, ms, vs, t, lr=HYPER["lr"], beta1=HYPER["beta1"], beta2=HYPER["beta2"], eps=HYPER["eps"], max_norm=None):
    """One step over the lists of float32 arrays: (p', m', v', total); total is None without ``max_norm``."""
    s = scalars(t, lr, beta1, beta2, eps)
    total = coef = None
    if max_norm is not None:
        total = total_norm(gs)
        coef = clip_coef(total, max_norm)
    po, mo, vo = [], [], []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for p, g, m, v in zip(ps, gs, ms, vs):
            p, g, m, v = (np.asarray(x, f32) for x in (p, g, m, v))
            if coef is not None:
                g = g * coef
            m2 = m + (g - m) * s["om_b1"]
            v2 = v * s["b2"] + (s["om_b2"] * g) * g
            denom = np.sqrt(v2) / s["bc2_sqrt"] + s["eps"]
            po.append((p - s["step_size"] * (m2 / denom)).astype(f32))
            mo.append(m2.astype(f32))
            vo.append(v2.astype(f32))
    return po, mo, vo, total


# ---- inputs
def inputs(numels, seed=0, scale=None, bad=None):
    """(p, g, m, v) lists of float32 arrays.  m and v are a plausible state (v >= 0); ``scale``: a function of the
    tensor's index that scales its gradient; ``bad``: a value (inf, NaN) put at the middle of the middle tensor's
    gradient."""
    rng = np.random.default_rng(77000 + 31 * len(numels) + numels[0] + seed)
    ps, gs, ms, vs = [], [], [], []
    for i, n in enumerate(numels):
        k = f32(1.0 if scale is None else scale(i))
        ps.append(rng.standard_normal(n).astype(f32))
        gs.append((k * rng.standard_normal(n)).astype(f32))
        ms.append((f32(0.1) * k * rng.standard_normal(n)).astype(f32))
        vs.append((f32(0.01) * k * k * rng.standard_normal(n) ** 2).astype(f32))
    if bad is not None:
        g = gs[len(gs) // 2]
        g[len(g) // 2] = bad
    return ps, gs, ms, vs


def state_offsets(numels):
    """The offset of every tensor's segment in the flat m and v, and their length."""
    at, out = 0, []
    for n in numels:
        out.append(at)
        at += (n + 3) // 4 * 4
    return out, at


def chunks(numels):
    return sum((n + C - 1) // C for n in numels)


# ---- the definition, torch-CPU float64
def torch_step(ps, gs, ms, vs, t, lr=HYPER["lr"], beta1=HYPER["beta1"], beta2=HYPER["beta2"], eps=HYPER["eps"],
               max_norm=None):
    import torch
    tt = lambda x: torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)  # noqa: E731
    params = [torch.nn.Parameter(tt(p)) for p in ps]
    for p, g in zip(params, gs):
        p.grad = tt(g)
    opt = torch.optim.Adam(params, lr=lr, betas=(beta1, beta2), eps=eps)
    sd = opt.state_dict()                                  # the state before this step
    sd["state"] = {i: {"step": torch.tensor(float(t - 1)), "exp_avg": tt(m), "exp_avg_sq": tt(v)}
                   for i, (m, v) in enumerate(zip(ms, vs))}
    opt.load_state_dict(sd)
    total = None
    if max_norm is not None:
        total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    opt.step()
    st = opt.state_dict()["state"]
    return ([p.detach().numpy() for p in params], [st[i]["exp_avg"].numpy() for i in range(len(ps))],
            [st[i]["exp_avg_sq"].numpy() for i in range(len(ps))], total)


def scales(ps, gs, ms, vs, t, lr=HYPER["lr"], beta1=HYPER["beta1"], beta2=HYPER["beta2"], eps=HYPER["eps"], max_norm=None):
    """The sums of magnitudes, in float64 from the float64 definition's own terms."""
    d64 = lambda x: np.asarray(x, np.float64)              # noqa: E731
    coef = 1.0
    if max_norm is not None:
        total = math.sqrt(sum(float((d64(g) ** 2).sum()) for g in gs))
        coef = min(1.0, max_norm / (total + CLIP_EPS))
    step_size, bc2_sqrt = lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t)
    sp, sm, sv = [], [], []
    for p, g, m, v in zip(ps, gs, ms, vs):
        p, g, m, v = d64(p), d64(g) * coef, d64(m), d64(v)
        m2 = m + (g - m) * (1.0 - beta1)
        v2 = v * beta2 + (1.0 - beta2) * g * g
        sp.append(np.abs(p) + np.abs(step_size * m2 / (np.sqrt(v2) / bc2_sqrt + eps)))
        sm.append(np.abs(m) + np.abs(g))
        sv.append(np.abs(v * beta2) + np.abs((1.0 - beta2) * g * g))
    return sp, sm, sv


def errors(got, ref, sc):
    """The largest normalised error of p', m', v' over lists of arrays (a zero scale wants an exactly zero difference)."""
    out = {}
    for name, a, b, s in zip(("p", "m", "v"), got[:3], ref[:3], sc):
        worst = 0.0
        for x, y, z in zip(a, b, s):
            diff = np.abs(np.asarray(x, np.float64) - y)
            ok = z > 0
            assert (diff[~ok] == 0).all(), name
            worst = max(worst, float(np.max(np.where(ok, diff / np.where(ok, z, 1.0), 0.0))))
        out[name] = worst
    if ref[3] is not None:
        out["total"] = abs(float(got[3]) - ref[3]) / ref[3]
    return out
