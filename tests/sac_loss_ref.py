"""The fused SAC update (usv_sac_critic_loss / _policy_loss / _loss_backward / usv_polyak_update) restated twice.

``critic`` / ``policy`` / ``scaled`` / ``polyak``: NumPy float32 in the order gym-usv_amd/csrc/usv_sac_math.hpp fixes
(every operation rounded on its own; the sum over rows by partials of P = 1024 rows, 256 strands of four rows, a
balanced tree over each 64 strands, (w0 + w1) + (w2 + w3), partials ascending).  Programs are compared with it bit
for bit.

``torch_critic`` / ``torch_policy``: torch-CPU float64 autograd of SB3's own lines (``F.mse_loss``, ``torch.min``,
``.mean()``): the definition.  Errors against it are divided by the sum of the absolute magnitudes of the terms of
each quantity (``critic_scales`` / ``policy_scales``), with N_i = |r_i| + |(1 - d_i) disc_i| (|qn_i| + |ent logp'_i|)
the target's:

    target_i : N_i                                loss : 0.5 / B sum_k sum_i (|q_k,i| + N_i)^2
    g_q_k,i  : (|q_k,i| + N_i) / B
    actor    : sum_i (|ent logp_i| + |qmin_i|) / B    ent_coef_loss : sum_i |log_ent| (|logp_i| + |te|) / B
    g_logp   : |ent| / B     g_q_pi : 1 / B (w is exact)     g_log_ent : sum_i (|logp_i| + |te|) / B
"""
import numpy as np

P, STRANDS, LANES, C = 1024, 256, 64, 4096
ROWS = (1, 2, 63, 64, 65, 255, 256, 257, P - 1, P, P + 1, 2 * P + 1)
NUMELS = (1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3)
TAUS = (0.005, 0.0, 1.0)
CEILING = 1e-5                                            # on every normalised error: a condition
TE = -2.0                                                 # the example's target entropy, -act_dim
f32 = np.float32


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def same(a, b):
    """Bitwise equal, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def tree(s):
    """sde_tree_sum: neighbours first."""
    while len(s) > 1:
        s = s[0::2] + s[1::2]
    return s[0]


def partial_sum(term):
    """One partial of <= P float32 terms.  A strand starts from +0.0 and so never holds -0.0: the rows that do
    not exist may be added as +0.0."""
    pad = np.zeros(P, f32)
    pad[:len(term)] = term
    acc = np.zeros(STRANDS, f32)
    for row in pad.reshape(P // STRANDS, STRANDS):
        acc = acc + row
    w = [tree(acc[LANES * v:LANES * (v + 1)]) for v in range(STRANDS // LANES)]
    return (w[0] + w[1]) + (w[2] + w[3])


def fsum(term):
    term, acc = np.asarray(term, f32), f32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for at in range(0, len(term), P):
            acc = acc + partial_sum(term[at:at + P])
    return f32(acc)


def critic(q1, q2, q1t, q2t, rew, done, ent=None, logp_next=None, disc=None, gamma=None):
    """dict of float32 target, loss, g_q1, g_q2."""
    B = f32(len(q1))
    qn = np.minimum(q1t, q2t)
    if ent is not None:
        qn = qn - f32(ent) * logp_next
    d = disc if disc is not None else f32(gamma)
    tgt = rew + ((f32(1.0) - done) * d) * qn
    d1, d2 = q1 - tgt, q2 - tgt
    loss = f32(0.5) * (fsum(d1 * d1) / B + fsum(d2 * d2) / B)
    return {"target": tgt, "loss": f32(loss), "g_q1": d1 / B, "g_q2": d2 / B}


def policy(logp, q1, q2, ent, log_ent=None, te=None):
    """dict of float32 actor_loss, g_logp, g_q1, g_q2 and, with log_ent, ent_coef_loss and g_log_ent."""
    B, ent = f32(len(logp)), f32(ent)
    with np.errstate(invalid="ignore"):
        qmin = np.minimum(q1, q2)
        w = np.where(q1 < q2, f32(1.0), np.where(q1 == q2, f32(0.5), f32(0.0))).astype(f32)
    out = {"actor_loss": f32(fsum(ent * logp - qmin) / B), "g_logp": np.full(len(logp), ent / B, f32),
           "g_q1": -w / B, "g_q2": -(f32(1.0) - w) / B}
    if log_ent is not None:
        tg = logp + f32(te)
        out["ent_coef_loss"] = f32(-(fsum(f32(log_ent) * tg) / B))
        out["g_log_ent"] = f32(-(fsum(tg) / B))
    return out


def scaled(g, up):
    """usv_sac_loss_backward: the unit gradient times the upstream scalar; None: zeros."""
    g = np.asarray(g, f32)
    return np.zeros_like(g) if up is None else g * f32(up)


def polyak_coeffs(tau):
    return f32(tau), f32(1.0 - tau)


def polyak(t, p, tau):
    tau_f, om = polyak_coeffs(tau)
    return (np.asarray(t, f32) * om) + (tau_f * np.asarray(p, f32))


# ---- inputs
def inputs(B, seed=0, ent=0.2, nan_q2_pi=False):
    """dict of float32 row arrays [B] and the scalars.  dones are 0 and 1 (both from two rows on); q1_pi == q2_pi on
    every third row, below and above it on the others; per-row discounts are powers of float32(0.99)."""
    rng = np.random.default_rng(9000 * B + seed)
    n = lambda s=1.0, m=0.0: (m + s * rng.standard_normal(B)).astype(f32)  # noqa: E731
    done = (rng.random(B) < 0.3).astype(f32)
    if B >= 2:
        done[0], done[1] = 0.0, 1.0
    q1p, q2p = n(5.0), n(5.0)
    q2p[::3] = q1p[::3]
    if nan_q2_pi:
        q2p[B // 2] = np.nan
    disc = (np.float64(0.99) ** rng.integers(1, 4, B)).astype(f32)
    return {"q1": n(5.0), "q2": n(5.0), "q1t": n(5.0), "q2t": n(5.0), "rew": n(2.0), "done": done,
            "logp_next": n(2.0, -1.0), "disc": disc, "gamma": 0.99, "logp": n(2.0, -1.0), "q1p": q1p, "q2p": q2p,
            "ent": f32(ent), "log_ent": f32(np.log(ent)) if ent > 0 else f32(-3.0), "te": TE}


CRITIC_FORMS = ("disc", "gamma", "td3")


def critic_case(x, form):
    """critic()'s arguments for a form: per-row discounts, the scalar gamma, or TD3's target (gamma, no entropy)."""
    a = [x[k] for k in ("q1", "q2", "q1t", "q2t", "rew", "done")]
    if form == "td3":
        return a, dict(gamma=x["gamma"])
    kw = dict(ent=x["ent"], logp_next=x["logp_next"])
    kw.update(dict(disc=x["disc"]) if form == "disc" else dict(gamma=x["gamma"]))
    return a, kw


# ---- the definition, torch-CPU float64 autograd
def torch_critic(q1, q2, q1t, q2t, rew, done, ent=None, logp_next=None, disc=None, gamma=None):
    import torch
    import torch.nn.functional as F
    t = lambda v, g=False: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64, requires_grad=g)  # noqa: E731
    q1, q2 = t(q1, True), t(q2, True)
    with torch.no_grad():
        q_next = torch.min(t(q1t), t(q2t))
        if ent is not None:
            q_next = q_next - float(ent) * t(logp_next)
        target = t(rew) + (1 - t(done)) * (t(disc) if disc is not None else float(f32(gamma))) * q_next
    loss = 0.5 * (F.mse_loss(q1, target) + F.mse_loss(q2, target))
    loss.backward()
    return {"target": target.numpy(), "loss": float(loss.detach()), "g_q1": q1.grad.numpy(), "g_q2": q2.grad.numpy()}


def torch_policy(logp, q1, q2, ent, log_ent=None, te=None):
    import torch
    t = lambda v, g=False: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64, requires_grad=g)  # noqa: E731
    logp, q1, q2 = t(logp, True), t(q1, True), t(q2, True)
    actor = (float(ent) * logp - torch.min(q1, q2)).mean()
    out = {}
    if log_ent is not None:
        le = t(log_ent, True)
        ent_loss = -(le * (logp.detach() + float(te))).mean()
        ent_loss.backward()
        out["ent_coef_loss"], out["g_log_ent"] = float(ent_loss.detach()), float(le.grad)
    actor.backward()
    out.update(actor_loss=float(actor.detach()), g_logp=logp.grad.numpy(), g_q1=q1.grad.numpy(), g_q2=q2.grad.numpy())
    return out


def critic_scales(q1, q2, q1t, q2t, rew, done, ent=None, logp_next=None, disc=None, gamma=None):
    d64 = lambda v: np.asarray(v, np.float64)                # noqa: E731
    B = len(q1)
    qn = np.abs(np.minimum(d64(q1t), d64(q2t)))
    if ent is not None:
        qn = qn + np.abs(float(ent) * d64(logp_next))
    N = np.abs(d64(rew)) + np.abs((1 - d64(done)) * (d64(disc) if disc is not None else float(f32(gamma)))) * qn
    s1, s2 = np.abs(d64(q1)) + N, np.abs(d64(q2)) + N
    return {"target": N, "loss": 0.5 / B * float((s1 * s1).sum() + (s2 * s2).sum()), "g_q1": s1 / B, "g_q2": s2 / B}


def policy_scales(logp, q1, q2, ent, log_ent=None, te=None):
    d64 = lambda v: np.asarray(v, np.float64)                # noqa: E731
    B, lp = len(logp), np.abs(d64(logp))
    out = {"actor_loss": float((np.abs(float(ent)) * lp + np.abs(np.minimum(d64(q1), d64(q2)))).sum()) / B,
           "g_logp": np.full(B, abs(float(ent)) / B), "g_q1": np.full(B, 1.0 / B), "g_q2": np.full(B, 1.0 / B)}
    if log_ent is not None:
        out["g_log_ent"] = float((lp + abs(te)).sum()) / B
        out["ent_coef_loss"] = abs(float(log_ent)) * out["g_log_ent"]
    return out


def errors(got, ref, scales):
    """The largest normalised error of every quantity of `ref` (a zero scale wants an exactly zero difference)."""
    out = {}
    for k, r in ref.items():
        diff, s = np.abs(np.asarray(got[k], np.float64) - r), np.asarray(scales[k], np.float64)
        ok = s > 0
        assert (diff[~ok] == 0).all() if diff.ndim else (ok or diff == 0), k
        out[k] = float(np.max(np.where(ok, diff / np.where(ok, s, 1.0), 0.0)))
    return out
