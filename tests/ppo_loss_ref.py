"""The fused PPO loss (usv_ppo_loss / usv_ppo_explained_variance) restated from its definition.

``define``: SB3's ``PPO.train`` lines for one minibatch in NumPy float64 (advantage normalisation with the
``len(advantages) > 1`` guard and torch's unbiased std, the clipped surrogate, ``clip_range_vf``, ``F.mse_loss``, the
entropy stand-in ``-log_prob`` where there is no entropy tensor, SB3's order of the weighted sum, ``approx_kl`` and
``clip_fraction``); ``explained64``: ``common/utils.py``'s ``explained_variance``.  ``torch_define``: the same lines in
torch-CPU float64 with the backward by autograd (``g_logp``, ``g_values``, ``g_entropy`` at unit upstream of ``loss``):
not a second copy of the gradient formulas.

``moments32`` / ``explained32``: the moments alone in NumPy float32 in the order gym-usv_amd/csrc/usv_ppo_math.hpp
fixes (two passes, every operation rounded on its own, the sums by ``sac_loss_ref.fsum``).  Programs are compared with
them bit for bit.

Error scales (``scales``): each error is divided by the sum of the absolute magnitudes of its terms.  With
M = mean|adv|, sd the float64 std, and per row  Sa = (|adv| + M) / (sd + 1e-8) + |a| Ssd / sd  (Sa = 0 without
normalisation: a is the input),  Sr = ratio (1 + |logp| + |old|)  (the rounding of logp - old carried through exp,
and exp's own),  P = Sr |a| + ratio Sa,  V = |v| without a value clip and 2 |old_v| + |v| with one:

    mean : M                                   std  : Ssd = sum (|adv| + M)^2 / (2 sd (B - 1)) + sd
    policy_loss : sum P / B                    value_loss : sum (|ret| + V)^2 / B      entropy_loss : sum |term| / B
    loss : the three with |ent_coef| and |vf_coef|
    approx_kl : sum (Sr + 1 + |logp| + |old|) / B             clip_fraction : itself (the count is exact)
    g_logp : (P + |ent_coef| without an entropy tensor) / B   g_values : 2 |vf_coef| (|ret| + V) / B
    g_entropy : |ent_coef| / B
    explained_variance : 1 + (vr / vy) (Sv(r) / vr + Sv(y) / vy),  Sv(x) = sum (|x| + mean|x|)^2 / B, |r| = |ret| + |v|
"""
import math

import numpy as np

import sac_loss_ref as S
from sde_eval_ref import DIRECTED

f32 = np.float32
P = S.P
CLIP, CLIP_VF, VF_COEF, ENT_COEF, ADV_EPS = 0.2, 0.25, 0.5, 0.01, 1e-8
ROWS = (1, 2, 3, 255, 256, 257, P - 1, P, P + 1, 2 * P + 1, 65 * P + 1)
FORM_ROWS = (1, 257, 2 * P + 1)
FORMS = tuple(dict(normalize=n, clip_vf=c, entropy=e) for n in (True, False) for c in (None, CLIP_VF) for e in (False, True))
FULL_FORM = FORMS[0]                                      # normalisation on, no value clip, no entropy tensor
NAMES = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")
MARGIN = 1e-4                                             # no | |ratio - 1| - clip | and no | |dv| - clip_vf | below it
VALUE_STEPS = (-0.5, -0.25, -0.125, 0.0, 0.125, 0.25, 0.5)

d64 = lambda v: np.asarray(v, np.float64)                 # noqa: E731


def inputs(B, seed=0, adv_mean=0.0, clip=CLIP, clip_vf=CLIP_VF):
    """dict of float32 row arrays [B]: logp, old_logp, adv (mean adv_mean standard deviations), values, old_values,
    returns, entropy.  Ratios are log-uniform in [0.6, 1.6]; a row whose float64 | |ratio - 1| - clip | is below
    MARGIN has its old_logp shifted by 0.01, and one whose | |values - old_values| - clip_vf | is has its values
    shifted by 0.01 (``margins_hold`` is the tests' assertion that none is left)."""
    rng = np.random.default_rng(31000 * B + seed)
    n = lambda s=1.0, m=0.0: (m + s * rng.standard_normal(B)).astype(f32)  # noqa: E731
    logp = n(2.0, -1.0)
    old = (d64(logp) - rng.uniform(math.log(0.6), math.log(1.6), B)).astype(f32)
    near = np.abs(np.abs(np.exp(d64(logp) - d64(old)) - 1.0) - clip) < MARGIN
    old[near] += f32(0.01)
    old_values = n(3.0)
    values = (old_values + n(0.3)).astype(f32)
    near = np.abs(np.abs(d64(values) - d64(old_values)) - clip_vf) < MARGIN
    values[near] += f32(0.01)
    return {"logp": logp, "old_logp": old, "adv": n(1.0, adv_mean), "values": values, "old_values": old_values,
            "returns": (old_values + n(1.0)).astype(f32), "entropy": n(0.5, 1.4)}


def margins_hold(x, clip=CLIP, clip_vf=CLIP_VF):
    r = np.exp(d64(x["logp"]) - d64(x["old_logp"]))
    dv = d64(x["values"]) - d64(x["old_values"])
    return bool((np.abs(np.abs(r - 1.0) - clip) >= MARGIN).all() and (np.abs(np.abs(dv) - clip_vf) >= MARGIN).all())


def directed(B, clip=CLIP):
    """inputs() whose rows take sde_eval_ref.DIRECTED's ratios and advantage signs in turn (|adv| drawn; a ratio of 1.0
    has old_logp == logp, so it is exactly 1) and VALUE_STEPS in turn: old_values = 1.0, values = 1.0 + step, exact in
    float32.  Also the directed (ratio, sign) of every row."""
    x = inputs(B, seed=77)
    rows = [DIRECTED[i % len(DIRECTED)] for i in range(B)]
    ratio, sign = np.array([r for r, _ in rows]), np.array([s for _, s in rows])
    x["old_logp"] = (d64(x["logp"]) - np.log(ratio)).astype(f32)
    x["old_logp"][ratio == 1.0] = x["logp"][ratio == 1.0]
    x["adv"] = (sign * (0.5 + np.abs(x["adv"]))).astype(f32)
    x["old_values"] = np.ones(B, f32)
    x["values"] = (1.0 + np.array([VALUE_STEPS[i % len(VALUE_STEPS)] for i in range(B)])).astype(f32)
    assert ((d64(x["values"]) - 1.0) == [VALUE_STEPS[i % len(VALUE_STEPS)] for i in range(B)]).all()
    return x, ratio, sign


def normalised(B, form):
    return bool(form["normalize"]) and B > 1


def define(x, form, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF):
    """dict of float64: the six outputs and, with normalisation, mean and std; ratio and a per row."""
    logp, old, adv, v, old_v, ret, ent = (d64(x[k]) for k in ("logp", "old_logp", "adv", "values", "old_values",
                                                              "returns", "entropy"))
    B, out = len(logp), {}
    a = adv
    if normalised(B, form):
        out["mean"], out["std"] = adv.mean(), adv.std(ddof=1)
        a = (adv - out["mean"]) / (out["std"] + ADV_EPS)
    ratio = np.exp(logp - old)
    policy = -np.minimum(a * ratio, a * np.clip(ratio, 1.0 - clip, 1.0 + clip)).mean()
    vp = v if form["clip_vf"] is None else old_v + np.clip(v - old_v, -form["clip_vf"], form["clip_vf"])
    value = ((ret - vp) ** 2).mean()
    entropy = -np.mean(ent) if form["entropy"] else -np.mean(-logp)
    out.update(loss=policy + ent_coef * entropy + vf_coef * value, policy_loss=policy, value_loss=value,
               entropy_loss=entropy, approx_kl=np.mean((ratio - 1.0) - (logp - old)),
               clip_fraction=np.mean((np.abs(ratio - 1.0) > clip).astype(np.float64)), ratio=ratio, a=a)
    return out


def torch_define(x, form, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF):
    """SB3's lines in torch-CPU float64 and their autograd: the six outputs as floats, g_logp, g_values, g_entropy
    (zeros without an entropy tensor) as arrays."""
    import torch
    import torch.nn.functional as F
    t = lambda k, g=False: torch.tensor(d64(x[k]), dtype=torch.float64, requires_grad=g)  # noqa: E731
    log_prob, values, entropy = t("logp", True), t("values", True), t("entropy", True)
    advantages, old_log_prob, old_values, returns = t("adv"), t("old_logp"), t("old_values"), t("returns")
    if form["normalize"] and len(advantages) > 1:
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    ratio = torch.exp(log_prob - old_log_prob)
    policy_loss_1 = advantages * ratio
    policy_loss_2 = advantages * torch.clamp(ratio, 1 - clip, 1 + clip)
    policy_loss = -torch.min(policy_loss_1, policy_loss_2).mean()
    clip_fraction = torch.mean((torch.abs(ratio - 1) > clip).double()).item()
    if form["clip_vf"] is None:
        values_pred = values
    else:
        values_pred = old_values + torch.clamp(values - old_values, -form["clip_vf"], form["clip_vf"])
    value_loss = F.mse_loss(returns, values_pred)
    entropy_loss = -torch.mean(entropy) if form["entropy"] else -torch.mean(-log_prob)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        log_ratio = log_prob - old_log_prob
        approx_kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio).item()
    loss.backward()
    return {"loss": loss.item(), "policy_loss": policy_loss.item(), "value_loss": value_loss.item(),
            "entropy_loss": entropy_loss.item(), "approx_kl": approx_kl, "clip_fraction": clip_fraction,
            "g_logp": log_prob.grad.numpy(), "g_values": values.grad.numpy(),
            "g_entropy": entropy.grad.numpy() if entropy.grad is not None else np.zeros(len(x["logp"]))}


def reference(x, form, **kw):
    """What a program is compared with: define()'s outputs and moments, torch_define()'s gradients."""
    ref, t = define(x, form, **kw), torch_define(x, form, **kw)
    out = {k: ref[k] for k in NAMES + (("mean", "std") if "mean" in ref else ())}
    out.update(g_logp=t["g_logp"], g_values=t["g_values"])
    if form["entropy"]:
        out["g_entropy"] = t["g_entropy"]
    return out


def explained64(values, returns):
    y, r = d64(returns), d64(returns) - d64(values)
    return float("nan") if np.var(y) == 0 else float(1.0 - np.var(r) / np.var(y))


# ---- the float32 order of the moments
def moments32(adv):
    """(mean, std) of B > 1 advantages."""
    adv, B = np.asarray(adv, f32), len(adv)
    mean = S.fsum(adv) / f32(B)
    d = adv - mean
    return f32(mean), f32(np.sqrt(S.fsum(d * d) / f32(B - 1)))


def explained32(values, returns):
    y, B = np.asarray(returns, f32), f32(len(returns))
    r = y - np.asarray(values, f32)
    my, mr = S.fsum(y) / B, S.fsum(r) / B
    dy, dr = y - my, r - mr
    vy, vr = S.fsum(dy * dy) / B, S.fsum(dr * dr) / B
    with np.errstate(invalid="ignore", divide="ignore"):
        return f32(np.nan) if vy == 0 else f32(f32(1.0) - vr / vy)


# ---- error scales
def spread_scale(mag):
    """Sv: the sum of the squared deviations' magnitudes over B, from the magnitudes of the values."""
    return float(((mag + mag.mean()) ** 2).sum()) / len(mag)


def scales(x, form, clip=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF):
    logp, old, adv, v, old_v, ret, ent = (np.abs(d64(x[k])) for k in ("logp", "old_logp", "adv", "values", "old_values",
                                                                      "returns", "entropy"))
    B, ref, out = len(logp), define(x, form, clip, vf_coef, ent_coef), {}
    Sa = np.zeros(B)
    if normalised(B, form):
        M, sd = adv.mean(), ref["std"]
        Ssd = float(((adv + M) ** 2).sum()) / (2.0 * sd * (B - 1)) + sd
        Sa = (adv + M) / (sd + ADV_EPS) + np.abs(ref["a"]) * Ssd / sd
        out.update(mean=M, std=Ssd)
    Sr = ref["ratio"] * (1.0 + logp + old)
    Pr = Sr * np.abs(ref["a"]) + ref["ratio"] * Sa
    V = v if form["clip_vf"] is None else 2.0 * old_v + v
    term = ent if form["entropy"] else logp
    out.update(policy_loss=Pr.sum() / B, value_loss=((ret + V) ** 2).sum() / B, entropy_loss=term.sum() / B,
               approx_kl=(Sr + 1.0 + logp + old).sum() / B, clip_fraction=ref["clip_fraction"],
               g_logp=(Pr + (0.0 if form["entropy"] else abs(ent_coef))) / B, g_values=2.0 * abs(vf_coef) * (ret + V) / B)
    out["loss"] = out["policy_loss"] + abs(ent_coef) * out["entropy_loss"] + abs(vf_coef) * out["value_loss"]
    if form["entropy"]:
        out["g_entropy"] = np.full(B, abs(ent_coef) / B)
    return out


def explained_scale(values, returns):
    y, v = d64(returns), d64(values)
    vy, vr = np.var(y), np.var(y - v)
    return 1.0 + (vr / vy) * (spread_scale(np.abs(y) + np.abs(v)) / vr + spread_scale(np.abs(y)) / vy)



def cases():
    """(B, form, inputs): every form at FORM_ROWS, the full row list for FULL_FORM, and advantage means of 5 and 100
    standard deviations for the moments."""
    out = [(B, form, inputs(B, seed=j)) for j, form in enumerate(FORMS) for B in FORM_ROWS]
    out += [(B, FULL_FORM, inputs(B, seed=9)) for B in ROWS if B not in FORM_ROWS]
    out += [(B, FULL_FORM, inputs(B, seed=10 + int(m), adv_mean=m)) for B in (3, 257, 2 * P + 1) for m in (5.0, 100.0)]
    return out


def check_directed(got, x, ratio, sign, B):
    """`got` is unpack()'s dict for directed(B) with an entropy tensor, normalisation off."""
    clipped = np.abs(ratio - 1.0) > CLIP
    assert S.same([got["clip_fraction"]], [np.float32(clipped.sum()) / np.float32(B)])
    gl = np.asarray(got["g_logp"], np.float32)
    assert (S.bits(gl[sign == 0]) << 1 == 0).all()                      # a zero advantage: exactly zero, either sign
    tie = (ratio == 1.0) & (sign != 0)                                   # unclipped, s1 == s2: the whole gradient
    assert S.same(gl[tie], (np.float32(-1.0) / np.float32(B)) * x["adv"][tie])
    # a clipped row passes no gradient where the clipped branch is the min: ratio above with adv > 0, below with adv < 0
    dead = ((ratio > 1.0 + CLIP) & (sign > 0)) | ((ratio < 1.0 - CLIP) & (sign < 0))
    live = clipped & ~dead & (sign != 0)
    assert dead.any() and live.any() and (S.bits(gl[dead]) << 1 == 0).all() and (gl[live] != 0).all()
    gv = np.asarray(got["g_values"], np.float32)
    dv = np.asarray(x["values"], np.float64) - 1.0
    inside = np.abs(dv) <= CLIP_VF
    assert (np.abs(dv) == CLIP_VF).any() and (~inside).any()
    assert (S.bits(gv[~inside]) << 1 == 0).all()
    want = ((np.float32(2.0) * np.float32(VF_COEF)) * (x["values"] - x["returns"])) / np.float32(B)
    assert S.same(gv[inside], want[inside])


errors = S.errors                                         # the largest normalised error of every quantity of ref
