"""The fused PPO loss on the GPU (gym_usv_amd.DevicePPOLoss: usv_ppo_loss / usv_ppo_explained_variance).

Bitwise, against the NumPy float32 restatement (tests/ppo_loss_ref.py): the advantage moments and the explained
variance.  Against the float64 definition (NumPy forward, torch-CPU autograd backward): every loss, statistic and
gradient, each error divided by the sum of the absolute magnitudes of its terms, measured over ppo_loss_ref.cases()
(every form at 1, 257 and 2 049 rows, the full row list for one form, advantage means of 5 and 100 standard
deviations), printed, and bounded at 4x the maximum measured on the MI355X (MEASURED below); independently each must
stay below the ceiling of 1e-5, a condition and not a measurement.

Exact properties as integers: the directed rows' clip count, torch.min's and torch.clamp's ties, the value clamp's
inclusive bounds; sentinels around every output; the same bits from a repeated call, a second stream and a small batch
after a large one on the same scratch.  The autograd wiring through DeviceSDE.evaluate and a linear value layer
against torch autograd of the torch lines on the same tensors, and the example's trainer in three modes."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import ppo_loss_ref as R
import sac_loss_ref as S
import sde_eval_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# maxima over R.cases() on the MI355X (rounded up)
MEASURED = {"loss": 1.85e-8, "policy_loss": 2.38e-8, "value_loss": 1.97e-8, "entropy_loss": 1.08e-7,
            "approx_kl": 9.74e-9, "clip_fraction": 4.61e-8, "mean": 9.48e-8, "std": 2.49e-8,
            "g_logp": 1.12e-7, "g_values": 1.17e-7, "g_entropy": 3.77e-8, "explained_variance": 1.12e-9}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
KEYS = ("logp", "old_logp", "adv", "values", "old_values", "returns", "entropy")


def dev():
    return torch.device("cuda", 0)


def to_dev(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(np.atleast_1d(np.asarray(x, np.float32)))).to(dev()).requires_grad_(grad)


def host(t):
    return t.detach().cpu().numpy().reshape(-1)


@pytest.fixture(scope="module")
def pl():
    from gym_usv_amd import DevicePPOLoss
    return DevicePPOLoss(dev())


def run_loss(pl, x, form, up=1.0, grad=True, column=False):
    """The device's six outputs, the moments and the gradients of up * loss, as ppo_loss_ref.reference()'s dict."""
    B = len(x["logp"])
    t = {k: to_dev(x[k], grad and k in ("logp", "values", "entropy")) for k in KEYS}
    if column:
        t = {k: v.detach().reshape(-1, 1).requires_grad_(v.requires_grad) for k, v in t.items()}
    cvf = form["clip_vf"]
    out = pl.loss(t["logp"], t["old_logp"], t["adv"], t["values"], t["returns"], clip_range=R.CLIP, vf_coef=R.VF_COEF,
                  ent_coef=R.ENT_COEF, normalize_advantage=form["normalize"], old_values=None if cvf is None else t["old_values"],
                  clip_range_vf=cvf, entropy=t["entropy"] if form["entropy"] else None)
    assert all(o.shape == () for o in out) and not any(o.requires_grad for o in out[1:])
    got = {k: host(o)[0] for k, o in zip(R.NAMES, out)}
    if R.normalised(B, form):
        got["mean"], got["std"] = host(pl.moments)
    else:
        assert pl.moments is None
    if grad:
        (out.loss * up).backward()
        got.update(g_logp=host(t["logp"].grad), g_values=host(t["values"].grad))
        if form["entropy"]:
            got["g_entropy"] = host(t["entropy"].grad)
        else:
            assert t["entropy"].grad is None
    else:
        assert not out.loss.requires_grad
    return got


def test_moments_bitwise_and_errors_against_the_float64_definition(pl):
    worst = {}
    for n, (B, form, x) in enumerate(R.cases()):
        assert R.margins_hold(x), B                       # the count comparison leaves no row out
        got = run_loss(pl, x, form, column=n % 2 == 1)
        if R.normalised(B, form):
            assert S.same([got["mean"], got["std"]], R.moments32(x["adv"])), (B, form)
        ref = R.reference(x, form)
        count = np.float32(round(ref["clip_fraction"] * B))
        assert S.same([got["clip_fraction"]], [count / np.float32(B)]), (B, form)
        for k, v in R.errors(got, ref, R.scales(x, form)).items():
            worst[k] = max(worst.get(k, 0.0), v)
        plain = run_loss(pl, x, form, grad=False)           # nothing saved: the same bits
        assert all(S.same([plain[k]], [got[k]]) for k in R.NAMES), (B, form)
    print("ppo loss errors:", {k: f"{v:.3e}" for k, v in sorted(worst.items())})
    assert set(worst) == set(BOUND) - {"explained_variance"}
    for k, v in worst.items():
        assert v <= BOUND[k] and v < S.CEILING, (k, v, BOUND[k])


def test_upstream_scalars_scale_the_unit_gradients(pl):
    x, form = R.inputs(257, seed=2), R.FORMS[3]
    unit = run_loss(pl, x, form)
    for up in (3.0, -0.37):
        got = run_loss(pl, x, form, up)
        for k in ("g_logp", "g_values", "g_entropy"):
            assert S.same(got[k], S.scaled(unit[k], up)), (up, k)


def test_directed_rows_exactly(pl):
    form = dict(normalize=False, clip_vf=R.CLIP_VF, entropy=True)
    for B in (45, R.P + 45):
        x, ratio, sign = R.directed(B)
        R.check_directed(run_loss(pl, x, form), x, ratio, sign, B)


def test_outputs_sit_between_untouched_sentinels(pl):
    """The C entry itself, its outputs inside one sentinel-filled buffer: [pad | g_logp | pad | g_values | pad |
    (g_entropy, not asked for) | pad | out | pad | moments | pad]."""
    from gym_usv_amd import _lib
    B, pad, mark = 2 * R.P + 1, 8, 12345.0
    x = R.inputs(B, seed=4)
    t = {k: to_dev(x[k]) for k in KEYS}
    for normalize in (1, 0):
        buf = torch.full((3 * B + 5 * pad + 6 + 2 + pad,), mark, device=dev())
        at = lambda i: buf.data_ptr() + 4 * i             # noqa: E731
        o_gl, o_gv, o_ge = pad, 2 * pad + B, 3 * pad + 2 * B
        o_out = 4 * pad + 3 * B
        o_mom = o_out + 6 + pad
        _lib.check(pl.lib.usv_ppo_loss(B, *(t[k].data_ptr() for k in ("logp", "old_logp", "adv", "values")), None,
                                       t["returns"].data_ptr(), t["entropy"].data_ptr(), normalize, R.CLIP, 0.0, R.ENT_COEF,
                                       R.VF_COEF, at(o_mom), at(o_out), at(o_gl), at(o_gv), None,
                                       pl._grown(B).data_ptr(), _lib.stream_ptr(dev())), pl.lib)
        b = host(buf)
        written = np.zeros(len(b), bool)
        written[o_gl:o_gl + B] = written[o_gv:o_gv + B] = written[o_out:o_out + 6] = True
        if normalize:
            written[o_mom:o_mom + 2] = True
        assert (b[~written] == mark).all() and (b[written] != mark).all()
        assert (b[o_ge:o_ge + B] == mark).all()             # a gradient that was not asked for is not written
        form = dict(normalize=bool(normalize), clip_vf=None, entropy=True)
        want = run_loss(pl, x, form)
        assert S.same(b[o_gl:o_gl + B], want["g_logp"]) and S.same(b[o_out:o_out + 6], [want[k] for k in R.NAMES])


def test_repeated_calls_a_second_stream_and_a_shared_scratch_give_the_same_bits(pl):
    from gym_usv_amd import DevicePPOLoss
    big, small, form = R.inputs(65 * R.P + 1, seed=6), R.inputs(257, seed=6), R.FORMS[1]

    def bits(obj, x):
        got = run_loss(obj, x, form)
        ev = host(obj.explained_variance(to_dev(x["values"]), to_dev(x["returns"])))
        return np.concatenate([S.bits(np.ravel(got[k])) for k in sorted(got)] + [S.bits(ev)])

    first_big, first_small = bits(pl, big), bits(DevicePPOLoss(dev()), small)
    assert (bits(pl, big) == first_big).all()
    assert (bits(pl, small) == first_small).all()            # 257 rows after 66 561 on the same scratch
    assert (bits(pl, big) == first_big).all()
    torch.cuda.synchronize()
    other, side = DevicePPOLoss(dev()), torch.cuda.Stream(dev())
    with torch.cuda.stream(side):
        a, b = bits(other, big), bits(other, small)
    side.synchronize()
    assert (a == first_big).all() and (b == first_small).all()


def test_explained_variance(pl):
    worst = 0.0
    for B in (257, 65 * R.P + 1):
        x = R.inputs(B, seed=3)
        got = host(pl.explained_variance(to_dev(x["values"]), to_dev(x["returns"])))
        assert S.same(got, [R.explained32(x["values"], x["returns"])]), B
        worst = max(worst, abs(float(got[0]) - R.explained64(x["values"], x["returns"])) / R.explained_scale(x["values"], x["returns"]))
    print(f"explained variance error: {worst:.3e}")
    assert worst <= BOUND["explained_variance"] and worst < S.CEILING
    v = to_dev(R.inputs(512)["values"]).reshape(2, 256)       # a rollout's [T, N]
    ev = pl.explained_variance(v, torch.full_like(v, 1.5))
    assert ev.shape == () and math.isnan(ev.item())
    with pytest.raises(ValueError):
        pl.explained_variance(v, v.reshape(-1))


def test_autograd_wiring_through_the_head_and_a_value_layer(pl):
    """(3 * loss).backward() through DeviceSDE.evaluate(...).log_prob and a linear value layer against torch autograd
    of the torch lines on the same tensors.  Both are float32 evaluations of one definition, each within the ceiling
    of it: the difference of every gradient stays under the ceiling times the sum of the magnitudes of its terms, with
    the rows' upstream magnitudes 3 x scales()' g_logp and g_values."""
    from gym_usv_amd import DeviceSDE
    n, L, A, F = 257, 64, 2, 16
    mean, lat, std, act, old, adv, _, _ = E.inputs(n, L, A)
    rng = np.random.default_rng(5)
    feat, w = rng.standard_normal((n, F)).astype(np.float32), (0.3 * rng.standard_normal(F)).astype(np.float32)
    ret = rng.standard_normal(n).astype(np.float32)
    head = DeviceSDE(n, L, A, dev(), 1, E.Q.LOW[:A], E.Q.HIGH[:A])
    dv = lambda a, g=False: torch.from_numpy(np.ascontiguousarray(a)).to(dev()).requires_grad_(g)  # noqa: E731
    lat_t, act_t, old_t, adv_t, ret_t, feat_t = (dv(a) for a in (lat, act, old, adv, ret, feat))

    def grads(kernel):
        mean_t, std_t = dv(mean, True), dv(std, True)
        layer = torch.nn.Linear(F, 1).to(dev())
        with torch.no_grad():
            layer.weight.copy_(dv(w).reshape(1, F))
            layer.bias.fill_(0.1)
        values = layer(feat_t).squeeze(-1)
        if kernel:
            logp = head.evaluate(mean_t, lat_t, std_t, act_t).log_prob
            out = pl.loss(logp, old_t, adv_t, values, ret_t, clip_range=R.CLIP, vf_coef=R.VF_COEF, ent_coef=R.ENT_COEF)
            loss, extra = out.loss, out.policy_loss
        else:
            s2 = (lat_t * lat_t) @ (std_t ** 2) + E.EPS
            logp = torch.distributions.Normal(mean_t, torch.sqrt(s2), validate_args=False).log_prob(act_t).sum(-1)
            a_ = (adv_t - adv_t.mean()) / (adv_t.std() + 1e-8)
            ratio = (logp - old_t).exp()
            pg = -torch.min(ratio * a_, ratio.clamp(1 - R.CLIP, 1 + R.CLIP) * a_).mean()
            loss = pg + R.ENT_COEF * -(-logp).mean() + R.VF_COEF * ((ret_t - values) ** 2).mean()
            extra = pg.detach()
        (3 * loss + 0 * extra).backward()                     # a statistic in the sum raises nothing and adds nothing
        return {"mean": mean_t.grad, "std": std_t.grad, "weight": layer.weight.grad.reshape(-1), "bias": layer.bias.grad,
                "logp": host(logp), "values": host(values)}

    ours, theirs = grads(True), grads(False)
    x = {"logp": theirs["logp"], "old_logp": old, "adv": adv, "values": theirs["values"], "old_values": theirs["values"],
         "returns": ret, "entropy": ret}
    sc = R.scales(x, R.FULL_FORM)
    var = (lat.astype(np.float64) ** 2) @ (std.astype(np.float64) ** 2)
    s_mean, _, s_std = E.grad_scales(mean, lat, std, act, None, 3.0 * sc["g_logp"], None, var, None)
    s_rows = 3.0 * sc["g_values"]
    scale = {"mean": s_mean, "std": s_std, "weight": s_rows @ np.abs(feat.astype(np.float64)), "bias": np.array([s_rows.sum()])}
    worst = {}
    for k, s in scale.items():
        diff = np.abs(host(ours[k]).astype(np.float64) - host(theirs[k]).astype(np.float64)).reshape(s.shape)
        assert np.abs(host(theirs[k])).max() > 0
        worst[k] = float(np.max(E.ratio_of(diff, s)))
    print("wiring differences:", {k: f"{v:.3e}" for k, v in worst.items()})
    assert all(v < S.CEILING for v in worst.values()), worst


def test_loss_alone_and_with_a_statistic_give_the_same_gradients(pl):
    x, form = R.inputs(257, seed=8), R.FORMS[0]
    want = run_loss(pl, x, form)
    lp, v = to_dev(x["logp"], True), to_dev(x["values"], True)
    out = pl.loss(lp, to_dev(x["old_logp"]), to_dev(x["adv"]), v, to_dev(x["returns"]), clip_range=R.CLIP,
                  vf_coef=R.VF_COEF, ent_coef=R.ENT_COEF)
    (out.loss + 0 * out.policy_loss + 2 * out.approx_kl + out.clip_fraction).backward()
    assert S.same(host(lp.grad), want["g_logp"]) and S.same(host(v.grad), want["g_values"])
    with pytest.raises(ValueError):
        pl.loss(lp, to_dev(x["old_logp"], True), to_dev(x["adv"]), v, to_dev(x["returns"]))
    with pytest.raises(ValueError):
        pl.loss(lp, to_dev(x["old_logp"]), to_dev(x["adv"]), v, to_dev(x["returns"]), clip_range_vf=0.2)


TRAINER = dict(envs=256, updates=2, n_steps=8, batch_size=512, log=print)
MODES = {"fused": dict(fused=True, frames=True, sde_kernel=True, eval_kernel=True),
         "entropy": dict(fused=False, use_sde=False),
         "clip_range_vf": dict(fused=True, frames=True, sde_kernel=True, eval_kernel=True, clip_range_vf=0.2)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_ppo_example_loss_kernel(mode):
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    from ppo_torch import train
    hist = train("usv-simple", loss_kernel=True, check_loss=True, **TRAINER, **MODES[mode])
    assert len(hist) == 2 and hist[-1]["losses_checked"] == 2 * 10 * 4
    for h in hist:
        for key in ("policy_loss", "value_loss", "entropy", "approx_kl"):
            assert math.isfinite(h[key]), h
        assert 0.0 <= h["clip_fraction"] <= 1.0, h
        assert math.isfinite(h["explained_variance"]) or math.isnan(h["explained_variance"]), h
    d = hist[-1]["loss_diff"]
    print("example loss differences:", mode, d)
    assert set(d) == {"policy", "value", "entropy"} and all(v < 1e-5 for v in d.values()), d


def test_ppo_example_without_the_flag_keeps_its_record():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    from ppo_torch import train
    hist = train("usv-simple", **dict(TRAINER, updates=1), fused=True, frames=True, sde_kernel=True, eval_kernel=True)
    assert set(hist[0]) == {"update", "policy_loss", "value_loss", "entropy", "std_mean", "episodes", "mean_abs_ye",
                            "env_steps", "wall_s"} | ({"ep_rew_mean", "ep_len_mean"} if hist[0]["episodes"] else set())
    with pytest.raises(ValueError):
        train("usv-simple", **dict(TRAINER, updates=1), check_loss=True)
