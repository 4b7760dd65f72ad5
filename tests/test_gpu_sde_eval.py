"""The gSDE evaluation head on the GPU (gym_usv_amd.DeviceSDE.evaluate: usv_sde_eval_forward / _backward) against
its definition in float64 (tests/sde_eval_ref.py: forward in NumPy, backward by torch-CPU autograd).

Exact properties are compared as integers: no tolerance.  Seven errors (sde_eval_ref.errors; each divided by the
sum of the absolute magnitudes of its terms) are measured over sde_eval_ref.SHAPES, printed, and bounded at 4x the
maximum measured on the MI355X, MEASURED below; independently each must stay below the ceiling of 1e-5, a condition
and not a measurement.  The gradient errors are taken at the device's own var, logp and ratio."""
import os
import sys

import numpy as np
import pytest
import torch

import sde_eval_ref as E
import sde_squash_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# maxima over E.SHAPES on the MI355X (rounded up)
MEASURED = {"var": 1.67e-7, "logp": 9.77e-8, "ratio": 5.96e-8, "sur": 6.54e-8, "g_mean": 1.89e-7, "g_lat": 2.54e-7,
            "g_std": 1.77e-7}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
SENTINEL = -7.0e33
PAD = 8                                                 # floats past L in the strided latent and g_lat rows
HEAD_N = 3                                              # the head's own n: not the evaluation's row count


def dev():
    return torch.device("cuda", 0)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(x, y):
    return bool((bits(x) == bits(y)).all())


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def strided(rows, fill):
    """[n, L] as a view of an [n, L + PAD] buffer whose tails hold `fill`: (view, whole)."""
    n, L = rows.shape
    whole = torch.full((n, L + PAD), fill, device=dev())
    whole[:, :L] = rows
    return whole[:, :L], whole


def guarded(*shape):
    """A tensor of `shape` between one sentinel row before and one after: (the view, the whole buffer)."""
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), SENTINEL, device=dev())
    return whole[1:-1], whole


def untouched(whole):
    return bool((whole[0] == SENTINEL).all()) and bool((whole[-1] == SENTINEL).all())


def make_head(L, A, n=HEAD_N, seed=Q.SEED):
    import gym_usv_amd
    return gym_usv_amd.DeviceSDE(n, L, A, dev(), seed, Q.LOW[:A], Q.HIGH[:A])


def forward(head, mean, lat, std, act, old=None, adv=None, clip=E.CLIP, with_var=True):
    """usv_sde_eval_forward into guarded outputs, sentinel rows checked: (logp, sur, ratio, var); sur and ratio are
    None without old / adv, var without with_var."""
    B, A = mean.shape
    logp, sur, ratio, var = guarded(B), guarded(B), guarded(B), guarded(B, A)
    ppo = old is not None
    head._eval_forward(mean, lat, std, act, old, adv, clip if ppo else None, logp[0], sur[0] if ppo else None,
                       ratio[0] if ppo else None, var[0] if with_var else None)
    torch.cuda.current_stream().synchronize()
    assert all(untouched(w) for _, w in (logp, sur, ratio, var))
    for (v, _), used in ((sur, ppo), (ratio, ppo), (var, with_var)):
        assert used or bool((v == SENTINEL).all())
    return logp[0], sur[0] if ppo else None, ratio[0] if ppo else None, var[0] if with_var else None


def backward(head, mean, lat, std, act, var, ratio, adv, gl, gs, clip=E.CLIP, with_g_lat=True):
    """usv_sde_eval_backward into guarded outputs and a strided g_lat whose tails are checked untouched:
    (g_mean, g_lat or None, g_std)."""
    B, A = mean.shape
    L = head.latent_dim
    (gm, gm_w), (gstd, gstd_w) = guarded(B, A), guarded(L, A)
    glat_whole = torch.full((B + 2, L + PAD), SENTINEL, device=dev())
    glat = glat_whole[1:-1, :L]
    head._eval_backward(mean, lat, std, act, var, ratio, adv, clip if ratio is not None else None, gl, gs, gm,
                        glat if with_g_lat else None, gstd)
    torch.cuda.current_stream().synchronize()
    assert untouched(gm_w) and untouched(gstd_w) and untouched(glat_whole)
    assert bool((glat_whole[:, L:] == SENTINEL).all())
    if not with_g_lat:
        assert bool((glat_whole == SENTINEL).all())
    return gm, glat if with_g_lat else None, gstd


_CASES = {}


def case(n, L, A):
    """One forward and backward of shape (n, L, A) on E.inputs, shared by the tests: device tensors and outputs.
    The head has HEAD_N rows of its own: the evaluation's row count is the call's."""
    if (n, L, A) not in _CASES:
        inp = E.inputs(n, L, A)
        mean, lat, std, act, old, adv, gl, gs = (to_dev(x) for x in inp)
        lat_v, _ = strided(lat, float("nan"))               # NaN past L: a read there would show
        head = make_head(L, A)
        logp, sur, ratio, var = forward(head, mean, lat_v, std, act, old, adv)
        cont = lambda t: t.contiguous()                     # noqa: E731
        gm, glat, gstd = backward(head, mean, lat_v, std, act, cont(var), cont(ratio), adv, gl, gs)
        _CASES[(n, L, A)] = dict(inp=inp, dev=(mean, lat_v, std, act, old, adv, gl, gs), head=head, logp=logp, sur=sur,
                                 ratio=ratio, var=var, g_mean=gm, g_lat=glat, g_std=gstd)
    return _CASES[(n, L, A)]


@pytest.mark.parametrize("n,L,A", E.SHAPES, ids=lambda v: str(v))
def test_against_the_float64_reference(n, L, A):
    c = case(n, L, A)
    got = {k: c[k].cpu().numpy() for k in ("var", "logp", "ratio", "sur", "g_mean", "g_lat", "g_std")}
    assert all(np.isfinite(v).all() for v in got.values())  # the zero latent row (s2 = 1e-6) included
    mean, act, adv = c["inp"][0], c["inp"][3], c["inp"][5]
    if n >= 2:
        assert (got["var"][0] == 0).all() and (act[-1] == mean[-1]).all() and (got["g_mean"][-1] == 0).all()
    assert (got["sur"][adv == 0] == 0).all()
    err = E.errors(got, c["inp"])
    print(f"sde eval errors n {n} L {L} A {A}: " + " ".join(f"{k} {v:.3e} (bound {BOUND[k]:.1e})" for k, v in err.items()))
    for k, v in err.items():
        assert v < E.CEILING, (k, v)
        assert v <= BOUND[k], (k, v, BOUND[k])


@pytest.mark.parametrize("n,L,A", E.SHAPES[:5], ids=lambda v: str(v))
def test_exact_properties(n, L, A):
    c = case(n, L, A)
    head = c["head"]
    mean, lat, std, act, old, adv, gl, gs = c["dev"]
    var, ratio = c["var"].contiguous(), c["ratio"].contiguous()
    # the log-probability that sample returned with its action, and with it as old_log_prob: ratio 1, sur = adv
    sampler = make_head(L, A, n=n, seed=5)
    a, _, lp = sampler.sample(mean, lat, std)
    a, lp = a.clone(), lp.clone()
    f = forward(head, mean, lat, std, a, lp, adv)
    assert same(f[0], lp) and bool((f[2] == 1.0).all()) and same(f[1], adv)
    # var is the squashed forward's
    outs = tuple(torch.empty(s, device=dev()) for s in ((n, A), (n, A), (n,), (n, A), (n, A)))
    sampler._squash_forward(mean, lat, std, outs)
    assert same(c["var"], outs[4])
    # without the PPO arguments and without var: the same log-probability
    g = forward(head, mean, lat, std, act, with_var=False)
    assert same(g[0], c["logp"]) and g[1] is None and g[2] is None
    # a repeated backward gives the same bits; NULL upstream gradients are zeros
    again = backward(head, mean, lat, std, act, var, ratio, adv, gl, gs)
    assert all(same(x, c[k]) for x, k in zip(again, ("g_mean", "g_lat", "g_std")))
    for null_l, null_s in ((True, False), (False, True), (True, True)):
        z = torch.zeros_like(gl)
        want = backward(head, mean, lat, std, act, var, ratio, adv, z if null_l else gl, z if null_s else gs)
        have = backward(head, mean, lat, std, act, var, ratio, adv, None if null_l else gl, None if null_s else gs)
        assert all(same(x, y) for x, y in zip(want, have)), (null_l, null_s)
    # without g_lat nothing of [n, L] is written and the rest keeps its bits
    no_lat = backward(head, mean, lat, std, act, var, ratio, adv, gl, gs, with_g_lat=False)
    assert no_lat[1] is None and same(no_lat[0], c["g_mean"]) and same(no_lat[2], c["g_std"])
    # without the surrogate the row's gradient is g_logp's alone
    plain = backward(head, mean, lat, std, act, var, None, None, gl, None)
    zero_s = backward(head, mean, lat, std, act, var, ratio, adv, gl, torch.zeros_like(gs))
    assert all(same(x, y) for x, y in zip(plain, zero_s))


def test_rows_of_a_call_equal_the_rows_alone():
    """Rows 2..4 of the 5-row call and row 700 of the 1027-row call (two rows per partial), each evaluated on its
    own (B = 3 and B = 1): every per-row output has the whole's bits, g_mean and g_lat included."""
    for (n, L, A), rows in (((5, 260, 2), slice(2, 5)), ((1027, 8, 2), slice(700, 701))):
        c = case(n, L, A)
        mean, lat, std, act, old, adv, gl, gs = c["dev"]
        m, x, a, o, d, l, s = (t[rows].contiguous() if t.dim() == 1 or t is not lat else t[rows]
                               for t in (mean, lat, act, old, adv, gl, gs))
        logp, sur, ratio, var = forward(c["head"], m, x, std, a, o, d)
        for got, k in ((logp, "logp"), (sur, "sur"), (ratio, "ratio"), (var, "var")):
            assert same(got, c[k][rows]), k
        gm, glat, _ = backward(c["head"], m, x, std, a, var.contiguous(), ratio.contiguous(), d, l, s)
        assert same(gm, c["g_mean"][rows]) and same(glat, c["g_lat"][rows])


@pytest.mark.parametrize("n,L,A", ((257, 300, 2), (1027, 8, 2)), ids=lambda v: str(v))
def test_result_does_not_depend_on_the_stream(n, L, A):
    """Forward and backward on a second stream give the first stream's bits: g_std's sum over rows (one row per
    partial at 257 rows, two at 1027) has a fixed order."""
    c = case(n, L, A)
    mean, lat, std, act, old, adv, gl, gs = c["dev"]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev())
    with torch.cuda.stream(s):
        f = forward(c["head"], mean, lat, std, act, old, adv)
        b = backward(c["head"], mean, lat, std, act, f[3].contiguous(), f[2].contiguous(), adv, gl, gs)
    s.synchronize()
    assert all(same(x, c[k]) for x, k in zip(f, ("logp", "sur", "ratio", "var")))
    assert all(same(x, c[k]) for x, k in zip(b, ("g_mean", "g_lat", "g_std")))


def torch_head(mean, lat, std, act, old, adv, clip=E.CLIP):
    """examples/ppo_torch.py's update head: (log_prob, surrogate) by torch ops."""
    var = (lat * lat) @ (std ** 2)
    logp = torch.distributions.Normal(mean, torch.sqrt(var + E.EPS), validate_args=False).log_prob(act).sum(-1)
    ratio = (logp - old).exp()
    return logp, torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv)


def test_autograd_wiring():
    """loss = -surrogate.mean() - 0.01 log_prob.mean() through std = log_std.exp() and a linear mean layer.  The
    gradients of mean and std are the backward call's bits; those of log_std and of the layer are within the
    reference's bounds of the torch head's on the same inputs (both are float32 evaluations of one expression; the
    kernel is within MEASURED of float64 and the torch head is given as much, so their difference is within
    2x MEASURED < BOUND; measured: g_mean 2.6e-7, g_std 3.6e-7, g_log_std 3.8e-7, g_weight 3.5e-7; log_std's gradient takes one more
    float32 multiplication, 2^-24, and the layer's are torch's sums of g_mean over the n rows, in an order that is
    torch's: up to (n - 1) 2^-24 of the sum of magnitudes on each side).  A detached latent
    gets no gradient and no [B, L] buffer; ratio carries none; under no_grad nothing is saved and no scratch made."""
    n, L, A = 5, 260, 2
    c = case(n, L, A)
    mean0, lat, std0, act, old, adv, gl, gs = c["dev"]
    lat = lat.contiguous()
    layer = torch.nn.Linear(L, A).to(dev())
    with torch.no_grad():
        layer.weight.mul_(0.01)
        layer.bias.copy_(mean0.mean(0))

    def leaves():
        w = layer.weight.detach().clone().requires_grad_(True)
        b = layer.bias.detach().clone().requires_grad_(True)
        ls = std0.log().requires_grad_(True)
        return w, b, ls

    w, b, ls = leaves()
    mean = torch.nn.functional.linear(lat, w, b)
    mean.retain_grad()
    std = ls.exp()
    std.retain_grad()
    a = (mean.detach() + (act - mean0)).contiguous()        # the case's deviations around this layer's mean
    o = torch_head(mean.detach(), lat, std.detach(), a, old, adv)[0] - (c["logp"] - old)   # and its log-ratios
    o = o.contiguous()
    head = make_head(L, A)
    ev = head.evaluate(mean, lat, std, a, o, adv, E.CLIP)
    assert type(ev).__name__ == "Evaluation" and ev._fields == ("log_prob", "surrogate", "ratio")
    assert ev.log_prob.requires_grad and ev.surrogate.requires_grad and not ev.ratio.requires_grad
    low = forward(head, mean.detach(), lat, std.detach(), a, o, adv)
    assert same(ev.log_prob, low[0]) and same(ev.surrogate, low[1]) and same(ev.ratio, low[2])
    # both sides of both clip bounds are present
    r = ev.ratio
    assert bool((r < 0.8).any()) and bool((r > 1.2).any()) and bool(((r > 0.8) & (r < 1.2)).any())
    up = {}
    ev.surrogate.register_hook(lambda g: up.__setitem__("sur", g.contiguous()))
    ev.log_prob.register_hook(lambda g: up.__setitem__("logp", g.contiguous()))
    (-(ev.surrogate).mean() - 0.01 * ev.log_prob.mean()).backward()
    torch.cuda.synchronize()
    g_sur, g_logp = up["sur"], up["logp"]                   # -1 / n and -0.01 / n as autograd rounded them
    assert abs(float(g_sur[0]) + 1.0 / n) < 1e-7 and abs(float(g_logp[0]) + 0.01 / n) < 1e-9
    want = backward(head, mean.detach(), lat, std.detach(), a, low[3].contiguous(), low[2].contiguous(), adv, g_logp,
                    g_sur, with_g_lat=False)
    assert same(mean.grad, want[0]) and same(std.grad, want[2])
    assert same(ls.grad, want[2] * std.detach())
    # the torch head on the same inputs
    w2, b2, ls2 = leaves()
    mean2 = torch.nn.functional.linear(lat, w2, b2)
    mean2.retain_grad()
    std2 = ls2.exp()
    std2.retain_grad()
    t_logp, t_sur = torch_head(mean2, lat, std2, a, o, adv)
    (-(t_sur).mean() - 0.01 * t_logp.mean()).backward()
    torch.cuda.synchronize()
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)     # noqa: E731
    s_mean, _, s_std = E.grad_scales(f64(mean), f64(lat), f64(std), f64(a), f64(adv), f64(g_logp), f64(g_sur),
                                     f64(low[3]), f64(low[2]))
    err = {"g_mean": E.ratio_of(np.abs(f64(mean.grad) - f64(mean2.grad)), s_mean).max(),
           "g_std": E.ratio_of(np.abs(f64(std.grad) - f64(std2.grad)), s_std).max(),
           "g_log_std": E.ratio_of(np.abs(f64(ls.grad) - f64(ls2.grad)), s_std * f64(std)).max(),
           # the layer's gradients are sums of g_mean over rows: the scale is the sum of the rows' scales
           "g_bias": E.ratio_of(np.abs(f64(b.grad) - f64(b2.grad)), s_mean.sum(0)).max(),
           "g_weight": E.ratio_of(np.abs(f64(w.grad) - f64(w2.grad)), s_mean.T @ np.abs(f64(lat))).max()}
    print("autograd against the torch head: " + " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert err["g_mean"] <= BOUND["g_mean"] and err["g_std"] <= BOUND["g_std"]
    assert err["g_log_std"] <= BOUND["g_std"] + 2.0 ** -24
    layer_bound = BOUND["g_mean"] + 2 * (n - 1) * 2.0 ** -24
    assert err["g_bias"] <= layer_bound and err["g_weight"] <= layer_bound
    # the latent: no gradient when detached, one when it requires it; only log_prob used: g_sur stays None
    x = lat.clone().requires_grad_(True)
    m3 = mean.detach().clone().requires_grad_(True)
    ev3 = head.evaluate(m3, x, std.detach(), a, o, adv, E.CLIP)
    (gl * ev3.log_prob).sum().backward()
    both = backward(head, m3.detach(), lat, std.detach(), a, low[3].contiguous(), low[2].contiguous(), adv, gl, None)
    assert same(m3.grad, both[0]) and same(x.grad, both[1])
    x4 = lat.clone().requires_grad_(True)
    head.evaluate(m3, x4.detach(), std.detach(), a, o, adv, E.CLIP).surrogate.sum().backward()
    assert x4.grad is None
    # no PPO arguments: surrogate and ratio are None; some of them: refused
    ev5 = head.evaluate(m3, lat, std.detach(), a)
    assert ev5.surrogate is None and ev5.ratio is None and same(ev5.log_prob, low[0]) and ev5.log_prob.requires_grad
    with pytest.raises(ValueError, match="come together"):
        head.evaluate(m3, lat, std.detach(), a, o, adv)
    with pytest.raises(ValueError):
        head.evaluate(m3, lat[:, :L - 4], std.detach(), a)
    # no_grad: fresh outputs, nothing saved, no scratch; B above the head's n and B = 1
    fresh = make_head(L, A)
    with torch.no_grad():
        e6 = fresh.evaluate(mean, lat, std, a, o, adv, E.CLIP)
        e7 = fresh.evaluate(mean[:1], lat[:1], std, a[:1], o[:1], adv[:1], E.CLIP)
    assert fresh._eval_scratch is None and fresh.n == HEAD_N < n
    assert not e6.log_prob.requires_grad and e6.log_prob.grad_fn is None
    assert same(e6.log_prob, low[0]) and same(e6.surrogate, low[1]) and same(e6.ratio, low[2])
    assert same(e7.log_prob, low[0][:1]) and same(e7.surrogate, low[1][:1])
    # the scratch grows with B
    m8 = mean.detach()[:2].clone().requires_grad_(True)
    fresh.evaluate(m8, lat[:2], std.detach(), a[:2]).log_prob.sum().backward()
    small = fresh._eval_scratch.numel()
    m9 = mean.detach().clone().requires_grad_(True)
    fresh.evaluate(m9, lat, std.detach(), a).log_prob.sum().backward()
    assert small == 2 * L * A and fresh._eval_scratch.numel() == n * L * A
    assert same(m9.grad[:2], m8.grad)


def test_trainer_runs_with_the_eval_kernel():
    """examples/ppo_torch.py with eval_kernel=True and check_eval=True: finite losses, log_std moved, and the two
    heads' log-probabilities within 1e-5 of each other in the reference's scale (both are float32 evaluations of
    one expression, each some 1e-7 from float64: the ceiling leaves two orders).  Without fused the flag is refused."""
    sys.path[:0] = [os.path.join(ROOT, "examples")]
    from ppo_torch import CONFIG_PPO, train
    kw = dict(envs=256, updates=2, n_steps=8, batch_size=512, log=lambda s: None, frames=True, sde_kernel=True,
              eval_kernel=True, check_eval=True)
    hist = train(fused=True, **kw)
    assert len(hist) == 2
    for r in hist:
        assert all(np.isfinite(r[k]) for k in ("policy_loss", "value_loss", "entropy", "std_mean")), r
        print("eval_logp_diff_max", r["eval_logp_diff_max"])
        assert 0 <= r["eval_logp_diff_max"] < 1e-5, r
    assert hist[-1]["std_mean"] != hist[0]["std_mean"]
    assert abs(hist[-1]["std_mean"] - float(np.exp(CONFIG_PPO["log_std_init"]))) > 0
    with pytest.raises(ValueError):
        train(fused=False, **kw)
    with pytest.raises(ValueError, match="eval_kernel"):
        train(fused=True, **dict(kw, sde_kernel=False))
