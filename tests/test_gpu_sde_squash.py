"""The squashed gSDE head on the GPU (gym_usv_amd.DeviceSDE.squashed: usv_sde_squash_forward / _backward)
against its definition in float64 (tests/sde_squash_ref.py: forward in NumPy, backward by torch-CPU autograd).

Exact properties are compared as integers: no tolerance.  Eight errors (sde_squash_ref.errors; each divided by
the sum of the absolute magnitudes of its terms) are measured over sde_squash_ref.SHAPES, printed, and bounded at
4x the maximum measured on the MI355X, MEASURED below; independently each must stay below the ceiling of 1e-5,
a condition and not a measurement.  The gradient errors are taken at the device's own u, var and normals; the
normals are bounded against the reference's on their own ("z"), as tests/test_gpu_sde.py does: see
sde_squash_ref.py's docstring."""
import os
import sys

import numpy as np
import pytest
import torch

import sde_squash_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# maxima over Q.SHAPES on the MI355X (rounded up)
MEASURED = {"z": 2.23e-7, "u": 1.33e-7, "a": 6.66e-8, "var": 1.68e-7, "logp": 1.40e-7, "g_mean": 1.54e-7,
            "g_lat": 2.17e-7, "g_std": 9.97e-8}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
SENTINEL = -7.0e33
PAD = 8                                                 # floats past L in the strided latent and g_lat rows


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


def make_head(n, L, A, gid0=Q.GID0, seed=Q.SEED, epoch=Q.EPOCH):
    import gym_usv_amd
    h = gym_usv_amd.DeviceSDE(n, L, A, dev(), seed, Q.LOW[:A], Q.HIGH[:A], env_id_offset=gid0)
    h.epoch = epoch
    return h


def forward(head, mean, lat, std):
    """usv_sde_squash_forward into guarded outputs, sentinel rows checked: (act, env, logp, gauss, var)."""
    n, A = head.n, head.act_dim
    outs = [guarded(n, A), guarded(n, A), guarded(n), guarded(n, A), guarded(n, A)]
    head._squash_forward(mean, lat, std, tuple(v for v, _ in outs))
    torch.cuda.current_stream().synchronize()
    assert all(untouched(w) for _, w in outs)
    return tuple(v for v, _ in outs)


def backward(head, mean, lat, std, gauss, var, ga, gl, epoch=None):
    """usv_sde_squash_backward into guarded outputs and a strided g_lat whose tails are checked untouched:
    (g_mean, g_lat, g_std)."""
    n, L, A = head.n, head.latent_dim, head.act_dim
    (gm, gm_w), (gs, gs_w) = guarded(n, A), guarded(L, A)
    glat_whole = torch.full((n + 2, L + PAD), SENTINEL, device=dev())
    glat = glat_whole[1:-1, :L]
    head._squash_backward(head.epoch if epoch is None else epoch, mean, lat, std, gauss, var, ga, gl, gm, glat, gs)
    torch.cuda.current_stream().synchronize()
    assert untouched(gm_w) and untouched(gs_w) and untouched(glat_whole)
    assert bool((glat_whole[:, L:] == SENTINEL).all())
    return gm, glat, gs


_CASES = {}


def case(n, L, A):
    """One forward and backward of shape (n, L, A) on Q.inputs, shared by the tests: device tensors and outputs."""
    if (n, L, A) not in _CASES:
        inp = Q.inputs(n, L, A)
        mean, lat, std, ga, gl = (to_dev(x) for x in inp)
        lat_v, _ = strided(lat, float("nan"))               # NaN past L: a read there would show
        head = make_head(n, L, A)
        act, env, logp, gauss, var = forward(head, mean, lat_v, std)
        gm, glat, gs = backward(head, mean, lat_v, std, gauss.contiguous(), var.contiguous(), ga, gl)
        _CASES[(n, L, A)] = dict(inp=inp, dev=(mean, lat_v, std, ga, gl), head=head, act=act, env=env, logp=logp,
                                 gauss=gauss, var=var, g_mean=gm, g_lat=glat, g_std=gs)
    return _CASES[(n, L, A)]


@pytest.mark.parametrize("n,L,A", Q.SHAPES, ids=lambda v: str(v))
def test_against_the_float64_reference(n, L, A):
    c = case(n, L, A)
    head, std = c["head"], c["dev"][2]
    z = head.weights(torch.ones_like(std))                  # the device's own normals: std = 1
    got = {k: c[k].cpu().numpy() for k in ("act", "env", "logp", "gauss", "var", "g_mean", "g_lat", "g_std")}
    got["z"] = z.cpu().numpy()
    assert all(np.isfinite(v).all() for v in got.values())  # the zero latent row and the saturated row included
    if n >= 2:
        assert (got["var"][0] == 0).all() and same(got["gauss"][0], c["inp"][0][0]) and (got["act"][-1] == 1.0).all()
    err = Q.errors(got, c["inp"])
    print(f"sde squash errors n {n} L {L} A {A}: " + " ".join(f"{k} {v:.3e} (bound {BOUND[k]:.1e})" for k, v in err.items()))
    for k, v in err.items():
        assert v < Q.CEILING, (k, v)
        assert v <= BOUND[k], (k, v, BOUND[k])


@pytest.mark.parametrize("n,L,A", Q.SHAPES[:5], ids=lambda v: str(v))
def test_exact_properties(n, L, A):
    c = case(n, L, A)
    head = c["head"]
    mean, lat, std, ga, gl = c["dev"]
    lo, hi = torch.tensor(Q.LOW[:A], device=dev()), torch.tensor(Q.HIGH[:A], device=dev())
    # env_actions is torch's unscale_action of actions, in the example's order
    assert same(c["env"], lo + (c["act"] + 1) * 0.5 * (hi - lo))
    assert bool((c["act"].abs() <= 1).all())
    # gaussian_actions is sample's unclipped action
    a, _, _ = head.sample(mean, lat, std)
    assert same(c["gauss"], a)
    # a repeated backward gives the same bits; NULL gradients are zeros
    gauss, var = c["gauss"].contiguous(), c["var"].contiguous()
    again = backward(head, mean, lat, std, gauss, var, ga, gl)
    assert all(same(x, c[k]) for x, k in zip(again, ("g_mean", "g_lat", "g_std")))
    for null_act, null_logp in ((True, False), (False, True), (True, True)):
        z_a, z_l = torch.zeros_like(ga), torch.zeros_like(gl)
        want = backward(head, mean, lat, std, gauss, var, z_a if null_act else ga, z_l if null_logp else gl)
        have = backward(head, mean, lat, std, gauss, var, None if null_act else ga, None if null_logp else gl)
        assert all(same(x, y) for x, y in zip(want, have)), (null_act, null_logp)
    # the forward without gauss / var (a call that is not differentiated) gives the same three outputs
    outs = [guarded(n, A), guarded(n, A), guarded(n)]
    head._squash_forward(mean, lat, std, tuple(v for v, _ in outs) + (None, None))
    torch.cuda.current_stream().synchronize()
    assert all(untouched(w) for _, w in outs)
    assert all(same(v, c[k]) for (v, _), k in zip(outs, ("act", "env", "logp")))
    # the backward's epoch is its argument: another epoch is another matrix
    other = backward(head, mean, lat, std, gauss, var, ga, gl, epoch=Q.EPOCH + 1)
    assert not same(other[1], c["g_lat"])


def test_shard_equals_rows_of_the_whole():
    n, L, A = 5, 260, 2
    c = case(n, L, A)
    mean, lat, std, ga, gl = c["dev"]
    part = make_head(3, L, A, gid0=Q.GID0 + 2)
    rows = slice(2, 5)
    m, x, g, l = mean[rows].contiguous(), lat[rows], ga[rows].contiguous(), gl[rows].contiguous()
    act, env, logp, gauss, var = forward(part, m, x, std)
    for got, k in ((act, "act"), (env, "env"), (logp, "logp"), (gauss, "gauss"), (var, "var")):
        assert same(got, c[k][rows]), k
    gm, glat, _ = backward(part, m, x, std, gauss.contiguous(), var.contiguous(), g, l)
    assert same(gm, c["g_mean"][rows]) and same(glat, c["g_lat"][rows])


@pytest.mark.parametrize("n,L,A", ((257, 300, 2), (1027, 8, 2)), ids=lambda v: str(v))
def test_result_does_not_depend_on_the_stream(n, L, A):
    """Forward and backward on a second stream give the first stream's bits: g_std's sum over rows (one row per
    partial at 257 rows, two at 1027) has a fixed order."""
    c = case(n, L, A)
    head = c["head"]
    mean, lat, std, ga, gl = c["dev"]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev())
    with torch.cuda.stream(s):
        f = forward(head, mean, lat, std)
        b = backward(head, mean, lat, std, f[3].contiguous(), f[4].contiguous(), ga, gl)
    s.synchronize()
    assert all(same(x, c[k]) for x, k in zip(f, ("act", "env", "logp", "gauss", "var")))
    assert all(same(x, c[k]) for x, k in zip(b, ("g_mean", "g_lat", "g_std")))


def test_autograd_wiring():
    """loss = (c * actions).sum() + (w * log_prob).sum() with std = log_std.exp(): the gradients of mean and latent
    are the backward call's bits, log_std's is g_std * std, and all three are compared with the float64 reference
    under the same bounds.  log_std's gradient takes one more float32 multiplication in torch: half an ulp,
    2^-24, of a value below its scale is added to its bound.  A second forward before backward(), a
    reset_noise() before backward() and non-contiguous upstream gradients change nothing; under no_grad the
    persistent buffers come back."""
    n, L, A = 5, 260, 2
    c = case(n, L, A)
    mean, lat, std0, ga, gl = c["dev"]
    lat = lat.contiguous()
    ls = std0.log().requires_grad_(True)                    # the leaf; std = exp(log_std) is what the head sees
    std = ls.exp()
    low = make_head(n, L, A)
    f = forward(low, mean, lat, std.detach())
    want = backward(low, mean, lat, std.detach(), f[3].contiguous(), f[4].contiguous(), ga, gl)
    head = make_head(n, L, A)
    m, x = mean.clone().requires_grad_(True), lat.clone().requires_grad_(True)
    s1 = head.squashed(m, x, std)
    assert type(s1).__name__ == "SquashedSample" and s1._fields == ("actions", "env_actions", "log_prob", "gaussian_actions")
    assert s1.actions.requires_grad and s1.log_prob.requires_grad
    assert not s1.env_actions.requires_grad and not s1.gaussian_actions.requires_grad
    for got, w in zip(s1, (f[0], f[1], f[2], f[3])):
        assert same(got, w)
    # a second forward on other inputs, no_grad calls and a new epoch, all before the first backward
    s2 = head.squashed(m.detach() * 0.5, (x.detach() + 1.0).requires_grad_(True), std.detach() * 2.0)
    assert s2.actions.data_ptr() != s1.actions.data_ptr() and not same(s2.actions, s1.actions)
    with torch.no_grad():
        p1 = head.squashed(m, x, std)
        ptrs = [t.data_ptr() for t in p1]
        assert same(p1.log_prob, f[2]) and not p1.actions.requires_grad
        p2 = head.squashed(m.detach() * 0.5, x.detach(), std.detach())
    assert ptrs == [t.data_ptr() for t in p2] and s1.actions.data_ptr() not in ptrs
    head.reset_noise()
    # the upstream gradient of actions arrives transposed: not contiguous
    loss = (ga.t().contiguous() * s1.actions.t()).sum() + (gl * s1.log_prob).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert same(m.grad, want[0]) and same(x.grad, want[1])
    assert same(ls.grad, want[2] * std.detach())
    # against the reference, at the device's own u, var and normals
    mean_np, lat_np, _, ga_np, gl_np = c["inp"]
    z = low.weights(torch.ones_like(std0)).cpu().numpy().astype(np.float64)
    u, var = f[3].cpu().numpy().astype(np.float64), f[4].cpu().numpy().astype(np.float64)
    std64 = std.detach().cpu().numpy().astype(np.float64)
    gm, glat, gstd = Q.grads(z, mean_np, lat_np, std64, u, var, ga_np, gl_np)
    Sm, s_lat, s_std = Q.grad_scales(z, mean_np, lat_np, std64, u, var, ga_np, gl_np)
    err = {"g_mean": Q.ratio(np.abs(m.grad.cpu().numpy() - gm), Sm).max(),
           "g_lat": Q.ratio(np.abs(x.grad.cpu().numpy() - glat), s_lat).max(),
           "g_log_std": Q.ratio(np.abs(ls.grad.cpu().numpy() - gstd * std64), s_std * std64).max()}
    print("autograd: " + " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert err["g_mean"] <= BOUND["g_mean"] and err["g_lat"] <= BOUND["g_lat"]
    assert err["g_log_std"] <= BOUND["g_std"] + 2.0 ** -24
    # only the inputs that need one get a gradient
    m2, x2 = mean.clone().requires_grad_(True), lat.clone().requires_grad_(True)
    s3 = head.squashed(m2, x2.detach(), std.detach())
    s3.log_prob.sum().backward()
    assert m2.grad is not None and x2.grad is None


def test_trainer_runs_with_the_sde_kernel():
    """examples/sac_torch.py with sde_kernel=True: 32 gradient steps with finite losses, a non-zero gradient in
    actor.log_std, and log_std moved from its initial -3."""
    sys.path[:0] = [os.path.join(ROOT, "examples")]
    from sac_torch import train
    hist = train("usv-simple", envs=256, steps=40, seed=0, log=lambda s: None, batch_size=256, learning_starts=8,
                 buffer_size=2560, device_replay=True, sde_kernel=True)
    assert sum(r["gradient_steps"] for r in hist) == 32
    for r in hist:
        assert all(np.isfinite(r[k]) for k in ("actor_loss", "critic_loss", "ent_coef", "ent_coef_loss")), r
        assert np.isfinite(r["log_std_mean"]) and r["log_std_grad_abs_max"] > 0, r
    assert hist[-1]["log_std_move_abs_max"] > 0 and abs(hist[-1]["log_std_mean"] + 3.0) < 0.1
