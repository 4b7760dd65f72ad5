"""The fused gSDE head on the GPU (gym_usv_amd.DeviceSDE: usv_sde_sample / usv_sde_weights) against its
definition restated in NumPy float64 (tests/sde_ref.py).

Exact properties are compared as integers: no tolerance.  Three errors are measured against the float64
reference, printed, and bounded at 4x the maximum measured on the MI355X over the cases below (three
different transcendentals contribute and the sample is small); independently each must stay below 1e-5,
which is a condition and not a measurement: above it an approximate intrinsic is used outside its range.

    z     |z_dev - z_ref| / max(1, r)      over weights(std = 1); r the pair's Box-Muller radius in float64
    a     |a - a_ref| / (|mean_k| + sum_j |lat_j| std_jk |z_jk|)
    logp  |logp - logp_ref(a_dev)| / (1 + sum_k (d_k^2 / s2_k + |ln s2_k|))     reference at the device's a

Measured maxima over CASES on the MI355X ("Fused gSDE head"): in MEASURED below."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import sde_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CEILING = 1e-5
MEASURED = {"z": 2.26e-7, "a": 4.98e-8, "logp": 1.17e-7}   # maxima over CASES, MI355X (rounded up)
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
LOW, HIGH = (0.0, -1.0), (1.0, 1.0)
SENTINEL = -7.0e33
# (n, L, A, row stride of the latent (0: L), env_id_offset, seed, epoch)
CASES = ((1, 4, 1, 0, 0, 3, 0),
         (3, 64, 2, 72, 5, 3, 7),                       # a latent row stride above L
         (64, 256, 2, 0, 0, 0, 1),                      # the distribution test's setting
         (65, 260, 1, 0, 0, 9, 2),                      # a partial second pass, a ragged last block
         (65, 260, 2, 0, 2 ** 32 - 2, 9, 0xFFFFFFFF),   # global env ids across 2^32
         (257, 512, 1, 0, 1, 4, 5))                     # two full passes, more than one block


def dev():
    return torch.device("cuda", 0)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def inputs(n, L, A, stride=0):
    """lat = relu(randn) as the ReLU body gives it, log_std around -2 +- 1, mean in the action Box +- 1."""
    rng = np.random.default_rng(1000 * n + 10 * L + A)
    lat = np.maximum(rng.standard_normal((n, L)), 0.0).astype(np.float32)
    std = np.exp(rng.uniform(-3.0, -1.0, (L, A))).astype(np.float32)
    lo, hi = np.float32(LOW[:A]), np.float32(HIGH[:A])
    mean = rng.uniform(lo - 1.0, hi + 1.0, (n, A)).astype(np.float32)
    d = dev()
    if stride:
        buf = torch.full((n, stride), float("nan"), device=d)
        buf[:, :L] = torch.from_numpy(lat).to(d)
        lat_d = buf[:, :L]
        assert lat_d.stride(0) == stride
    else:
        lat_d = torch.from_numpy(lat).to(d)
    return (mean, lat, std), (torch.from_numpy(mean).to(d), lat_d, torch.from_numpy(std).to(d))


def guarded(*shape):
    """A tensor of `shape` between one sentinel row before and one after: (the view, the whole buffer)."""
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), SENTINEL, device=dev())
    return whole[1:-1], whole


def untouched(whole):
    return bool((whole[0] == SENTINEL).all()) and bool((whole[-1] == SENTINEL).all())


def make_head(n, L, A, gid0=0, seed=3, epoch=0):
    import gym_usv_amd
    h = gym_usv_amd.DeviceSDE(n, L, A, dev(), seed, LOW[:A], HIGH[:A], env_id_offset=gid0)
    h.epoch = epoch
    return h


def run(head, mean, lat, std):
    """sample into guarded outputs, whose sentinel rows are checked untouched: (a, a_env, logp)."""
    n, A = head.n, head.act_dim
    outs = [guarded(n, A), guarded(n, A), guarded(n)]
    got = head.sample(mean, lat, std, out=tuple(v for v, _ in outs))
    torch.cuda.current_stream().synchronize()
    assert all(untouched(w) for _, w in outs)
    return got


def weights(head, std):
    """weights into a guarded output, whose sentinel rows are checked untouched."""
    view, whole = guarded(head.n, head.latent_dim, head.act_dim)
    head.weights(std, out=view)
    torch.cuda.current_stream().synchronize()
    assert untouched(whole)
    return view


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c[0]}-L{c[1]}-A{c[2]}" + ("-stride" if c[3] else "") +
                         ("-gid2p32" if c[4] > 2 ** 31 else ""))
def test_head_against_the_float64_reference(case):
    n, L, A, stride, gid0, seed, epoch = case
    (mean, lat, std), (mean_d, lat_d, std_d) = inputs(n, L, A, stride)
    head = make_head(n, L, A, gid0, seed, epoch)
    a, a_env, logp = run(head, mean_d, lat_d, std_d)
    wv = weights(head, torch.ones_like(std_d))
    a, a_env, logp, zdev = (x.cpu().numpy() for x in (a, a_env, logp, wv))
    assert np.isfinite(a).all() and np.isfinite(logp).all() and np.isfinite(zdev).all()
    z, r = R.normals(seed, gid0, epoch, n, L, A)
    err = {"z": float((np.abs(zdev - z) / np.maximum(1.0, r)).max())}
    a_ref, scale, _ = R.sample(seed, gid0, epoch, mean, lat, std)
    err["a"] = float((np.abs(a - a_ref) / scale).max())
    lp, lscale = R.logp_of(a, mean, lat, std)
    err["logp"] = float((np.abs(logp - lp) / lscale).max())
    print(f"sde errors n {n} L {L} A {A}: " + " ".join(f"{k} {v:.3e} (bound {BOUND[k]:.1e})" for k, v in err.items()))
    # the clip, exactly torch's
    lo, hi = torch.tensor(LOW[:A], device=dev()), torch.tensor(HIGH[:A], device=dev())
    at = torch.from_numpy(a).to(dev())
    assert (bits(a_env) == bits(torch.max(torch.min(at, hi), lo))).all()
    for k, v in err.items():
        assert v < CEILING, (k, v)
        assert v <= BOUND[k], (k, v, BOUND[k])


@pytest.mark.parametrize("case", CASES[:5], ids=lambda c: f"n{c[0]}-L{c[1]}-A{c[2]}")
def test_exact_properties(case):
    n, L, A, stride, gid0, seed, epoch = case
    _, (mean_d, lat_d, std_d) = inputs(n, L, A, stride)
    head = make_head(n, L, A, gid0, seed, epoch)
    a, a_env, logp = run(head, mean_d, lat_d, std_d)
    first = [bits(x) for x in (a, a_env, logp)]
    W = weights(head, std_d)
    # the same epoch twice: the same bits (fresh outputs)
    a2, e2, l2 = run(head, mean_d, lat_d, std_d)
    assert all((x == bits(y)).all() for x, y in zip(first, (a2, e2, l2)))
    assert (bits(W) == bits(weights(head, std_d))).all()
    # lat = 0: a == mean
    zero = torch.zeros_like(lat_d)
    a0, _, _ = run(head, mean_d, zero, std_d)
    assert (bits(a0) == bits(mean_d)).all()
    # one-hot latents and mean = 0: sample returns a row of weights()
    for j in sorted({0, 3, L // 2 + 1, L - 1}):
        hot = torch.zeros((n, L), device=dev())
        hot[:, j] = 1.0
        ah, _, _ = run(head, torch.zeros_like(mean_d), hot, std_d)
        assert (bits(ah) == bits(W[:, j, :])).all(), j
    # epoch + 1 (wrapping at 2^32): another matrix in every env
    head.reset_noise()
    assert head.epoch == (epoch + 1) & 0xFFFFFFFF
    W1 = weights(head, std_d)
    assert bool((W1 != W).flatten(1).any(1).all())
    head.epoch = epoch                                   # settable: back to the first matrix
    assert (bits(weights(head, std_d)) == bits(W)).all()


def test_shard_equals_rows_of_the_whole():
    L, A = 64, 2
    _, (mean_d, lat_d, std_d) = inputs(8, L, A)
    whole, part = make_head(8, L, A, 0, 21, 6), make_head(4, L, A, 4, 21, 6)
    a, e, lp = run(whole, mean_d, lat_d, std_d)
    a4, e4, lp4 = run(part, mean_d[4:].contiguous(), lat_d[4:], std_d)
    assert (bits(a[4:]) == bits(a4)).all() and (bits(e[4:]) == bits(e4)).all() and (bits(lp[4:]) == bits(lp4)).all()
    assert (bits(weights(whole, std_d)[4:]) == bits(weights(part, std_d))).all()


def test_result_does_not_depend_on_the_stream():
    n, L, A = 65, 256, 2
    _, (mean_d, lat_d, std_d) = inputs(n, L, A)
    head = make_head(n, L, A, 0, 8, 2)
    a, e, lp = run(head, mean_d, lat_d, std_d)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev())
    with torch.cuda.stream(s):
        a2, e2, lp2 = run(head, mean_d, lat_d, std_d)
        W2 = weights(head, std_d)
    s.synchronize()
    assert (bits(a) == bits(a2)).all() and (bits(e) == bits(e2)).all() and (bits(lp) == bits(lp2)).all()
    assert (bits(W2) == bits(weights(head, std_d))).all()


def test_device_normals_distribution():
    """weights(std = 1) in the reference's setting (seed 0, epoch 1, 64 envs, L = 256, A = 2: 32 768 normals)
    passes the statistics the reference itself passes within 3 (tests/test_sde_math.py), here with bound 4."""
    ones = torch.ones((256, 2), device=dev())
    head = make_head(64, 256, 2, 0, 0, 1)
    z1 = weights(head, ones).cpu().numpy().astype(np.float64)
    head.reset_noise()
    z2 = weights(head, ones).cpu().numpy().astype(np.float64)
    n = z1.size
    assert n == 32768
    zm, zv = R.stats(z1)
    c_cols, c_ep = R.corr(z1[..., 0], z1[..., 1]), R.corr(z1, z2)
    print(f"device normals: mean z {zm:.3f} var z {zv:.3f} corr cols {c_cols:.5f} epochs {c_ep:.5f}")
    assert abs(zm) < 4 and abs(zv) < 4
    assert abs(c_cols) < 4 / math.sqrt(n) and abs(c_ep) < 4 / math.sqrt(n)     # n = all 32 768 normals, in both
    try:
        from scipy import stats as S
    except ImportError:
        return
    p = S.kstest(z1.ravel(), "norm").pvalue
    print(f"device normals: KS p {p:.3f}")
    assert p > 0.01


def test_trainer_rollout_is_consistent_with_torch():
    """One --fused --sde-kernel rollout of examples/ppo_torch.py at 256 envs x 8 steps: the stored logp equals
    model.dist(obs).log_prob(act).sum(-1) recomputed by torch, within the logp bound plus torch's own float32
    error, which is measured here against the same model in float64 (the largest difference over the buffer).
    With sde_sample_freq = 4 the epoch advances by ceil(8 / 4) per rollout."""
    import copy
    sys.path[:0] = [os.path.join(ROOT, "examples")]
    import gym_usv_amd
    from ppo_torch import PPO
    env = gym_usv_amd.make_vec("usv-simple", 256, seed=0, copy=False)
    ppo = PPO(env, n_steps=8, batch_size=256, seed=0, fused=True, sde_kernel=True)
    assert ppo.head is not None and ppo.W is None
    for k in range(2):
        e0 = ppo.head.epoch
        ppo.rollout()
        assert ppo.head.epoch - e0 == math.ceil(8 / 4)
    assert ppo.W is None                                 # no exploration matrix was ever allocated
    ro, model = ppo.ro, ppo.model
    with torch.no_grad():
        obs, act = ro.obs.reshape(8 * 256, -1), ro.act.reshape(8 * 256, -1)
        dist, lat = model.dist(obs)
        lp32 = dist.log_prob(act).sum(-1)
        m64 = copy.deepcopy(model).double()
        lp64 = m64.dist(obs.double())[0].log_prob(act.double()).sum(-1)
        torch_err = float((lp32.double() - lp64).abs().max())
        _, lscale = R.logp_of(act.cpu().numpy(), dist.mean.cpu().numpy(), lat.cpu().numpy(),
                              model.log_std.exp().cpu().numpy())
        diff = (ro.logp.reshape(-1) - lp32).abs().double().cpu().numpy()
    tol = BOUND["logp"] * lscale + torch_err
    print(f"trainer: max |logp - torch| {diff.max():.3e}, torch vs float64 {torch_err:.3e}, "
          f"worst diff / tol {float((diff / tol).max()):.3f}")
    assert np.isfinite(diff).all() and (diff <= tol).all()
    env.close()
