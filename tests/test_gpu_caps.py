"""The CAPS regulariser on the GPU (gym_usv_amd.DeviceCAPS: usv_caps_perturb / usv_caps_loss, the backward through
usv_sac_loss_backward).

Loss, squash=False: bitwise against the NumPy float32 restatement (tests/caps_ref.py), the scaled gradients for
upstream 1, another scalar and an unused loss, under no_grad, repeated and on a second stream, with rows at zero
distance and a NaN row.

Loss, squash=True: rows at zero distance give exactly zero; everything else against torch-CPU float64 autograd of
the definition, the loss's error over the loss and each gradient's over (lambda_t + lambda_s) / B, on inputs whose
rows keep both distances at least 0.05 in action space (caps_ref.floored_inputs says why).  The errors are printed
and bounded at 4x the maximum measured on the MI355X (MEASURED below); independently each must stay below the
ceiling of 1e-4, a condition and not a measurement.

Perturbation: |out - (obs + eps z64)| / (|obs| + eps r) with z64 and the pair's Box-Muller radius r from sde_ref, printed
and bounded the same way under the ceiling of 1e-5 that tests/test_gpu_sde.py has for z; a guard region, repeated
calls, a second stream, epochs, seeds, rows independent of B, eps = 0, out aliasing obs, and the sample moments."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import caps_ref as C
import sac_loss_ref as S
import sde_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# maxima over the cases below on the MI355X (rounded up)
MEASURED = {"loss": 1.69e-7, "temporal": 1.51e-7, "spatial": 2.23e-7, "g_mean": 6.78e-7, "g_next": 4.79e-7,
            "g_near": 3.73e-7, "near": 1.70e-7}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
NEAR_CEILING = 1e-5
LT, LS, EPS = 10.0, 5.0, 0.1
ROWS = (1, 63, 1024, 1025, 2049)
ACTS = (1, 2, 3)
UPSTREAMS = (1.0, -0.37, None)
SHAPES = ((3, 715), (257, 5), (64, 1), (2, 8))            # rows that are not 16-B aligned, a partial last block,
SENTINEL = -7.0e33                                        # W < 4, aligned rows


def dev():
    return torch.device("cuda", 0)


def to_dev(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev()).requires_grad_(grad)


def host(t):
    return t.detach().cpu().numpy()


def make(squash=False, lambda_t=LT, lambda_s=LS, eps_s=EPS, seed=11):
    from gym_usv_amd import DeviceCAPS
    return DeviceCAPS(dev(), seed, lambda_t, lambda_s, eps_s, squash=squash)


def run_loss(caps, x, up=1.0, grad=True):
    """The device's three outputs and, with grad, the gradients of up * loss (None: of other work, the loss
    unused)."""
    m, mn, mr = (to_dev(v, grad) for v in x)
    if not grad:
        with torch.no_grad():
            out = caps.loss(m, mn, mr)
        assert not out.loss.requires_grad
    else:
        out = caps.loss(m, mn, mr)
        assert out.loss.requires_grad and not out.temporal.requires_grad and not out.spatial.requires_grad
    assert out.loss.shape == out.temporal.shape == out.spatial.shape == ()
    got = {k: host(getattr(out, k)) for k in ("loss", "temporal", "spatial")}
    if grad:
        if up is None:                                    # the loss takes no part in what is differentiated
            (m.sum() * 0.0).backward()
            assert mn.grad is None and mr.grad is None and bool((m.grad == 0).all())
            got.update(g_mean=None, g_next=None, g_near=None)
        else:
            (out.loss * up).backward()
            got.update(g_mean=host(m.grad), g_next=host(mn.grad), g_near=host(mr.grad))
    return got


def test_loss_equals_the_restatement_bitwise():
    caps = make()
    for B in ROWS:
        for A in ACTS:
            x = C.inputs(B, A, seed=1)
            want = C.loss(*x, LT, LS, False)
            for up in UPSTREAMS:
                got = run_loss(caps, x, up)
                for k in ("loss", "temporal", "spatial"):
                    assert S.same(got[k], want[k]), (B, A, k)
                for k in ("g_mean", "g_next", "g_near"):
                    if up is None:
                        assert got[k] is None
                    else:
                        assert S.same(got[k], C.scaled(want[k], up)), (B, A, up, k)
                if up == 1.0:                             # mean_next == mean on every fifth row, mean_near on row 2
                    assert (got["g_next"][::5] == 0).all() and (got["g_mean"][::5] == -got["g_near"][::5]).all()
                    assert B <= 2 or (got["g_near"][2] == 0).all()
            got = run_loss(caps, x, grad=False)
            for k in ("loss", "temporal", "spatial"):
                assert S.same(got[k], want[k]), (B, A, k)
    # only one input requires grad: the others' gradients stay None
    x = C.inputs(63, 2, seed=1)
    m, mn, mr = to_dev(x[0]), to_dev(x[1], True), to_dev(x[2])
    caps.loss(m, mn, mr).loss.backward()
    assert m.grad is None and mr.grad is None and S.same(host(mn.grad), C.loss(*x, LT, LS, False)["g_next"])
    # lambda_t = 0 and a NaN row
    x = C.inputs(1025, 2, seed=1)
    got, want = run_loss(make(lambda_t=0.0), x), C.loss(*x, 0.0, LS, False)
    assert all(S.same(got[k], want[k]) for k in want) and (got["g_next"] == 0).all()
    x = C.inputs(S.P + 1, 3, nan_row=True)
    got, want = run_loss(caps, x), C.loss(*x, LT, LS, False)
    assert all(S.same(got[k], want[k]) for k in want)
    assert math.isnan(got["loss"]) and math.isnan(got["spatial"]) and not math.isnan(got["temporal"])
    assert np.isnan(got["g_near"]).sum() == 3 and not np.isnan(got["g_next"]).any()


def test_repeated_calls_and_a_second_stream_give_the_same_bits():
    """The multi-block hand-off: whichever block ends last, and on whichever stream, the bits are the restatement's."""
    x = C.inputs(2049, 2, seed=3)
    want = C.loss(*x, LT, LS, False)

    def check(obj):
        got = run_loss(obj, x)
        assert all(S.same(got[k], want[k]) for k in want)

    caps = make()
    for _ in range(4):
        check(caps)
    torch.cuda.synchronize()
    other, side = make(), torch.cuda.Stream(dev())
    with torch.cuda.stream(side):
        for _ in range(3):
            check(other)
    side.synchronize()
    small = make()                                        # a small batch first, then a larger one: the scratch regrows
    run_loss(small, C.inputs(5, 2))
    check(small)


def test_squashed_loss_against_the_float64_definition():
    caps = make(squash=True)
    worst = {}
    for B in ROWS:
        for A in ACTS:
            x = C.floored_inputs(B, A, seed=2)
            for k, v in C.errors(run_loss(caps, x), C.torch_loss(*x, LT, LS, True), LT, LS).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("caps squash errors:", {k: f"{v:.3e}" for k, v in sorted(worst.items())})
    assert set(worst) == set(BOUND) - {"near"}
    for k, v in worst.items():
        assert v < C.CEILING, (k, v)
        assert v <= BOUND[k], (k, v, BOUND[k])
    # rows whose mean_next is mean bit for bit: exactly zero, whatever tanh rounds to
    x = C.inputs(1025, 2, seed=4)
    got = run_loss(caps, x)
    assert (x[1][::5] == x[0][::5]).all() and (got["g_next"][::5] == 0).all() and (got["g_near"][2] == 0).all()
    got = run_loss(caps, (x[0], x[0].copy(), x[0].copy()))
    assert all((got[k] == 0).all() for k in got), got


def guarded(B, W, offset=0):
    """A [B, W] view `offset` floats into a sentinel-filled buffer with at least W floats on either side."""
    whole = torch.full((B * W + 2 * W + 8,), SENTINEL, device=dev())
    at = W + offset
    return whole[at:at + B * W].view(B, W), whole, at


def untouched(whole, at, n):
    return bool((whole[:at] == SENTINEL).all()) and bool((whole[at + n:] == SENTINEL).all())


def near_error(out, obs, z, r, eps):
    ref = obs.astype(np.float64) + eps * z
    return float((np.abs(out - ref) / (np.abs(obs) + eps * r)).max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_near_against_the_float64_reference(shape):
    B, W = shape
    seed, epoch = 0x1234567890ABCDEF, 5
    caps = make(seed=seed)
    caps.epoch = epoch
    rng = np.random.default_rng(B * W)
    obs = rng.standard_normal((B, W)).astype(np.float32)
    obs_d = to_dev(obs)
    view, whole, at = guarded(B, W, offset=1 if W % 4 else 0)
    assert caps.near(obs_d, out=view) is view
    torch.cuda.synchronize()
    assert untouched(whole, at, B * W)
    out = host(view)
    z, r = C.normals(seed, epoch, B, W)
    err = near_error(out, obs, z, r, np.float64(np.float32(EPS)))
    print(f"caps near [{B}, {W}]: {err:.3e} (bound {BOUND['near']:.1e})")
    assert err < NEAR_CEILING and err <= BOUND["near"], err
    # a fresh output, again, on another stream: the same bits
    fresh = caps.near(obs_d)
    assert fresh.shape == (B, W) and not fresh.requires_grad and S.same(host(fresh), out)
    side = torch.cuda.Stream(dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        again = caps.near(obs_d)
    side.synchronize()
    assert S.same(host(again), out)
    # out aliasing obs
    alias = obs_d.clone()
    caps.near(alias, out=alias)
    assert S.same(host(alias), out)
    # rows [0, B1) do not depend on B
    B1 = max(1, B // 2)
    assert S.same(host(caps.near(obs_d[:B1].contiguous())), out[:B1])
    # another epoch, another seed: other noise; eps = 0: obs itself
    caps.reset_noise()
    assert caps.epoch == epoch + 1
    moved = host(caps.near(obs_d))
    assert (moved != out).mean() > 0.9
    z2, r2 = C.normals(seed, epoch + 1, B, W)
    assert near_error(moved, obs, z2, r2, np.float64(np.float32(EPS))) < NEAR_CEILING
    other = make(seed=seed + 1)
    other.epoch = epoch
    assert (host(other.near(obs_d)) != out).mean() > 0.9
    still = make(eps_s=0.0, seed=seed)
    assert (host(still.near(obs_d)) == obs).all()
    caps.epoch = 2 ** 32                                  # wraps
    assert caps.epoch == 0


def test_near_is_refused_for_bad_tensors():
    caps = make()
    good = torch.zeros(4, 6, device=dev())
    for bad in (good.double(), good[:, :5], torch.zeros(6, device=dev()), torch.zeros(0, 6, device=dev()), good.cpu(), 3.0):
        with pytest.raises(ValueError):
            caps.near(bad)
    for out in (torch.zeros(4, 5, device=dev()), good.double(), good.t()):
        with pytest.raises(ValueError):
            caps.near(good, out=out)
    m = torch.zeros(4, 2, device=dev())
    for a in ((m, m, m.cpu()), (m, torch.zeros(4, 3, device=dev()), m), (torch.zeros(4, 9, device=dev()),) * 3):
        with pytest.raises(ValueError):
            caps.loss(*a)


def test_near_sample_moments():
    """The mean and variance of (out - obs) / eps over [64, 715] within 4 standard errors of 0 and 1; the float64
    reference normals pass the same statistics within 3."""
    B, W, seed, epoch = 64, 715, 21, 2
    z, _ = C.normals(seed, epoch, B, W)
    zm, zv = R.stats(z)
    assert abs(zm) < 3 and abs(zv) < 3, (zm, zv)
    caps = make(seed=seed, eps_s=0.5)                     # a power of two: (out - obs) / eps is z up to out's rounding
    caps.epoch = epoch
    obs = np.random.default_rng(1).standard_normal((B, W)).astype(np.float32)
    out = host(caps.near(to_dev(obs)))
    gm, gv = R.stats((out.astype(np.float64) - obs) / 0.5)
    print(f"caps near moments: device {gm:.2f} {gv:.2f}, reference {zm:.2f} {zv:.2f}")
    assert abs(gm) < 4 and abs(gv) < 4, (gm, gv)


def sac_run(lambda_t, lambda_s, check):
    """examples/sac_torch.py's loop with 256 envs: the training records and the actor's weights at the end."""
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    import gym_usv_amd
    from sac_torch import SAC
    env = gym_usv_amd.make_vec("usv-simple", 256, seed=0, copy=False, max_episode_steps=11)
    sac = SAC(env, seed=0, device_replay=True, sde_kernel=True, loss_kernel=True, caps=True, caps_kernel=True,
              check_caps=check, batch_size=64, learning_starts=8, train_freq=8, gradient_steps=4, buffer_size=2560,
              lambda_t=lambda_t, lambda_s=lambda_s)
    hist = []
    for at in range(0, 32, 8):
        sac.collect(8, random_actions=at < 8)
        if at >= 8:
            hist.append(sac.train(4))
    weights = torch.cat([p.detach().flatten() for p in sac.actor.parameters()]).cpu()
    env.close()
    return hist, weights


def test_sac_example_caps_kernel():
    hist, weights = sac_run(LT, LS, True)
    assert len(hist) == 3 and hist[-1]["caps_checked"] == 12
    for h in hist:
        for key in ("actor_loss", "critic_loss", "ent_coef", "ent_coef_loss", "caps_temporal", "caps_spatial"):
            assert math.isfinite(h[key]), h
        assert h["caps_temporal"] > 0 and h["caps_spatial"] > 0, h
    print("example caps difference:", [h["caps_diff"] for h in hist], [(h["caps_temporal"], h["caps_spatial"]) for h in hist])
    # the kernel and torch's float32 lines are two evaluations of one definition: within the ceiling of each other
    assert hist[-1]["caps_diff"] < C.CEILING, hist[-1]
    # the regulariser reaches the actor: without its weights the same run ends elsewhere
    _, plain = sac_run(0.0, 0.0, False)
    assert torch.isfinite(weights).all() and not torch.equal(weights, plain)
    from sac_torch import train
    # --caps alone: the torch lines, without any of the kernels' flags
    hist = train("usv-simple", envs=64, steps=24, batch_size=32, learning_starts=8, train_freq=8, gradient_steps=2,
                 buffer_size=640, seed=0, log=print, device_replay=True, caps=True, max_episode_steps=11)
    assert len(hist) == 2 and all(math.isfinite(h["actor_loss"]) and h["caps_temporal"] > 0 and h["caps_spatial"] > 0
                                  for h in hist), hist
    for kw in (dict(caps=True, n_steps=3), dict(caps_kernel=True), dict(caps=True, check_caps=True)):
        with pytest.raises(ValueError):
            train("usv-simple", envs=64, steps=8, log=print, **kw)
