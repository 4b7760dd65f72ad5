"""The fused SAC update on the GPU (gym_usv_amd.DeviceSACLoss / DevicePolyak: usv_sac_critic_loss / _policy_loss /
_loss_backward / usv_polyak_update).

Bitwise, against the NumPy float32 restatement (tests/sac_loss_ref.py): every output of both losses, the scaled
gradients for upstream 1, another scalar and None, Polyak (a pair of views 4 B off a 16-B boundary, a list with a
zero-element tensor included, a list of 130 pairs), repeated calls and calls on a second stream.

Against torch-CPU float64 autograd of SB3's lines: ten errors, each divided by the sum of the absolute magnitudes of
its terms, measured over sac_loss_ref.ROWS, printed, and bounded at 4x the maximum measured on the MI355X (MEASURED
below); independently each must stay below the ceiling of 1e-5, a condition and not a measurement.

Polyak against torch's own mul_ / add_(alpha=) on the device: |diff| <= 2^-23 (|t om| + |tau p|) per element.  Both
compute fl(fl(t om) + x) with x = fl(tau p) here and the exact tau p where torch's add_ fuses the multiply-add; the
two x differ by at most 2^-24 |tau p|, so the two results differ by at most that plus one rounding of a sum no
larger than |t om| + |tau p|, 2^-24 of it: the bound is their total, rounded up.  The number of elements that
differ at all is printed."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import sac_loss_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# maxima over S.ROWS on the MI355X (rounded up)
MEASURED = {"critic target": 1.30e-7, "critic loss": 6.87e-8, "critic g_q1": 1.57e-7, "critic g_q2": 1.55e-7,
            "policy actor_loss": 2.67e-8, "policy ent_coef_loss": 9.91e-8, "policy g_logp": 3.08e-8,
            "policy g_q1": 5.92e-8, "policy g_q2": 5.92e-8, "policy g_log_ent": 6.39e-8}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
UPSTREAMS = (1.0, -0.37)


def dev():
    return torch.device("cuda", 0)


def to_dev(x, grad=False, column=False):
    t = torch.from_numpy(np.ascontiguousarray(np.atleast_1d(np.asarray(x, np.float32)))).to(dev())
    if column:
        t = t.reshape(-1, 1)
    return t.requires_grad_(grad)


def host(t):
    return t.detach().cpu().numpy().reshape(-1)


@pytest.fixture(scope="module")
def sl():
    from gym_usv_amd import DeviceSACLoss
    return DeviceSACLoss(dev())


def run_critic(sl, x, form, up=1.0, column=False, grad=True):
    """The device's target, loss and the gradients of up * loss."""
    q1, q2 = to_dev(x["q1"], grad, column), to_dev(x["q2"], grad, column)
    kw = {} if form == "td3" else dict(ent_coef=to_dev(x["ent"]), logp_next=to_dev(x["logp_next"]))
    kw.update(dict(discounts=to_dev(x["disc"], column=column)) if form == "disc" else dict(gamma=x["gamma"]))
    out = sl.critic(q1, q2, to_dev(x["q1t"], column=column), to_dev(x["q2t"], column=column), to_dev(x["rew"], column=column),
                    to_dev(x["done"]), **kw)
    assert out.loss.shape == () and out.target.shape == q1.shape and not out.target.requires_grad
    got = {"target": host(out.target), "loss": host(out.loss)[0]}
    if grad:
        (out.loss * up).backward()
        got.update(g_q1=host(q1.grad), g_q2=host(q2.grad))
    else:
        assert not out.loss.requires_grad
    return got


def run_policy(sl, x, with_le=True, up=(1.0, 1.0), grad=True):
    """The device's losses and the gradients of up[0] * actor_loss + up[1] * ent_coef_loss (None: left out)."""
    logp, q1, q2 = to_dev(x["logp"], grad), to_dev(x["q1p"], grad, True), to_dev(x["q2p"], grad, True)
    le = to_dev(x["log_ent"], grad) if with_le else None
    out = sl.policy(logp, q1, q2, to_dev(x["ent"]), **(dict(log_ent_coef=le, target_entropy=x["te"]) if with_le else {}))
    got = {"actor_loss": host(out.actor_loss)[0]}
    if with_le:
        got["ent_coef_loss"] = host(out.ent_coef_loss)[0]
    else:
        assert out.ent_coef_loss is None
    if grad:
        terms = [l * u for l, u in zip((out.actor_loss, out.ent_coef_loss), up) if l is not None and u is not None]
        sum(terms[1:], terms[0]).backward()
        got.update(g_logp=logp.grad, g_q1=q1.grad, g_q2=q2.grad, g_log_ent=le.grad if with_le else None)
        got = {k: (None if v is None else host(v) if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
    return got


def test_critic_equals_the_restatement_bitwise(sl):
    for B in S.ROWS:
        for j, form in enumerate(S.CRITIC_FORMS):
            x = S.inputs(B, seed=j, ent=0.0 if (form == "gamma" and B % 2) else 0.2)
            a, kw = S.critic_case(x, form)
            want = S.critic(*a, **kw)
            for up in UPSTREAMS:
                got = run_critic(sl, x, form, up, column=B % 2 == 0)
                assert S.same(got["target"], want["target"]) and S.same(got["loss"], want["loss"]), (B, form)
                for k in ("g_q1", "g_q2"):
                    assert S.same(got[k], S.scaled(want[k], up)), (B, form, up, k)
            got = run_critic(sl, x, form, grad=False)
            assert S.same(got["target"], want["target"]) and S.same(got["loss"], want["loss"]), (B, form)


def test_policy_equals_the_restatement_bitwise(sl):
    for B in S.ROWS:
        for with_le in (True, False):
            x = S.inputs(B, seed=3 + with_le)
            want = S.policy(x["logp"], x["q1p"], x["q2p"], x["ent"], *((x["log_ent"], x["te"]) if with_le else ()))
            for up in ((1.0, 1.0), (-0.37, 2.5), (None, 1.0), (1.0, None)):
                if not with_le and up[0] is None:
                    continue
                got = run_policy(sl, x, with_le, up)
                assert S.same(got["actor_loss"], want["actor_loss"]), (B, with_le)
                for k in ("g_logp", "g_q1", "g_q2"):
                    if up[0] is None:                     # actor_loss took no part: the backward wrote zeros
                        assert got[k] is None or S.same(got[k], np.zeros(B)), (B, k)
                    else:
                        assert S.same(got[k], S.scaled(want[k], up[0])), (B, with_le, up, k)
                if with_le:
                    assert S.same(got["ent_coef_loss"], want["ent_coef_loss"]), B
                    assert S.same(got["g_log_ent"], S.scaled([want["g_log_ent"]], up[1])), (B, up)
            got = run_policy(sl, x, with_le, grad=False)
            assert S.same(got["actor_loss"], want["actor_loss"])
    x = S.inputs(S.P + 1, nan_q2_pi=True)
    got = run_policy(sl, x)
    assert math.isnan(got["actor_loss"]) and not math.isnan(got["ent_coef_loss"])


def test_an_ent_coef_that_requires_grad_is_refused(sl):
    x = S.inputs(5)
    ent = to_dev(x["ent"], grad=True)
    with pytest.raises(ValueError):
        sl.policy(to_dev(x["logp"]), to_dev(x["q1p"]), to_dev(x["q2p"]), ent)
    with pytest.raises(ValueError):
        sl.critic(*(to_dev(x[k]) for k in ("q1", "q2", "q1t", "q2t", "rew", "done")), ent_coef=ent,
                  logp_next=to_dev(x["logp_next"]), gamma=0.99)
    with pytest.raises(ValueError):
        sl.critic(*(to_dev(x[k]) for k in ("q1", "q2", "q1t", "q2t", "rew", "done")), gamma=0.99, discounts=to_dev(x["disc"]))


def test_repeated_calls_and_a_second_stream_give_the_same_bits(sl):
    """The multi-block hand-off: whichever block ends last, and on whichever stream, the bits are the restatement's."""
    from gym_usv_amd import DeviceSACLoss
    B = 2 * S.P + 1
    x = S.inputs(B, seed=5)
    a, kw = S.critic_case(x, "disc")
    want_c = S.critic(*a, **kw)
    want_p = S.policy(x["logp"], x["q1p"], x["q2p"], x["ent"], x["log_ent"], x["te"])

    def check(obj):
        got = run_critic(obj, x, "disc")
        assert S.same(got["loss"], want_c["loss"]) and S.same(got["g_q1"], want_c["g_q1"])
        got = run_policy(obj, x)
        assert S.same(got["actor_loss"], want_p["actor_loss"]) and S.same(got["ent_coef_loss"], want_p["ent_coef_loss"])
        assert S.same(got["g_log_ent"], [want_p["g_log_ent"]])

    for _ in range(4):
        check(sl)
    torch.cuda.synchronize()
    other, side = DeviceSACLoss(dev()), torch.cuda.Stream(dev())
    with torch.cuda.stream(side):
        for _ in range(3):
            check(other)
    side.synchronize()
    check(DeviceSACLoss(dev()))                           # a small batch first, then a larger one: the scratch regrows
    small = DeviceSACLoss(dev())
    run_critic(small, S.inputs(5), "gamma")
    check(small)


def test_errors_against_the_float64_definition(sl):
    worst = {}
    for B in S.ROWS:
        for j, form in enumerate(S.CRITIC_FORMS):
            x = S.inputs(B, seed=j)
            a, kw = S.critic_case(x, form)
            for k, v in S.errors(run_critic(sl, x, form), S.torch_critic(*a, **kw), S.critic_scales(*a, **kw)).items():
                worst["critic " + k] = max(worst.get("critic " + k, 0.0), v)
        x = S.inputs(B, seed=4)
        a = (x["logp"], x["q1p"], x["q2p"], x["ent"], x["log_ent"], x["te"])
        for k, v in S.errors(run_policy(sl, x), S.torch_policy(*a), S.policy_scales(*a)).items():
            worst["policy " + k] = max(worst.get("policy " + k, 0.0), v)
    print("sac loss errors:", {k: f"{v:.3e}" for k, v in sorted(worst.items())})
    assert set(worst) == set(BOUND)
    for k, v in worst.items():
        assert v <= BOUND[k] and v < S.CEILING, (k, v, BOUND[k])


def polyak_lists(rng):
    """(params, targets) with S.NUMELS elements each, a zero-element pair, and a pair of views 4 B past a 16-B
    boundary."""
    params, targets = [], []
    for n in S.NUMELS:
        params.append(to_dev(rng.standard_normal(n)))
        targets.append(to_dev(rng.standard_normal(n)))
    params.insert(2, torch.zeros(0, device=dev()))
    targets.insert(2, torch.zeros(0, device=dev()))
    n = S.C + 7
    pb, tb = to_dev(rng.standard_normal(n + 1)), to_dev(rng.standard_normal(n + 1))
    params.append(pb[1:])
    targets.append(tb[1:])
    assert params[-1].data_ptr() % 16 == 4 and targets[-1].data_ptr() % 16 == 4
    two = to_dev(rng.standard_normal((3, S.C // 2 + 1)))    # a matrix, and only its target misaligned
    tb2 = to_dev(rng.standard_normal(two.numel() + 1))
    params.append(two)
    targets.append(tb2[1:].view(two.shape))
    return params, targets, (pb, tb, tb2)


def test_polyak_equals_the_restatement_bitwise():
    from gym_usv_amd import DevicePolyak
    rng = np.random.default_rng(3)
    params, targets, bases = polyak_lists(rng)
    heads = [b[0].item() for b in bases]
    pol = DevicePolyak(params, targets)
    want = [host(t) for t in targets]
    for tau in S.TAUS[:1] * 3 + S.TAUS[1:]:
        pol.step(tau)
        want = [S.polyak(w, host(p), tau) for w, p in zip(want, params)]
        for t, w in zip(targets, want):
            assert S.same(host(t), w), (tau, t.shape)
    assert [b[0].item() for b in bases] == heads            # the element in front of each view is untouched
    assert S.same(host(targets[-2]), host(params[-2]))      # tau = 1 came last: the targets are the parameters
    # a parameter moved to new memory: the table is rebuilt
    params[0].data = params[0].data.clone() + 1.0
    before = host(targets[0])
    pol.step(0.25)
    assert S.same(host(targets[0]), S.polyak(before, host(params[0]), 0.25))
    from gym_usv_amd import UsvLibError
    for tau in (-0.1, 1.5, float("nan")):
        with pytest.raises(UsvLibError):
            pol.step(tau)
    with pytest.raises(UsvLibError):
        DevicePolyak([params[0]], [params[0]]).step(0.5)


def test_polyak_over_130_pairs_equals_the_restatement_bitwise():
    """130 pairs, 129 of them with elements (more than the 96 tensors a launch of a by-value table takes, should
    Polyak ever move to one).  1 .. 9 elements each, packed into one buffer a float apart (so most are misaligned, and a
    write past a tensor's end would show), a zero-element pair in the middle, and behind 99 others a pair of C + 1
    elements (two chunks, a one-element tail) 4 B off a 16-B boundary.  The same list as two objects of 65 pairs each
    gives the same bits."""
    from gym_usv_amd import DevicePolyak
    rng = np.random.default_rng(6)
    sizes = [1 + i % 9 for i in range(128)]
    sizes.insert(64, 0)
    sizes.insert(100, S.C + 1)
    spans, at = [], 0
    for n in sizes:
        if n > 9:
            at += (1 - at) % 4                              # float 1 of a group of four: 4 B past the boundary
        spans.append((at, at + n))
        at += n + 1
    p_flat, t_flat = to_dev(rng.standard_normal(at)), to_dev(rng.standard_normal(at))
    assert p_flat.data_ptr() % 16 == 0 and t_flat.data_ptr() % 16 == 0
    t_split = t_flat.clone()
    views = lambda flat: [flat[a:b] for a, b in spans]      # noqa: E731
    params, targets, halves = views(p_flat), views(t_flat), views(t_split)
    assert len(params) == 130 and params[100].numel() == S.C + 1 and params[64].numel() == 0
    assert params[100].data_ptr() % 16 == 4 and targets[100].data_ptr() % 16 == 4
    whole = DevicePolyak(params, targets)
    first, second = DevicePolyak(params[:65], halves[:65]), DevicePolyak(params[65:], halves[65:])
    want, src = host(t_flat), host(p_flat)
    for tau in (0.005, 0.3, 0.9):
        whole.step(tau)
        first.step(tau)
        second.step(tau)
        for a, b in spans:
            want[a:b] = S.polyak(want[a:b], src[a:b], tau)
        assert S.same(host(t_flat), want), tau              # the floats between the tensors included
        assert S.same(host(t_split), want), tau
    assert S.same(host(p_flat), src)


def test_polyak_against_torch_on_the_device():
    from gym_usv_amd import DevicePolyak
    rng = np.random.default_rng(4)
    params, targets, _ = polyak_lists(rng)
    tau = 0.005
    mine = [t.clone() for t in targets]
    pol = DevicePolyak(params, mine)
    differ = total = 0
    for _ in range(3):
        size = [(t * (1 - tau)).abs() + (tau * p).abs() for t, p in zip(mine, params)]
        theirs = [t.clone() for t in mine]
        pol.step(tau)
        for p, t in zip(params, theirs):
            t.mul_(1 - tau).add_(p, alpha=tau)
        for a, b, s in zip(mine, theirs, size):
            diff = (a - b).abs()
            assert bool((diff <= 2.0 ** -23 * s).all()), float((diff / s.clamp_min(1e-30)).max())
            differ += int((diff != 0).sum())
            total += a.numel()
    print(f"polyak against torch mul_/add_: {differ} of {total} elements differ")


def test_sac_example_loss_kernel():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    from sac_torch import train
    hist = train("usv-simple", envs=256, steps=40, batch_size=64, learning_starts=8, train_freq=8, gradient_steps=4,
                 buffer_size=2560, seed=0, log=print, device_replay=True, sde_kernel=True, loss_kernel=True,
                 check_loss=True, max_episode_steps=11)
    assert len(hist) == 4 and hist[-1]["losses_checked"] == 16
    for h in hist:
        for key in ("actor_loss", "critic_loss", "ent_coef", "ent_coef_loss"):
            assert math.isfinite(h[key]), h
    d = hist[-1]["loss_diff"]
    print("example loss differences:", d)
    # the kernels and torch's float32 lines are two evaluations of one definition: each within the ceiling of it
    for key in ("critic", "actor", "ent_coef"):
        assert d[key] < S.CEILING, d
    assert d["polyak_ratio"] <= 2.0 ** -23, d
    with pytest.raises(ValueError):
        train("usv-simple", envs=64, steps=8, check_loss=True, log=print)
