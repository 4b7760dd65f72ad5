"""The fused optimizer step on the GPU (gym_usv_amd.DeviceAdam: usv_adam_step).

Bitwise, against the NumPy float32 restatement (tests/optim_ref.py): parameters, both moments and the norm over three
consecutive steps on the lists of the host test, with clipping that bites, clipping that does not and none; views 4 B
off a 16-B boundary against their aligned copies; a list that takes two launches per pass against one tensor of the
same chunks; repeated steps, a second stream, the ticket word.

Against torch.optim.Adam (float32) + clip_grad_norm_ on the device, one step from the same state three times over:
each quantity over the sum of the magnitudes of its terms, under the bound of the float64 comparison
(test_optim_math.BOUND: 4x the errors measured there) and, independently, under the 1e-5 ceiling.  Both are float32
evaluations of one definition; the number of elements that differ at all is printed.

state_dict round trips through torch.optim.Adam, .grad, zero_grad, and the two examples with adam_kernel=True."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import optim_ref as R
from test_optim_math import BITES, BOUND, LISTS, SPARES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev())


def host(t):
    return t.detach().cpu().numpy().reshape(-1)


def shifted(x):
    """`x` as a view one element into a fresh buffer: 4-B but not 16-B aligned."""
    base = torch.empty(len(x) + 1, dtype=torch.float32, device=dev())
    base[1:] = to_dev(x)
    v = base[1:]
    assert v.data_ptr() % 16 == 4
    return v


def make(ps, max_norm, shift=False):
    from gym_usv_amd import DeviceAdam
    params = [shifted(p) if shift else to_dev(p) for p in ps]
    return DeviceAdam(params, lr=R.HYPER["lr"], betas=(R.HYPER["beta1"], R.HYPER["beta2"]), eps=R.HYPER["eps"],
                      max_grad_norm=max_norm), params


def set_grads(params, gs, shift=False):
    for p, g in zip(params, gs):
        p.grad = shifted(g) if shift else to_dev(g)


def moments(opt):
    return ([host(opt._segment(opt.exp_avg, i)) for i in range(len(opt.params))],
            [host(opt._segment(opt.exp_avg_sq, i)) for i in range(len(opt.params))])


def ticket(opt):
    return int(opt._scratch[:1].view(torch.int32).item())


def same_lists(a, b):
    return R.same(np.concatenate(a), np.concatenate(b))


def run_steps(numels, max_norm, steps=3, shift=False, seed=0):
    """`steps` consecutive steps from zero moments, each checked against the restatement; the final (p, m, v, norm)."""
    ps, _, ms, vs = R.inputs(numels, seed=seed)
    ms, vs = [np.zeros_like(m) for m in ms], [np.zeros_like(v) for v in vs]
    opt, params = make(ps, max_norm, shift)
    norm = None
    for t in range(1, steps + 1):
        gs = R.inputs(numels, seed=seed + 50 * t)[1]
        set_grads(params, gs, shift)
        norm = opt.step()
        ps, ms, vs, total = R.step(ps, gs, ms, vs, t, max_norm=max_norm)
        m, v = moments(opt)
        key = (list(numels)[:4], len(numels), max_norm, t, shift)
        assert same_lists([host(p) for p in params], ps), key
        assert same_lists(m, ms) and same_lists(v, vs), key
        assert (norm is None) == (max_norm is None), key
        if norm is not None:
            assert norm.shape == () and R.same(host(norm), [total]), (key, host(norm), total)
        assert all(R.same(host(p.grad), g) for p, g in zip(params, gs)), key     # .grad is not written
        assert ticket(opt) == 0 and opt.step_count == t, key
    return [host(p) for p in params], *moments(opt), None if norm is None else host(norm)


@pytest.mark.parametrize("max_norm", (BITES, SPARES, None))
def test_device_equals_the_restatement_bitwise(max_norm):
    for numels in LISTS:
        run_steps(numels, max_norm)


@pytest.mark.parametrize("max_norm", (BITES, None))
def test_misaligned_views_give_the_bits_of_their_aligned_copies(max_norm):
    for numels in (R.NUMELS, (2 * R.C + 3,)):
        a = run_steps(numels, max_norm)
        b = run_steps(numels, max_norm, shift=True)
        assert all(same_lists(x, y) for x, y in zip(a[:3], b[:3]))
        assert max_norm is None or R.same(a[3], b[3])


def test_step_1000_and_bad_gradients_equal_the_restatement_bitwise():
    numels = R.NUMELS
    for bad, max_norm in ((None, BITES), (np.inf, BITES), (np.nan, BITES), (np.inf, None), (np.nan, None)):
        ps, gs, ms, vs = R.inputs(numels, seed=5, bad=bad)
        opt, params = make(ps, max_norm)
        sd = opt.state_dict()
        sd["state"] = {i: {"step": torch.tensor(999.0), "exp_avg": to_dev(m), "exp_avg_sq": to_dev(v)}
                       for i, (m, v) in enumerate(zip(ms, vs))}
        opt.load_state_dict(sd)
        assert opt.step_count == 999
        set_grads(params, gs)
        norm = opt.step()
        want = R.step(ps, gs, ms, vs, 1000, max_norm=max_norm)
        m, v = moments(opt)
        assert same_lists([host(p) for p in params], want[0]) and same_lists(m, want[1]) and same_lists(v, want[2]), bad
        if max_norm is not None:
            assert R.same(host(norm), [want[3]])
        if bad is not None:
            assert np.isnan(np.concatenate(want[0])).sum() == (
                sum(numels) if (max_norm is not None and np.isnan(bad)) else 1)


def test_a_list_over_two_launches_sums_as_one_tensor_of_the_same_chunks():
    """130 tensors of C elements take two launches per pass (96 tensors a launch); one tensor of 130 C elements has
    the same chunks: the same norm and the same updated elements, bitwise, and the restatement's norm."""
    n = 130
    assert n > R.K
    rng = np.random.default_rng(8)
    p, g = rng.standard_normal(n * R.C).astype(np.float32), rng.standard_normal(n * R.C).astype(np.float32)
    opt_l, params_l = make(list(p.reshape(n, R.C)), 0.5)
    opt_1, params_1 = make([p], 0.5)
    for t in range(2):
        set_grads(params_l, list(g.reshape(n, R.C)))
        set_grads(params_1, [g])
        norm_l, norm_1 = opt_l.step(), opt_1.step()
        assert R.same(host(norm_l), host(norm_1)) and ticket(opt_l) == 0 == ticket(opt_1)
        assert R.same(np.concatenate([host(x) for x in params_l]), host(params_1[0]))
        if t == 0:
            assert R.same(host(norm_1), [R.total_norm([g])])
    assert R.same(host(opt_l.exp_avg), host(opt_1.exp_avg)) and R.same(host(opt_l.exp_avg_sq), host(opt_1.exp_avg_sq))


def test_repeated_steps_and_a_second_stream_give_equal_bits():
    numels = R.NUMELS + (R.BIG,)
    ps, gs, _, _ = R.inputs(numels, seed=9)
    outs = []
    side = torch.cuda.Stream(device=dev())
    for k in range(4):
        opt, params = make(ps, 0.5)
        set_grads(params, gs)
        if k == 3:
            side.wait_stream(torch.cuda.current_stream(dev()))
            with torch.cuda.stream(side):
                norms = [opt.step(), opt.step()]
            side.synchronize()
        else:
            norms = [opt.step(), opt.step()]
        assert ticket(opt) == 0
        outs.append(([host(p) for p in params], *moments(opt), [host(x) for x in norms]))
    for o in outs[1:]:
        assert all(same_lists(a, b) for a, b in zip(o, outs[0]))


def test_against_torch_adam_on_the_device():
    numels = R.NUMELS + (2 * R.C + 3,)
    scale = lambda i: 10.0 ** -(i % 5)                    # noqa: E731
    worst, differ, count = {}, 0, 0
    for max_norm in (0.5, None):
        ps = R.inputs(numels, seed=21, scale=scale)[0]
        opt, params = make(ps, max_norm)
        theirs = [p.clone() for p in params]
        ref = torch.optim.Adam(theirs, lr=R.HYPER["lr"], betas=(R.HYPER["beta1"], R.HYPER["beta2"]), eps=R.HYPER["eps"])
        for t in range(1, 4):
            gs = R.inputs(numels, seed=21 + t, scale=scale)[1]
            before = ([host(p) for p in params], gs, *moments(opt))
            set_grads(params, gs)
            set_grads(theirs, gs)
            for a, b in zip(theirs, params):              # one step from the same state
                a.data.copy_(b)
            ref.load_state_dict(opt.state_dict())
            total = None
            if max_norm is not None:
                total = float(torch.nn.utils.clip_grad_norm_(theirs, max_norm))
            ref.step()
            norm = opt.step()
            st = ref.state_dict()["state"]
            want = ([host(p).astype(np.float64) for p in theirs],
                    [host(st[i]["exp_avg"]).astype(np.float64) for i in range(len(numels))],
                    [host(st[i]["exp_avg_sq"]).astype(np.float64) for i in range(len(numels))], total)
            got = ([host(p) for p in params], *moments(opt), None if norm is None else host(norm)[0])
            for k, v in R.errors(got, want, R.scales(*before, t, max_norm=max_norm)).items():
                worst[k] = max(worst.get(k, 0.0), v)
            differ += int(sum((a != b).sum() for a, b in zip(got[0], want[0])))
            count += sum(numels)
    print(f"DeviceAdam against torch.optim.Adam float32: {worst}; {differ} of {count} parameter elements differ")
    for k, v in worst.items():
        assert math.isfinite(v) and v < R.CEILING and v <= BOUND[k], (k, v, BOUND[k])


def test_state_dict_round_trips_through_torch_adam():
    numels = (5, 300, R.C + 1)
    ps = R.inputs(numels, seed=31)[0]
    hyper = dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-7)
    from gym_usv_amd import DeviceAdam
    a_params = [to_dev(p).view(-1, 1) if i == 1 else to_dev(p) for i, p in enumerate(ps)]
    a = DeviceAdam(a_params, max_grad_norm=None, **hyper)
    assert a.state_dict()["state"] == {}
    for t in range(2):
        set_grads(a_params, [g.reshape(p.shape) for g, p in zip(R.inputs(numels, seed=32 + t)[1], a_params)])
        a.step()
    sd = a.state_dict()
    assert set(sd) == {"state", "param_groups"} and len(sd["param_groups"]) == 1 and sd["param_groups"][0]["lr"] == 1e-3
    assert all(sd["state"][i]["exp_avg"].shape == a_params[i].shape and float(sd["state"][i]["step"]) == 2.0 for i in range(3))
    # into torch and back into a second DeviceAdam: the same moments, count and hyper-parameters
    t_params = [p.clone() for p in a_params]
    ref = torch.optim.Adam(t_params)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["betas"] == (0.8, 0.99)
    b_params = [p.clone() for p in a_params]
    b = DeviceAdam(b_params)
    b.load_state_dict(ref.state_dict())
    assert (b.lr, b.betas, b.eps, b.step_count) == (1e-3, (0.8, 0.99), 1e-7, 2)
    assert R.same(host(a.exp_avg), host(b.exp_avg)) and R.same(host(a.exp_avg_sq), host(b.exp_avg_sq))
    # stepping continues with equal results after the load, and torch's own step from the loaded state is close
    gs = R.inputs(numels, seed=40)[1]
    for params in (a_params, b_params, t_params):
        set_grads(params, [g.reshape(p.shape) for g, p in zip(gs, params)])
    a.step(), b.step(), ref.step()
    assert all(R.same(host(x), host(y)) for x, y in zip(a_params, b_params))
    assert all(torch.allclose(x, y, rtol=1e-5, atol=1e-7) for x, y in zip(a_params, t_params))
    assert int(ref.state_dict()["state"][0]["step"]) == 3 == a.step_count
    with pytest.raises(ValueError):
        b.load_state_dict(torch.optim.Adam([b_params[0]]).state_dict())          # another number of parameters


def test_grad_rules_zero_grad_and_lr():
    from gym_usv_amd import DeviceAdam, UsvLibError
    w = torch.nn.Parameter(to_dev(np.ones((4, 6), np.float32)))
    b = torch.nn.Parameter(to_dev(np.ones(6, np.float32)))
    opt = DeviceAdam([w, b], lr=0.1, max_grad_norm=10.0)
    (w.sum() + b.sum()).backward()
    keep = (w.grad.clone(), b.grad.clone())
    norm = opt.step()
    assert torch.equal(w.grad, keep[0]) and torch.equal(b.grad, keep[1])         # unchanged by step()
    assert abs(float(norm) - math.sqrt(30.0)) < 1e-5
    assert torch.allclose(w, torch.full_like(w, 0.9), atol=1e-6)                  # Adam's first step: lr * sign(g)
    opt.zero_grad()
    assert w.grad is None and b.grad is None
    with pytest.raises(ValueError):                                               # torch would skip it
        opt.step()
    assert opt.step_count == 1
    # a non-contiguous gradient is copied; lr is read at every step
    opt.lr = 0.0
    w.grad, b.grad = torch.ones((6, 4), device=dev()).t(), torch.ones(6, device=dev())
    assert not w.grad.is_contiguous()
    before = w.detach().clone()
    opt.step()
    assert torch.equal(w, before) and opt.step_count == 2
    opt.lr = float("nan")
    with pytest.raises(UsvLibError):
        opt.step()
    assert opt.step_count == 2
    with pytest.raises(ValueError):
        DeviceAdam([w.detach().t()])


def ppo_run(adam_kernel):
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    import gym_usv_amd
    from ppo_torch import PPO
    env = gym_usv_amd.make_vec("usv-simple", 256, seed=0, copy=False)
    ppo = PPO(env, n_steps=8, batch_size=512, seed=0, fused=True, frames=True, sde_kernel=True, eval_kernel=True,
              adam_kernel=adam_kernel)
    first = torch.cat([p.detach().flatten() for p in ppo.model.parameters()]).cpu()
    recs = []
    for _ in range(2):
        ppo.rollout()
        recs.append(ppo.update())
    last = torch.cat([p.detach().flatten() for p in ppo.model.parameters()]).cpu()
    env.close()
    return recs, first, last


def test_ppo_example_adam_kernel():
    from gym_usv_amd import DeviceAdam
    recs, first, last = ppo_run(True)
    assert all(math.isfinite(r[k]) for r in recs for k in ("policy_loss", "value_loss", "entropy", "std_mean")), recs
    assert torch.isfinite(last).all() and not torch.equal(first, last)
    _, first2, last2 = ppo_run(True)
    assert torch.equal(first, first2) and torch.equal(last.view(torch.int32), last2.view(torch.int32))
    from ppo_torch import train
    hist = train(envs=256, updates=1, n_steps=8, batch_size=512, log=lambda s: None, fused=True, adam_kernel=True)
    assert len(hist) == 1 and math.isfinite(hist[0]["value_loss"])
    assert DeviceAdam.__module__ == "gym_usv_amd.optim"


def sac_run(adam_kernel):
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    import gym_usv_amd
    from sac_torch import SAC
    env = gym_usv_amd.make_vec("usv-simple", 256, seed=0, copy=False, max_episode_steps=11)
    sac = SAC(env, seed=0, device_replay=True, sde_kernel=True, loss_kernel=True, adam_kernel=adam_kernel, batch_size=64,
              learning_starts=8, train_freq=8, gradient_steps=4, buffer_size=2560)
    nets = (sac.actor, sac.critic)
    flat = lambda: torch.cat([p.detach().flatten() for n in nets for p in n.parameters()] + [sac.log_ent.detach()]).cpu()  # noqa: E731
    first, hist = flat(), []
    for at in range(0, 24, 8):
        sac.collect(8, random_actions=at < 8)
        if at >= 8:
            hist.append(sac.train(4))
    last = flat()
    env.close()
    return hist, first, last


def test_sac_example_adam_kernel():
    hist, first, last = sac_run(True)
    assert len(hist) == 2
    assert all(math.isfinite(h[k]) for h in hist for k in ("actor_loss", "critic_loss", "ent_coef", "ent_coef_loss")), hist
    assert torch.isfinite(last).all() and not torch.equal(first, last) and last[-1] != first[-1]
    _, first2, last2 = sac_run(True)
    assert torch.equal(first, first2) and torch.equal(last.view(torch.int32), last2.view(torch.int32))
    from sac_torch import train
    hist = train("usv-simple", envs=64, steps=24, batch_size=32, learning_starts=8, train_freq=8, gradient_steps=2,
                 buffer_size=640, seed=0, log=lambda s: None, device_replay=True, adam_kernel=True, max_episode_steps=11)
    assert len(hist) == 2 and all(math.isfinite(h["critic_loss"]) for h in hist), hist
