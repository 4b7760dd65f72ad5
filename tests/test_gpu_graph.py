"""The graph-capturable update on the GPU: the device-resident step and noise counters (DeviceAdam, DeviceSDE and
DeviceCAPS with capturable=True: usv_adam_step_dev, usv_sde_*_dev, usv_caps_perturb_dev, usv_counter_add), their
replay through gym_usv_amd.capture_step, the refusals under capture and the SAC example with --graph.

Everything is compared as integers, no tolerance: the capturable forms against tests/optim_ref.py's restatement fed the
scalars the device derived (which are within 1 float32 ulp of the host's, the device's pow being another library) and
against the default forms at the same counter; the replays against the eager capturable run of the same number of
calls.  The frozen-counter assertions of the replay tests are what a capture built over host integers would fail:
a replay's noise differs from the one before it, and the clock block counts warm-up, capture and replays.

The issue's small gSDE shape (3, 5, 2) cannot exist: latent_dim is a multiple of 4 in [4, 4096] in both forms
(a ValueError, asserted below); (3, 8, 2) takes its place."""
import os
import sys

import numpy as np
import pytest
import torch

import optim_ref as R
import sde_squash_ref as Q
from test_clock_math import ulps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ADAM_LISTS = ((1, 3, 4, 4097, 8197),                       # across the 4-float padding and the 4 096-element chunk
              tuple(1 + i % 5 for i in range(97)))          # across the 96-tensor group: two launches per pass, one tick
SDE_SHAPES = ((3, 8, 2), (130, 300, 2))
SDE_PARTIALS = (2050, 4, 1)                                 # past 1 024 rows: two rows per partial of g_std
CAPS_SHAPES = ((3, 5), (256, 715))
RESETS = (0, 1, 3)
WARMUP, REPLAYS = 3, 5


def dev():
    return torch.device("cuda", 0)


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev())


def host(t):
    return t.detach().cpu().numpy().reshape(-1)


def same(a, b):
    return R.same(host(a) if isinstance(a, torch.Tensor) else a, host(b) if isinstance(b, torch.Tensor) else b)


def same_lists(a, b):
    return R.same(np.concatenate([host(x) if isinstance(x, torch.Tensor) else x for x in a]),
                  np.concatenate([host(x) if isinstance(x, torch.Tensor) else x for x in b]))


# ---- 1. Adam, eager
def make_adam(ps, max_norm, capturable):
    from gym_usv_amd import DeviceAdam
    params = [to_dev(p) for p in ps]
    return DeviceAdam(params, lr=R.HYPER["lr"], betas=(R.HYPER["beta1"], R.HYPER["beta2"]), eps=R.HYPER["eps"],
                      max_grad_norm=max_norm, capturable=capturable), params


def set_grads(params, gs):
    for p, g in zip(params, gs):
        p.grad = to_dev(g)


def moments(opt):
    return ([host(opt._segment(opt.exp_avg, i)) for i in range(len(opt.params))],
            [host(opt._segment(opt.exp_avg_sq, i)) for i in range(len(opt.params))])


def step_with(scal, *args, **kw):
    """tests/optim_ref.py's ``step`` fed the scalars ``scal`` in place of the ones it would take from ``t``."""
    keep = R.scalars
    R.scalars = lambda *a: scal
    try:
        return R.step(*args, **kw)
    finally:
        R.scalars = keep


def device_scalars(opt, t):
    """The block's scalars after step ``t`` as the restatement's dict: the step is ``t``, lr the host's, the two
    derived ones within 1 ulp of the host's.  Also whether they are the host's bits."""
    step, lr, step_size, bc2_sqrt = opt.clock()
    assert step == t and lr == R.HYPER["lr"]
    want = R.scalars(t, R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"], R.HYPER["eps"])
    got = dict(want, step_size=np.float32(step_size), bc2_sqrt=np.float32(bc2_sqrt))
    d = ulps([got["step_size"], got["bc2_sqrt"]], [want["step_size"], want["bc2_sqrt"]])
    print(f"step {t}: step_size {got['step_size']!r} bc2_sqrt {got['bc2_sqrt']!r}: {d.tolist()} ulp from the host's")
    assert d.max() <= 1
    return got, bool(d.max() == 0)


def check_against_restatement(opt, params, norm, want, key):
    ps, ms, vs, total = want
    m, v = moments(opt)
    assert same_lists(params, ps), key
    assert same_lists(m, ms) and same_lists(v, vs), key
    assert (norm is None) == (total is None), key
    if norm is not None:
        assert same(norm, [total]), key


@pytest.mark.parametrize("max_norm", (0.5, None))
@pytest.mark.parametrize("numels", ADAM_LISTS, ids=("chunks", "97"))
def test_adam_capturable_eager(numels, max_norm):
    ps, _, ms, vs = R.inputs(numels, seed=3)
    ms, vs = [np.zeros_like(m) for m in ms], [np.zeros_like(v) for v in vs]
    cap, cp = make_adam(ps, max_norm, True)
    plain, pp = make_adam(ps, max_norm, False)
    assert cap.step_count == 0 and cap.clock()[:2] == (0, R.HYPER["lr"])
    agree = True                                            # the two forms have had equal scalars so far
    for t in range(1, 6):
        gs = R.inputs(numels, seed=3 + 50 * t)[1]
        set_grads(cp, gs)
        set_grads(pp, gs)
        n_cap, n_plain = cap.step(), plain.step()
        scal, equal = device_scalars(cap, t)                # the step has advanced once, 97 tensors or five
        want = step_with(scal, ps, gs, ms, vs, t, max_norm=max_norm)
        if max_norm is not None:
            assert want[3] > max_norm                       # the clip bites
        check_against_restatement(cap, cp, n_cap, want, (len(numels), max_norm, t))
        ps, ms, vs = want[:3]
        agree = agree and equal
        if agree:                                           # equal scalars: the default form's bits
            assert same_lists(cp, pp) and all(same_lists(a, b) for a, b in zip(moments(cap), moments(plain)))
            assert n_cap is None or same(n_cap, n_plain)
    assert cap.step_count == 5 == plain.step_count

    # a checkpoint far along: load_state_dict writes the block, and the next step is 10^6 + 1
    sd = cap.state_dict()
    for st in sd["state"].values():
        st["step"] = torch.tensor(1.0e6)
    sd["param_groups"][0]["lr"] = R.HYPER["lr"]
    late, lp = make_adam(ps, max_norm, True)
    late.load_state_dict(sd)
    assert late.step_count == 10 ** 6 and late.clock()[1] == R.HYPER["lr"]
    gs = R.inputs(numels, seed=999)[1]
    set_grads(lp, gs)
    n_late = late.step()
    scal, _ = device_scalars(late, 10 ** 6 + 1)
    check_against_restatement(late, lp, n_late, step_with(scal, ps, gs, ms, vs, 10 ** 6 + 1, max_norm=max_norm),
                              (len(numels), max_norm, "late"))

    # state_dict() through torch.optim.Adam and back
    topt = torch.optim.Adam([torch.nn.Parameter(p.clone()) for p in cp], lr=1e-3)
    topt.load_state_dict(cap.state_dict())
    back, _ = make_adam(ps, max_norm, True)
    back.load_state_dict(topt.state_dict())
    assert back.step_count == 5 and back.lr == R.HYPER["lr"] == back.clock()[1] and back.betas == cap.betas
    assert all(same_lists(a, b) for a, b in zip(moments(back), moments(cap)))
    assert all(int(s["step"]) == 5 for s in topt.state_dict()["state"].values())


def test_adam_lr_is_a_stream_ordered_write():
    cap, cp = make_adam([np.ones(5, np.float32)], None, True)
    cap.lr = 1e-4
    assert cap.lr == 1e-4 == cap.clock()[1]
    set_grads(cp, [np.ones(5, np.float32)])
    cap.step()
    step, lr, step_size, _ = cap.clock()
    want = R.scalars(1, 1e-4, R.HYPER["beta1"], R.HYPER["beta2"], R.HYPER["eps"])
    assert step == 1 and ulps([step_size], [want["step_size"]]).max() <= 1
    with pytest.raises(ValueError):
        cap.lr = -1.0


# ---- 2. gSDE and CAPS, eager
def make_heads(n, L, A):
    import gym_usv_amd
    return [gym_usv_amd.DeviceSDE(n, L, A, dev(), Q.SEED, Q.LOW[:A], Q.HIGH[:A], env_id_offset=Q.GID0, copy=True,
                                  capturable=c) for c in (True, False)]


_SDE_INPUTS = {}


def sde_inputs(n, L, A):
    if (n, L, A) not in _SDE_INPUTS:
        _SDE_INPUTS[(n, L, A)] = tuple(to_dev(x) for x in Q.inputs(n, L, A))
    return _SDE_INPUTS[(n, L, A)]


def squashed_with_backward(head, inp, between=None):
    """``head.squashed`` on fresh leaves and its backward: (actions, env_actions, log_prob, gaussian_actions, g_mean,
    g_lat, g_std).  ``between`` runs after the forward."""
    mean, lat, std = (x.clone().requires_grad_(True) for x in inp[:3])
    ga, gl = inp[3], inp[4]
    out = head.squashed(mean, lat, std)
    if between is not None:
        between()
    ((out.actions * ga).sum() + (out.log_prob * gl).sum()).backward()
    return tuple(out) + (mean.grad, lat.grad, std.grad)


@pytest.mark.parametrize("n,L,A", SDE_SHAPES, ids=str)
def test_sde_capturable_equals_the_default_form_at_the_same_epoch(n, L, A):
    cap, plain = make_heads(n, L, A)
    inp = sde_inputs(n, L, A)
    mean, lat, std = inp[:3]
    done = 0
    for k in RESETS:
        while done < k:
            cap.reset_noise()
            done += 1
        plain.epoch = k
        assert cap.epoch == k
        for a, b in zip(cap.sample(mean, lat, std), plain.sample(mean, lat, std)):
            assert same(a, b), ("sample", k)
        assert same(cap.weights(std), plain.weights(std)), ("weights", k)
        for i, (a, b) in enumerate(zip(squashed_with_backward(cap, inp), squashed_with_backward(plain, inp))):
            assert same(a, b), ("squashed", k, i)
        for a, b in zip(cap.squashed(mean, lat, std), plain.squashed(mean, lat, std)):     # the no-grad path
            assert same(a, b), ("squashed, no grad", k)
    assert not same(plain.weights(std), make_heads(n, L, A)[1].weights(std))     # epoch 3 is not epoch 0
    cap.epoch = 0xFFFFFFFF
    assert cap.epoch == 0xFFFFFFFF
    plain.epoch = 0xFFFFFFFF
    assert same(cap.weights(std), plain.weights(std))
    cap.reset_noise()                                       # wraps
    plain.epoch = 0
    assert cap.epoch == 0 and same(cap.weights(std), plain.weights(std))
    with pytest.raises(RuntimeError, match="between"):
        squashed_with_backward(cap, inp, between=cap.reset_noise)
    with pytest.raises(RuntimeError, match="between"):
        squashed_with_backward(cap, inp, between=lambda: setattr(cap, "epoch", 5))
    squashed_with_backward(plain, inp, between=plain.reset_noise)       # the default form keeps the forward's epoch


def test_sde_capturable_backward_across_the_partials_boundary():
    n, L, A = SDE_PARTIALS
    cap, plain = make_heads(n, L, A)
    inp = sde_inputs(n, L, A)
    cap.reset_noise()
    plain.epoch = 1
    for i, (a, b) in enumerate(zip(squashed_with_backward(cap, inp), squashed_with_backward(plain, inp))):
        assert same(a, b), i


def test_the_issues_small_shape_is_refused_by_both_forms():
    import gym_usv_amd
    for c in (True, False):
        with pytest.raises(ValueError):
            gym_usv_amd.DeviceSDE(3, 5, 2, dev(), 1, Q.LOW, Q.HIGH, capturable=c)


def make_caps(capturable):
    import gym_usv_amd
    return gym_usv_amd.DeviceCAPS(dev(), 23, eps_s=0.1, capturable=capturable)


def caps_obs(B, W):
    g = torch.Generator(device="cpu").manual_seed(100 * B + W)
    return torch.randn((B, W), generator=g).to(dev())


@pytest.mark.parametrize("B,W", CAPS_SHAPES, ids=str)
def test_caps_capturable_equals_the_default_form_at_the_same_epoch(B, W):
    cap, plain = make_caps(True), make_caps(False)
    obs = caps_obs(B, W)
    done, seen = 0, []
    for k in RESETS:
        while done < k:
            cap.reset_noise()
            done += 1
        plain.epoch = k
        assert cap.epoch == k
        a = cap.near(obs)
        assert same(a, plain.near(obs)), k
        seen.append(host(a))
    assert not R.same(seen[0], seen[1]) and not R.same(seen[1], seen[2])
    cap.epoch = 0xFFFFFFFF
    plain.epoch = 0xFFFFFFFF
    assert cap.epoch == 0xFFFFFFFF and same(cap.near(obs), plain.near(obs))
    cap.reset_noise()
    assert cap.epoch == 0 and R.same(host(cap.near(obs)), seen[0])


# ---- 3. replays
def replayed(make, calls_before_replays=WARMUP + 1):
    """``make()`` gives (fn, state, feed): ``fn`` the step, ``state()`` a tuple of arrays, ``feed(j)`` what changes the
    step's inputs before call ``j`` (0: the warm-up and capture calls; 1..: replay j).  Runs it captured and eagerly and
    compares the state after every replay; returns the captured run's states."""
    from gym_usv_amd import capture_step
    fn, state, feed = make()
    feed(0)
    captured = capture_step(fn, warmup=WARMUP)
    efn, estate, efeed = make()
    efeed(0)
    for _ in range(calls_before_replays):
        efn()
    states = []
    for j in range(1, REPLAYS + 1):
        feed(j)
        captured.replay()
        efeed(j)
        efn()
        got, want = state(captured), estate(None)
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert R.same(a, b), (j, i)
        states.append(got)
    return states


def test_adam_replays_count_their_steps():
    numels = ADAM_LISTS[0]
    opts = []

    def make():
        ps = R.inputs(numels, seed=5)[0]
        opt, params = make_adam(ps, 0.5, True)
        set_grads(params, [np.zeros_like(p) for p in ps])  # static: a replay reads these addresses
        last = []

        def fn():
            last[:] = [opt.step()]
            return last[0]

        def feed(j):
            for p, g in zip(params, R.inputs(numels, seed=70 + j)[1]):
                p.grad.copy_(to_dev(g))

        def state(captured):
            m, v = moments(opt)
            return [host(p) for p in params] + m + v + [host(captured.out if captured is not None else last[0])]

        opts.append(opt)
        return fn, state, feed

    states = replayed(make)
    cap, eager = opts
    assert cap.step_count == WARMUP + 1 + REPLAYS == eager.step_count       # not the captured step over and over
    assert cap.clock() == eager.clock()
    assert not R.same(states[0][-1], states[1][-1])         # the static norm holds each replay's own


def test_sde_replays_draw_new_noise():
    n, L, A = SDE_SHAPES[1]
    inp = sde_inputs(n, L, A)
    heads = []

    def make():
        head = make_heads(n, L, A)[0]
        leaves = [x.clone().requires_grad_(True) for x in inp[:3]]
        last = []

        def fn():
            head.reset_noise()
            for x in leaves:
                x.grad = None                               # inside: the captured backward allocates from the graph's pool
            out = head.squashed(*leaves)
            ((out.actions * inp[3]).sum() + (out.log_prob * inp[4]).sum()).backward()
            last[:] = [tuple(t.detach() for t in out) + tuple(x.grad for x in leaves)]      # the autograd graph goes
            return last[0]

        heads.append(head)
        return fn, lambda c: [host(t) for t in (c.out if c is not None else last[0])], lambda j: None

    states = replayed(make)
    assert not R.same(states[0][0], states[1][0])           # replay 2's actions are not replay 1's
    assert not R.same(states[0][5], states[1][5])           # ... nor its g_lat
    assert heads[0].epoch == WARMUP + 1 + REPLAYS == heads[1].epoch


def test_caps_replays_draw_new_noise():
    B, W = CAPS_SHAPES[1]
    obs = caps_obs(B, W)
    objs = []

    def make():
        caps = make_caps(True)
        last = []

        def fn():
            caps.reset_noise()
            last[:] = [caps.near(obs)]
            return last[0]

        objs.append(caps)
        return fn, lambda c: [host(c.out if c is not None else last[0])], lambda j: None

    states = replayed(make)
    assert not R.same(states[0][0], states[1][0])
    assert objs[0].epoch == WARMUP + 1 + REPLAYS == objs[1].epoch


def test_polyak_replays():
    import gym_usv_amd

    def make():
        src = [to_dev(p) for p in R.inputs(ADAM_LISTS[0], seed=8)[0]]
        dst = [torch.zeros_like(p) for p in src]
        pol = gym_usv_amd.DevicePolyak(src, dst)

        def feed(j):
            for p, g in zip(src, R.inputs(ADAM_LISTS[0], seed=40 + j)[0]):
                p.copy_(to_dev(g))

        return (lambda: pol.step(0.005)), (lambda c: [host(t) for t in dst]), feed

    states = replayed(make)
    assert not R.same(np.concatenate(states[0]), np.concatenate(states[1]))


def test_polyak_prepare_uploads_and_step_needs_no_upload_then():
    import gym_usv_amd
    src, dst = [to_dev(np.arange(9))], [to_dev(np.zeros(9))]
    pol = gym_usv_amd.DevicePolyak(src, dst)
    pol.prepare()
    assert pol._ptrs == pol._current()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pol.step(0.5)                                       # no upload pending: legal under capture, first step or not
    g.replay()
    torch.cuda.synchronize()
    assert same(dst[0], np.arange(9) * np.float32(0.5))


# ---- 5. the example
def test_sac_example_with_graph():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import sac_torch
    flags = dict(device_replay=True, sde_kernel=True, loss_kernel=True, adam_kernel=True, caps=True, caps_kernel=True)
    for bad in (dict(flags, adam_kernel=False), dict(flags, caps_kernel=False), dict(flags, device_replay=False),
                dict(flags, sde_kernel=False), dict(flags, check_loss=True)):
        with pytest.raises(ValueError):
            sac_torch.train(envs=64, steps=8, graph=True, log=lambda s: None, **bad)
    cfg = dict(envs=64, steps=24, seed=3, log=lambda s: None, buffer_size=64 * 64, batch_size=64, learning_starts=8,
               train_freq=8, gradient_steps=3, **flags)     # two rounds: six gradient steps

    def run(graph):
        keep = []
        hist = sac_torch.train(graph=graph, keep=keep, **cfg)
        sac = keep[0]
        params = [p.detach().clone() for m in (sac.actor, sac.critic, sac.target) for p in m.parameters()] + \
            [sac.log_ent.detach().clone()]
        return hist, params, sac

    h1, p1, sac = run(True)
    h2, p2, _ = run(True)
    assert len(h1) == 2 and sac.opt_a.step_count == 6 == sac.opt_c.step_count == sac.opt_e.step_count
    assert sac.head_mb.epoch == 6 == sac.caps_dev.epoch     # the warm-up's four steps were undone
    assert same_lists(p1, p2)                               # two runs of one seed
    for rec in h1:
        for k in ("actor_loss", "critic_loss", "ent_coef", "ent_coef_loss", "caps_temporal", "caps_spatial"):
            assert np.isfinite(rec[k]), (k, rec)
    h3, p3, _ = run(False)
    diff = max(float((a - b).abs().max()) for a, b in zip(p1, p3))
    print(f"SAC example, 64 envs, six gradient steps: largest |parameter difference| with and without --graph = {diff!r}")
    assert np.isfinite(diff)


# ---- 4. refusals under capture (last: an error here must not reach another test through an invalidated stream)
def test_refusals_under_capture_leave_the_capture_valid():
    import gym_usv_amd
    n, L, A = SDE_SHAPES[0]
    inp = sde_inputs(n, L, A)
    plain_opt, pp = make_adam([np.ones(7, np.float32)], 0.5, False)
    set_grads(pp, [np.ones(7, np.float32)])
    cap_opt, cpar = make_adam([np.ones(7, np.float32)], 0.5, True)
    set_grads(cpar, [np.ones(7, np.float32)])
    cap_head, plain_head = make_heads(n, L, A)
    plain_caps, obs = make_caps(False), caps_obs(3, 5)
    pol = gym_usv_amd.DevicePolyak([to_dev(np.ones(9))], [to_dev(np.zeros(9))])      # never stepped: upload pending
    leaves = [x.clone().requires_grad_(True) for x in inp[:3]]
    counter = torch.zeros(4, device=dev())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                               # its exit ends the capture, as a finally does
        counter.add_(1.0)
        with pytest.raises(RuntimeError, match="capturable=True"):
            plain_opt.step()
        with pytest.raises(RuntimeError, match="capturable=True"):
            plain_head.squashed(*leaves)
        with pytest.raises(RuntimeError, match="capturable=True"):
            plain_head.sample(*inp[:3])
        with pytest.raises(RuntimeError, match="capturable=True"):
            plain_head.weights(inp[2])
        with pytest.raises(RuntimeError, match="capturable=True"):
            plain_caps.near(obs)
        with pytest.raises(RuntimeError, match="prepare"):
            pol.step(0.005)
        with pytest.raises(RuntimeError, match="captur"):
            pol.prepare()
        with pytest.raises(RuntimeError, match="captur"):
            cap_opt.lr = 1e-4
        with pytest.raises(RuntimeError, match="captur"):
            cap_head.epoch = 3
        counter.add_(1.0)
    g.replay()
    torch.cuda.synchronize()                                # no invalidated-capture error is pending
    assert counter.tolist() == [2.0] * 4
    assert plain_opt.step_count == 0 and cap_opt.step_count == 0 and pol._ptrs is None
    plain_opt.step()                                        # and the refused objects work outside a capture
    pol.step(0.005)
    torch.cuda.synchronize()
    assert plain_opt.step_count == 1
