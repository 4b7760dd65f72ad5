"""N-step sampling of the device replay buffer on the GPU (DeviceReplay.gather_nstep / sample_nstep:
usv_replay_gather_nstep) against SB3's NStepReplayBuffer._get_samples restated on full storage
(tests/replay_nstep_ref.py): the same scripted steps go into both, and every gathered output must equal the
reference's.  Every comparison is bitwise (tensors compared as integers): no tolerance."""
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

import replay_nstep_ref as N
import replay_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

A = 2
BATCHES = (1, 3, 4, 5, 257)             # the samples-per-wave tail, a full wave of four, more than a block
N_STEPS = (1, 2, 3, 7, 8, 32)           # beyond R, beyond k, runs that wrap the slot ring, the largest
GAMMAS = (0.99, 1.0, 0.0)
FIELDS = ("observations", "actions", "next_observations", "dones", "rewards", "discounts")


def dev():
    return torch.device("cuda", 0)


def bits_t(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits_t(a), bits_t(b))


def off_by_one_float(t):
    """A contiguous copy of float32 `t` whose base is one float past its allocation."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.flatten()
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


def make(n, R, k, D, keep, misaligned=False):
    from gym_usv_amd.replay import DeviceReplay
    rb = DeviceReplay(n, R * n, k * D, A, dev(), n_stack=k, clear_keeps_sign=keep)
    assert rb.rows == R and (rb.n_steps, rb.gamma) == (1, 0.99)
    if misaligned:
        for name in ("frames", "next_frame", "act", "rew"):
            setattr(rb, name, off_by_one_float(getattr(rb, name)))
        rb._bind()
    return rb


def upload(sc):
    return {key: torch.from_numpy(np.ascontiguousarray(v)).to(dev()) for key, v in sc.items()}


def feed(rb, g, lo, hi, misaligned=False):
    give = off_by_one_float if misaligned else (lambda t: t)
    for t in range(lo, hi):
        rb.put_obs(give(g["windows"][t]), give(g["act"][t]))
        rb.put_step(give(g["rew"][t]), g["term"][t], g["trunc"][t], give(g["windows"][t + 1]), give(g["final_stack"][t]))


def compare(rb, ref, count, n_steps, gamma, seen, seed=0, misaligned=False):
    """Every valid index (in order and permuted) and every batch size of BATCHES through `rb.gather_nstep`.
    The reference is computed once, for every valid index, and read at the indices of each set."""
    from gym_usv_amd.replay import NStepReplaySamples
    assert (rb.size, rb.pos, rb.full) == (ref.size, ref.pos, ref.full)
    M = ref.size * ref.n
    rb.set_n_steps(n_steps, gamma)
    want, m, _, kinds = N.get_nstep(ref, np.arange(M), n_steps, gamma, count=count)
    assert (m <= min(n_steps, ref.size) - 1).all()
    np.add.at(seen, kinds, 1)
    want = [torch.from_numpy(np.ascontiguousarray(w)).to(dev()) for w in want]
    gen = torch.Generator().manual_seed(seed)
    sets = [torch.cat((torch.arange(M), torch.randperm(M, generator=gen)))]
    sets += [torch.randint(0, M, (B,), generator=gen) for B in BATCHES]
    differ = []
    for i in sets:
        i = i.to(dev())
        out = None
        if misaligned:
            out = tuple(off_by_one_float(torch.zeros((i.numel(), w.shape[1]), device=dev())) for w in want)
        got = rb.gather_nstep(i, out=out)
        assert isinstance(got, NStepReplaySamples) and got._fields == FIELDS
        for t, w in zip(got, want):
            assert t.shape == (i.numel(), w.shape[1])
            differ.append((bits_t(t) != bits_t(w[i])).any())
    differ = torch.stack(differ).reshape(len(sets), len(FIELDS)).cpu()          # one read-back per call
    assert not differ.any(), ([(s, FIELDS[f]) for s, f in differ.nonzero().tolist()], rb.n, rb.n_stack, rb.d, rb.rows,
                              count, n_steps, gamma)


def check(n, k, D, R, keep, pattern, seen, n_steps=N_STEPS, misaligned=False, turn=0):
    counts = P.counts_of(R)
    sc = P.script(n, max(counts), k, D, A, pattern, keep)
    refs = P.run(sc, n, R, k, D, A, counts)
    rb, g = make(n, R, k, D, keep, misaligned), upload(sc)
    at = 0
    for c in counts:
        feed(rb, g, at, c, misaligned)
        at = c
        for i, ns in enumerate(n_steps):
            compare(rb, refs[c], c, ns, GAMMAS[(i + c + turn) % len(GAMMAS)], seen, seed=n + c, misaligned=misaligned)
    assert rb.bad_indices() == 0
    return rb, refs[counts[-1]], counts[-1]


def all_stops_seen(seen):
    """A run stopped by a done, by a timeout and at the last stored row, and one not stopped: a script that
    never cuts a run shows nothing."""
    assert (seen > 0).all(), dict(zip(N.STOPS, seen.tolist()))


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("k", (1, 2, 5))
@pytest.mark.parametrize("n", (1, 65))
def test_scripted_stores_equal_the_definition(n, k, keep):
    seen, turn = np.zeros(4, np.int64), 0
    for D in (1, 3, 4, 143):
        for R in sorted({1, 2, 3, k + 2}):
            check(n, k, D, R, keep, P.PATTERNS[(turn + n + k) % len(P.PATTERNS)], seen, turn=turn)
            turn += 1
    assert turn >= len(P.PATTERNS)                      # every pattern was used
    all_stops_seen(seen)


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_done_patterns(pattern):
    """Every pattern at a shape whose windows wrap the frame ring and whose runs wrap the slot ring."""
    seen = np.zeros(4, np.int64)
    for keep in (False, True):
        check(65, 5, 6, 7, keep, pattern, seen, n_steps=(2, 3, 8))
    assert seen[2] > 0 and seen[3] > 0
    assert seen[0] > 0 or pattern in ("none", "all_trunc", "consecutive", "last")
    assert seen[1] > 0 or pattern in ("none", "both", "double")


def test_n_steps_1_is_gather():
    seen = np.zeros(4, np.int64)
    for keep, gamma in ((False, 0.99), (True, 0.5)):
        rb, ref, count = check(65, 5, 6, 7, keep, "random", seen, n_steps=(1,))
        rb.set_n_steps(1, gamma)
        M = ref.size * ref.n
        i = torch.cat((torch.arange(M), torch.randperm(M, generator=torch.Generator().manual_seed(3)))).to(dev())
        one, ns = rb.gather(i), rb.gather_nstep(i)
        for a, b in zip(one, ns[:5]):
            assert same(a, b)
        assert same(ns.discounts, torch.full((2 * M, 1), float(np.float32(gamma)), device=dev()))
    all_stops_seen(seen)


@pytest.mark.parametrize("keep", (False, True))
def test_misaligned_bases(keep):
    seen = np.zeros(4, np.int64)
    for k, D, R in ((5, 6, 2), (5, 143, 3)):
        check(65, k, D, R, keep, "random", seen, misaligned=True)      # every base one float past its allocation
    all_stops_seen(seen)


def test_bad_and_out_of_range_indices():
    n, k, D, R = 65, 5, 6, 7
    sc = P.script(n, R + 1, k, D, A, "double", True)
    refs = P.run(sc, n, R, k, D, A, [3, R + 1])
    rb, g = make(n, R, k, D, True), upload(sc)
    rb.set_n_steps(3, 0.99)
    raw = [3, -1, 4, 3 * n, 3 * n - 1, 2 ** 40, 0, -2 ** 63, -n, 5 * n + 2, R * n, R * n - 1]
    idx = torch.tensor(raw, dtype=torch.int64, device=dev())
    expect, at = 0, 0
    for count in (3, R + 1):
        feed(rb, g, at, count)
        at = count
        ok = (idx >= 0) & (idx < min(count, R) * n)       # 5 n + 2 and R n - 1 are valid only once the ring is full
        got = rb.gather_nstep(idx)                        # no error status: the call returns
        expect += int((~ok).sum())
        assert rb.bad_indices() == expect
        want, _, _, _ = N.get_nstep(refs[count], idx[ok].cpu().numpy(), 3, 0.99, count=count)
        assert len(got) == 6
        for t, w in zip(got, want):
            assert torch.isnan(t[~ok]).all()
            assert same(t[ok], torch.from_numpy(np.ascontiguousarray(w)).to(dev()))
    rb.gather_nstep(idx[1:2])                             # B = 1, bad
    assert rb.bad_indices() == expect + 1


def test_refused_between_put_obs_and_put_step_and_no_host_sync():
    from gym_usv_amd.replay import DeviceReplay
    n, k, D, R = 65, 5, 6, 3
    sc = P.script(n, 3, k, D, A)
    rb, g = make(n, R, k, D, False), upload(sc)
    rb.set_n_steps(3, 0.99)
    with pytest.raises(RuntimeError):
        rb.sample_nstep(4)                                # empty
    feed(rb, g, 0, 2)
    idx = torch.arange(4, device=dev())
    rb.gather_nstep(idx)
    rb.put_obs(g["windows"][2], g["act"][2])
    with pytest.raises(RuntimeError):
        rb.gather_nstep(idx)
    with pytest.raises(RuntimeError):
        rb.sample_nstep(4)
    rb.put_step(g["rew"][2], g["term"][2], g["trunc"][2], g["windows"][3], g["final_stack"][2])
    mb = rb.sample_nstep(2048, generator=torch.Generator(device=dev()).manual_seed(1))
    assert [tuple(t.shape) for t in mb] == [(2048, k * D), (2048, A), (2048, k * D), (2048, 1), (2048, 1), (2048, 1)]
    assert not any(torch.isnan(t).any() for t in mb) and rb.bad_indices() == 0
    for bad in (dict(n_steps=0, gamma=0.9), dict(n_steps=33, gamma=0.9), dict(n_steps=2, gamma=1.5)):
        with pytest.raises(ValueError):
            rb.set_n_steps(**bad)
    for fn in (DeviceReplay.sample_nstep, DeviceReplay.gather_nstep):
        src = inspect.getsource(fn)
        for word in (".item(", ".tolist(", ".cpu(", ".numpy(", "synchronize"):
            assert word not in src, (fn.__name__, word)


def test_through_the_real_ring():
    """usv-simple behind DeviceWrappers(5): the torch shadow is the example's full-storage TorchReplay, which
    is given wr.stacked before the step and where(done, final_stack, stacked) after it."""
    import gym_usv_amd
    from gym_usv_amd.replay import DeviceReplay, discount_table
    from gym_usv_amd.wrappers import DeviceWrappers
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    from sac_torch import TorchReplay
    n, k, R, steps, n_steps, gamma = 256, 5, 7, 30, 3, 0.99
    env = gym_usv_amd.make_vec("usv-simple", n, seed=3, max_episode_steps=11, copy=False)
    D, W = env.obs_dim, 5 * env.obs_dim
    wr = DeviceWrappers(n, D, k, env.device, env.reward.dtype)
    rb = DeviceReplay(n, R * n, W, env.act_dim, env.device, env.reward.dtype, n_stack=k, n_steps=n_steps, gamma=gamma)
    d = env.device
    shadow, table = TorchReplay(n, R * n, W, env.act_dim, d), discount_table(gamma, n_steps)
    obs, _ = env.reset(seed=3)
    wr.reset(obs)
    gen = torch.Generator(device=d).manual_seed(1)
    lo = torch.as_tensor(env.single_action_space.low, device=d)
    hi = torch.as_tensor(env.single_action_space.high, device=d)
    seen_trunc = seen_term = cut = whole = 0
    for c in range(steps):
        a = lo + (hi - lo) * torch.rand((n, env.act_dim), device=d, generator=gen)
        for buf in (rb, shadow):
            buf.put_obs(wr.stacked, a)
        obs, rew, term, trunc, info = env.step(a)
        stacked, final_stack, _ = wr.step(obs, rew, info["_final_obs"], info["final_obs"])
        for buf in (rb, shadow):
            buf.put_step(rew, term, trunc, stacked, final_stack)
        seen_trunc += int((trunc.bool() & ~term.bool()).sum())
        seen_term += int(term.bool().sum())
        if c in (0, R - 1, R, steps - 1):
            M = rb.size * n
            i = torch.cat((torch.arange(M, device=d), torch.randperm(M, device=d, generator=gen)))
            got, want = rb.gather_nstep(i), shadow.gather_nstep(i, n_steps, table)
            for name, t, w in zip(FIELDS, got, want):
                assert same(t, w), (name, c)
            full = float(np.float32(gamma ** n_steps))
            cut += int((got.discounts != full).sum())
            whole += int((got.discounts == full).sum())
    assert seen_trunc > 0 and seen_term > 0             # TimeLimit truncations and collisions both occurred
    assert cut > 0 and whole > 0                        # runs that were cut and runs of all three steps
    assert rb.full and rb.bad_indices() == 0
    env.close()


def test_sac_example_with_n_steps():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    from sac_torch import train
    hist = train("usv-simple", envs=256, steps=24, batch_size=256, learning_starts=8, train_freq=8, gradient_steps=4,
                 buffer_size=256 * 10, seed=0, log=print, device_replay=True, check_replay=True, n_steps=3,
                 max_episode_steps=11)
    assert len(hist) == 2 and hist[-1]["minibatches_checked"] == 8
    for h in hist:
        for key in ("actor_loss", "critic_loss", "ent_coef"):
            assert math.isfinite(h[key]), h
