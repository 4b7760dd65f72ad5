"""The device replay buffer on the GPU (gym_usv_amd.replay.DeviceReplay: usv_replay_put_obs / _put_step /
_gather) against full storage (tests/replay_ref.py, SB3's ReplayBuffer restated): the same scripted steps
go into both, and every gathered output must equal the reference's.  Every comparison is bitwise (tensors
compared as integers): no tolerance."""
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

import replay_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

A = 2
BATCHES = (1, 3, 4, 5, 257)             # the samples-per-wave tail, a full wave of four, more than a block
FIELDS = ("observations", "actions", "next_observations", "dones", "rewards")


def dev():
    return torch.device("cuda", 0)


def bits_t(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and torch.equal(bits_t(a), bits_t(b))


def off_by_one_float(t):
    """A contiguous copy of float32 `t` whose base is one float past its allocation."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.flatten()
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


def make(n, R, k, D, keep, f64=False, misaligned=False):
    from gym_usv_amd.replay import DeviceReplay
    rb = DeviceReplay(n, R * n, k * D, A, dev(), torch.float64 if f64 else torch.float32, n_stack=k,
                      clear_keeps_sign=keep)
    assert rb.rows == R and rb.frames.shape == (n, R + k - 1, D) and rb.next_frame.shape == (R, n, D)
    if misaligned:
        for name in ("frames", "next_frame", "act", "rew"):
            setattr(rb, name, off_by_one_float(getattr(rb, name)))
        rb._bind()
    return rb


def upload(sc):
    return {key: torch.from_numpy(np.ascontiguousarray(v)).to(dev()) for key, v in sc.items()}


def feed(rb, g, lo, hi, misaligned=False, wide=0):
    """Scripted steps lo .. hi - 1 into `rb`."""
    n, W = rb.n, rb.w
    give = off_by_one_float if misaligned else (lambda t: t)

    def window(t):
        if not wide:
            return give(g["windows"][t])
        buf = torch.full((n, W + wide), float("nan"), device=dev())        # a row stride of W + wide
        buf[:, 1:W + 1] = g["windows"][t]
        return buf[:, 1:W + 1]

    for t in range(lo, hi):
        rb.put_obs(window(t), give(g["act"][t]))
        rb.put_step(g["rew"][t] if g["rew"].dtype == torch.float64 else give(g["rew"][t]), g["term"][t], g["trunc"][t],
                    window(t + 1), give(g["final_stack"][t]))


def compare(rb, ref, seed=0, misaligned=False):
    """Every valid index (in order and permuted) and every batch size of BATCHES through `rb.gather`."""
    from gym_usv_amd.replay import ReplaySamples
    assert (rb.size, rb.pos, rb.full) == (ref.size, ref.pos, ref.full)
    M = ref.size * ref.n
    gen = torch.Generator().manual_seed(seed)
    sets = [torch.cat((torch.arange(M), torch.randperm(M, generator=gen)))]
    sets += [torch.randint(0, M, (B,), generator=gen) for B in BATCHES]
    for i in sets:
        want = ref.get(i.numpy())
        out = None
        if misaligned:
            out = ReplaySamples(*(off_by_one_float(torch.zeros(w.shape, device=dev())) for w in want))
        got = rb.gather(i.to(dev()), out=out)
        assert isinstance(got, ReplaySamples) and got._fields == FIELDS
        for name, t, w in zip(FIELDS, got, want):
            assert same(t, torch.from_numpy(w).to(dev())), (name, i.numel(), rb.n, rb.n_stack, rb.d, rb.rows, rb.size)


def check(n, k, D, R, keep, pattern="random", f64=False, misaligned=False, wide=0):
    counts = P.counts_of(R)
    sc = P.script(n, max(counts), k, D, A, pattern, keep, f64=f64)
    refs = P.run(sc, n, R, k, D, A, counts)
    rb, g = make(n, R, k, D, keep, f64, misaligned), upload(sc)
    at = 0
    for c in counts:
        feed(rb, g, at, c, misaligned, wide)
        at = c
        compare(rb, refs[c], seed=n + c, misaligned=misaligned)
    assert rb.bad_indices() == 0
    return rb, refs[counts[-1]], sc


SHAPES = [(k, D, R) for k in (1, 2, 5) for D in (1, 3, 4, 143) for R in (1, 2, k + 2)]


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("n", (1, 65, 257))
def test_scripted_stores_equal_full_storage(n, keep):
    for i, (k, D, R) in enumerate(SHAPES):
        check(n, k, D, R, keep, P.PATTERNS[(i + n) % len(P.PATTERNS)], f64=(i + n) % 2 == 1)


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("n", (1, 65, 257))
def test_misaligned_bases_and_a_strided_source(n, keep):
    for k, D, R in ((5, 4, 7), (5, 6, 2), (5, 143, 3), (2, 3, 4), (1, 143, 2)):
        check(n, k, D, R, keep, "random", misaligned=True)    # every base one float past its allocation
        check(n, k, D, R, keep, "double", wide=5)             # source windows with row stride W + 5


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_done_patterns(pattern):
    for keep in (False, True):
        rb, _, _ = check(65, 5, 6, 7, keep, pattern)
        assert rb._count == 18


@pytest.mark.parametrize("normalize", (None, {}))
def test_through_the_real_ring(normalize):
    """usv-simple behind DeviceWrappers(5): the torch shadow holds wr.stacked.clone() taken before the step
    and where(done, final_stack, stacked) taken after it."""
    import gym_usv_amd
    from gym_usv_amd.replay import DeviceReplay
    from gym_usv_amd.wrappers import DeviceWrappers
    n, k, R, steps = 256, 5, 7, 30
    env = gym_usv_amd.make_vec("usv-simple", n, seed=3, max_episode_steps=11, copy=False)
    D, W = env.obs_dim, 5 * env.obs_dim
    wr = DeviceWrappers(n, D, k, env.device, env.reward.dtype, normalize=normalize)
    rb = DeviceReplay(n, R * n, W, env.act_dim, env.device, torch.float32 if normalize is not None else env.reward.dtype,
                      n_stack=k)
    d = env.device
    s_obs, s_next = torch.zeros((R, n, W), device=d), torch.zeros((R, n, W), device=d)
    s_act, s_rew = torch.zeros((R, n, env.act_dim), device=d), torch.zeros((R, n), device=d)
    s_done, s_to = torch.zeros((R, n), device=d), torch.zeros((R, n), device=d)
    obs, _ = env.reset(seed=3)
    wr.reset(obs)
    gen = torch.Generator(device=d).manual_seed(1)
    lo = torch.as_tensor(env.single_action_space.low, device=d)
    hi = torch.as_tensor(env.single_action_space.high, device=d)
    seen_trunc = seen_term = 0
    for c in range(steps):
        a = lo + (hi - lo) * torch.rand((n, env.act_dim), device=d, generator=gen)
        p = c % R
        s_obs[p], s_act[p] = wr.stacked.clone(), a
        rb.put_obs(wr.stacked, a)
        obs, rew, term, trunc, info = env.step(a)
        done = info["_final_obs"].bool()
        stacked, final_stack, _ = wr.step(obs, rew, info["_final_obs"], info["final_obs"])
        r = wr.norm_rew if normalize is not None else rew
        rb.put_step(r, term, trunc, stacked, final_stack)
        s_next[p] = torch.where(done[:, None], final_stack, stacked)
        s_rew[p], s_done[p] = r.float(), done.float()
        s_to[p] = (trunc.bool() & ~term.bool()).float()
        seen_trunc += int((trunc.bool() & ~term.bool()).sum())
        seen_term += int(term.bool().sum())
        if c in (0, R - 1, R, steps - 1):
            M = rb.size * n
            i = torch.cat((torch.arange(M, device=d), torch.randperm(M, device=d, generator=gen)))
            got = rb.gather(i)
            assert same(got.observations, s_obs.reshape(-1, W)[i]), c
            assert same(got.next_observations, s_next.reshape(-1, W)[i]), c
            assert same(got.actions, s_act.reshape(-1, env.act_dim)[i]), c
            assert same(got.rewards, s_rew.reshape(-1, 1)[i]), c
            assert same(got.dones, (s_done * (1 - s_to)).reshape(-1, 1)[i]), c
    assert seen_trunc > 0 and seen_term > 0             # TimeLimit truncations and collisions both occurred
    assert rb.full and rb.bad_indices() == 0
    env.close()


def test_bad_and_out_of_range_indices():
    n, k, D, R = 65, 5, 6, 7
    sc = P.script(n, R + 1, k, D, A, "double", True)
    refs = P.run(sc, n, R, k, D, A, [3, R + 1])
    rb, g = make(n, R, k, D, True), upload(sc)
    raw = [3, -1, 4, 3 * n, 3 * n - 1, 2 ** 40, 0, -2 ** 63, -n, 5 * n + 2, R * n, R * n - 1]
    idx = torch.tensor(raw, dtype=torch.int64, device=dev())
    expect, at = 0, 0
    for count in (3, R + 1):
        feed(rb, g, at, count)
        at = count
        ok = (idx >= 0) & (idx < min(count, R) * n)       # 5 n + 2 and R n - 1 are valid only once the ring is full
        got = rb.gather(idx)                              # no error status: the call returns
        expect += int((~ok).sum())
        assert rb.bad_indices() == expect
        for t, w in zip(got, refs[count].get(idx[ok].cpu().numpy())):
            assert torch.isnan(t[~ok]).all()
            assert same(t[ok], torch.from_numpy(w).to(dev()))
    rb.gather(idx[1:2])                                   # B = 1, bad
    assert rb.bad_indices() == expect + 1


def test_sample_stays_in_range_and_makes_no_host_sync():
    from gym_usv_amd.replay import DeviceReplay
    n, k, D, R = 65, 2, 3, 5
    sc = P.script(n, R + 2, k, D, A)
    rb, g = make(n, R, k, D, False), upload(sc)
    with pytest.raises(RuntimeError):
        rb.sample(4)                                      # empty
    for count in (2, R + 2):
        feed(rb, g, rb._count, count)
        # every stored action row is unique: the sampled actions say which (slot, env) pairs were drawn
        flat = rb.act.reshape(-1, A)[:rb.size * n]
        mb = rb.sample(2048, generator=torch.Generator(device=dev()).manual_seed(count))
        assert mb.observations.shape == (2048, k * D) and mb.dones.shape == (2048, 1)
        assert not torch.isnan(mb.actions).any() and rb.bad_indices() == 0
        hit = (mb.actions[:, None, :] == flat[None, :, :]).all(-1)
        assert hit.any(1).all()                           # every sample is a valid pair
        assert hit.any(0).float().mean() > 0.9            # and the draw covers the valid range
    for fn in (DeviceReplay.sample, DeviceReplay.gather):
        src = inspect.getsource(fn)
        for word in (".item(", ".tolist(", ".cpu(", ".numpy(", "synchronize"):
            assert word not in src, (fn.__name__, word)


def test_gather_between_put_obs_and_put_step_raises():
    n, k, D, R = 65, 5, 6, 3
    sc = P.script(n, 3, k, D, A)
    rb, g = make(n, R, k, D, False), upload(sc)
    feed(rb, g, 0, 2)
    idx = torch.arange(4, device=dev())
    rb.gather(idx)
    rb.put_obs(g["windows"][2], g["act"][2])
    with pytest.raises(RuntimeError):
        rb.gather(idx)
    with pytest.raises(RuntimeError):
        rb.sample(4)
    with pytest.raises(RuntimeError):
        rb.put_obs(g["windows"][2], g["act"][2])
    rb.put_step(g["rew"][2], g["term"][2], g["trunc"][2], g["windows"][3], g["final_stack"][2])
    with pytest.raises(RuntimeError):
        rb.put_step(g["rew"][2], g["term"][2], g["trunc"][2], g["windows"][3], g["final_stack"][2])
    compare(rb, P.run(sc, n, R, k, D, A, [3])[3])


@pytest.mark.parametrize("keep", (False, True))
def test_clear_then_reuse_equals_a_fresh_object(keep):
    n, k, D, R = 65, 5, 6, 4
    first = P.script(n, 6, k, D, A, "random", keep, seed=1)
    second = P.script(n, 9, k, D, A, "double", keep, seed=2)
    used, fresh = make(n, R, k, D, keep), make(n, R, k, D, keep)
    feed(used, upload(first), 0, 6)
    used.clear()
    assert (used.size, used.pos, used.full) == (0, 0, False)
    g = upload(second)
    feed(used, g, 0, 9)
    feed(fresh, g, 0, 9)
    ref = P.run(second, n, R, k, D, A, [9])[9]
    compare(used, ref)
    compare(fresh, ref)
    i = torch.arange(R * n, device=dev())
    for a, b in zip(used.gather(i), fresh.gather(i)):
        assert same(a, b)


def test_replay_keeps_one_frame_per_transition():
    from gym_usv_amd.replay import DeviceReplay
    n, k, D = 64, 5, 143
    rb = DeviceReplay(n, 32 * n + 5, k * D, A, dev(), n_stack=k)
    assert rb.rows == 32 and rb.frames.numel() == n * 36 * D and rb.next_frame.numel() == 32 * n * D
    full = 2 * 32 * n * k * D * 4
    assert rb.nbytes() < full / (k - 0.5)


def test_sac_example():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    from sac_torch import train
    hist = train("usv-simple", envs=256, steps=40, batch_size=256, learning_starts=8, train_freq=8, gradient_steps=8,
                 buffer_size=256 * 10, seed=0, log=print, device_replay=True, check_replay=True)
    assert len(hist) == 4 and hist[-1]["env_steps"] == 40 * 256           # every env step is accounted for
    assert sum(h["gradient_steps"] for h in hist) == 32 and hist[-1]["minibatches_checked"] == 32
    for h in hist:
        for key in ("actor_loss", "critic_loss", "ent_coef"):
            assert math.isfinite(h[key]), h
