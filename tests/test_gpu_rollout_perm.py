"""The graph-capturable minibatch sampler on the GPU (gym_usv_amd.rollout.RolloutSampler: usv_rollout_gather_perm):
its indices against tests/rollout_perm_ref.py's restatement, its outputs against ``DeviceRollout.gather`` at those
indices, the device cursor, and replays of a recorded ``next()`` and of a recorded PPO minibatch step against the same
calls made eagerly.  Every comparison is bitwise (tensors compared as integers): no tolerance."""
import functools

import numpy as np
import pytest
import torch

import rollout_frames_ref as F
import rollout_perm_ref as P
from test_gpu_rollout_frames import A, bits_t, dev, feed, make, same

pytestmark = pytest.mark.gpu

K = 5
# (N, T, B): M = 6; M = 35, no power of two, so positions walk; four waves' worth; M above 2^16, more than one block
SHAPES = ((3, 2, 1), (3, 2, 2), (3, 2, 3), (3, 2, 6), (5, 7, 5), (5, 7, 7), (64, 8, 128), (40_000, 2, 1000))
SEED = 0x0123456789ABCDEF


def frame_width(n):
    return 143 if n == 64 else 3


@functools.lru_cache(maxsize=None)
def rollout(n, T, frames):
    """A filled rollout with episode starts inside the window, so that frame mode's live masks matter.  Shared: no
    test writes to it."""
    D = frame_width(n)
    sc = F.script(n, T, K, D, A, "random", False)
    ro = make(n, T, K, D, False, frames)
    feed(ro, sc)
    assert bool(ro.start[1:T].any())
    return ro


def all_same(pairs):
    """One device flag for many bitwise comparisons: a single sync."""
    ok = torch.ones((), dtype=torch.bool, device=dev())
    for a, b in pairs:
        assert a.shape == b.shape and a.dtype == b.dtype
        ok = ok & (bits_t(a) == bits_t(b)).all()
    return bool(ok)


@pytest.mark.parametrize("frames", (False, True))
@pytest.mark.parametrize("n,T,B", SHAPES)
def test_two_epochs_equal_the_restatement_and_gather(n, T, B, frames):
    ro = rollout(n, T, frames)
    M = n * T
    smp = ro.sampler(B, SEED)
    assert smp.batches_per_epoch == M // B and smp.state_dict() == {"seed": SEED, "epoch": 0, "batch": 0}
    every = 1 if smp.batches_per_epoch <= 8 else 16
    pairs, calls, cursor = [], 0, (0, 0)
    for epoch in range(2):
        perm = P.permutation(SEED, epoch, M)
        assert (np.sort(perm) == np.arange(M)).all()
        seen = []
        for b in range(M // B):
            idx = torch.empty(B, dtype=torch.int64, device=dev())
            mb = smp.next(idx_out=idx)
            seen.append(idx)
            pairs += list(zip(mb, ro.gather(idx)))
            cursor = P.cursor_ticked(*cursor, M // B)
            calls += 1
            if calls % every == 0:
                sd = smp.state_dict()
                assert (sd["epoch"], sd["batch"]) == cursor == (smp.epoch, smp.batch)
        assert np.array_equal(torch.cat(seen).cpu().numpy(), perm), epoch     # index for index the restatement
    assert all_same(pairs)                                  # every output, bit for bit ro.gather(idx_out)
    assert (smp.epoch, smp.batch) == (2, 0) and ro.bad_indices() == 0


@pytest.mark.parametrize("frames", (False, True))
def test_outputs_given_by_the_caller_and_no_idx_out(frames):
    from gym_usv_amd.rollout import RolloutSamples
    n, T, B = 5, 7, 7
    ro = rollout(n, T, frames)
    a, b = ro.sampler(B, 3), ro.sampler(B, 3)
    out = RolloutSamples(*(torch.zeros(s, device=dev()) for s in ((B, ro.w), (B, A), (B,), (B,), (B,), (B,))))
    got = a.next(out=out)
    assert all(x is y for x, y in zip(got, out))
    idx = torch.empty(B, dtype=torch.int64, device=dev())
    assert all_same(zip(out, b.next(idx_out=idx)))
    assert np.array_equal(idx.cpu().numpy(), P.minibatch(3, 0, 0, n * T, B))
    with pytest.raises(ValueError):
        a.next(idx_out=idx[:3])
    with pytest.raises(ValueError):
        a.next(idx_out=idx.to(torch.int32))
    with pytest.raises(ValueError):
        ro.sampler(4, 3)                                    # 4 does not divide 35
    assert a.batch == 1                                     # a refused call moved nothing


def test_setting_the_cursor_and_the_wrap_of_the_epoch():
    n, T, B = 5, 7, 5
    ro = rollout(n, T, True)
    smp = ro.sampler(B, SEED)
    last = smp.batches_per_epoch - 1
    smp.epoch, smp.batch = 0xFFFFFFFF, last
    assert (smp.epoch, smp.batch) == (0xFFFFFFFF, last)
    idx = torch.empty(B, dtype=torch.int64, device=dev())
    smp.next(idx_out=idx)
    assert np.array_equal(idx.cpu().numpy(), P.minibatch(SEED, 0xFFFFFFFF, last, n * T, B))
    assert (smp.epoch, smp.batch) == (0, 0)                 # one call wraps both
    with pytest.raises(ValueError):
        smp.batch = last + 1


def test_a_checkpoint_continues_the_sequence():
    n, T, B = 5, 7, 5
    ro = rollout(n, T, False)
    a = ro.sampler(B, SEED)
    for _ in range(9):                                      # into the second epoch
        a.next()
    sd = a.state_dict()
    assert sd == {"seed": SEED, "epoch": 1, "batch": 2}
    b = ro.sampler(B, 1)
    b.load_state_dict(sd)
    for _ in range(7):
        ia, ib = (torch.empty(B, dtype=torch.int64, device=dev()) for _ in range(2))
        assert all_same(list(zip(a.next(idx_out=ia), b.next(idx_out=ib))) + [(ia, ib)])
    assert a.state_dict() == b.state_dict()


@pytest.mark.parametrize("frames", (False, True))
@pytest.mark.parametrize("n,T,B", ((5, 7, 7), (64, 8, 128)))
def test_a_recorded_next_reads_another_minibatch_at_every_replay(n, T, B, frames):
    from gym_usv_amd import capture_step
    from gym_usv_amd.rollout import RolloutSamples
    ro = rollout(n, T, frames)
    smp, eager = ro.sampler(B, SEED), ro.sampler(B, SEED)
    static = RolloutSamples(*(torch.zeros(s, device=dev()) for s in ((B, ro.w), (B, A), (B,), (B,), (B,), (B,))))
    static_idx = torch.zeros(B, dtype=torch.int64, device=dev())
    captured = capture_step(lambda: smp.next(out=static, idx_out=static_idx), warmup=1)     # two calls
    for _ in range(2):
        eager.next()
    seen = []
    for j in range(smp.batches_per_epoch + 2):              # through an epoch boundary
        captured.replay()
        idx = torch.empty(B, dtype=torch.int64, device=dev())
        want = eager.next(idx_out=idx)
        assert all_same(list(zip(static, want)) + [(static_idx, idx)]), j
        seen.append(static_idx.cpu().numpy().copy())
    calls = 2 + smp.batches_per_epoch + 2
    assert smp.state_dict() == eager.state_dict()
    assert (smp.epoch, smp.batch) == divmod(calls, smp.batches_per_epoch) and smp.epoch >= 1
    assert not np.array_equal(seen[0], seen[1])             # not the recorded minibatch over and over
    with torch.cuda.graph(torch.cuda.CUDAGraph()):          # a cursor write under capture would be recorded, not made
        static_idx.add_(0)
        with pytest.raises(RuntimeError, match="captur"):
            smp.epoch = 3
        with pytest.raises(RuntimeError, match="captur"):
            smp.batch = 0


def test_a_recorded_minibatch_step_equals_the_eager_calls():
    """sampler.next, a two-layer policy and value, DeviceSDE.evaluate, DevicePPOLoss.loss, the backward and
    DeviceAdam(capturable=True).step() recorded once: five replays against five eager calls."""
    from gym_usv_amd import DeviceAdam, DevicePPOLoss, DeviceSDE, capture_step
    from gym_usv_amd.rollout import RolloutSamples
    n, T, B, L = 64, 8, 128, 8
    ro = rollout(n, T, True)

    def build():
        torch.manual_seed(11)
        body, mu, vf = torch.nn.Linear(ro.w, L), torch.nn.Linear(L, A), torch.nn.Linear(L, 1)
        for m in (body, mu, vf):
            m.to(dev())
        log_std = torch.nn.Parameter(torch.zeros(L, A, device=dev()))
        params = [*body.parameters(), *mu.parameters(), *vf.parameters(), log_std]
        opt = DeviceAdam(params, lr=1e-3, max_grad_norm=0.5, capturable=True)
        head = DeviceSDE(B, L, A, dev(), 1, [-1.0] * A, [1.0] * A)
        pl, smp = DevicePPOLoss(dev()), ro.sampler(B, SEED)
        static = RolloutSamples(*(torch.zeros(s, device=dev()) for s in ((B, ro.w), (B, A), (B,), (B,), (B,), (B,))))
        last = []

        def fn():
            mb = smp.next(out=static)
            lat = torch.relu(body(mb.observations))
            logp = head.evaluate(mu(lat), lat.detach(), log_std.exp(), mb.actions).log_prob
            out = pl.loss(logp, mb.old_log_prob, mb.advantages, vf(lat).squeeze(-1), mb.returns, clip_range=0.2,
                          vf_coef=0.5, ent_coef=0.01)
            opt.zero_grad()                                 # inside: the recorded backward allocates from the graph's pool
            out.loss.backward()
            opt.step()
            last[:] = [torch.stack(tuple(out)).detach(), pl.moments]      # the autograd graph goes
            return last[0], last[1]

        def state(out):
            stats, moments = out if out is not None else last
            return [p.detach() for p in params] + [opt.exp_avg, opt.exp_avg_sq, stats, moments]

        return fn, state, opt, smp, pl

    fn, state, opt, smp, pl = build()
    captured = capture_step(fn, warmup=3)                   # four calls
    efn, estate, eopt, esmp, _ = build()
    for _ in range(4):
        efn()
    stats = []
    for j in range(5):
        captured.replay()
        efn()
        got, want = state(captured.out), estate(None)
        assert all_same(zip(got, want)), j
        stats.append(got[-2].cpu().numpy().copy())
        assert np.isfinite(stats[-1]).all() and bool(torch.isfinite(got[0]).all())
    assert opt.step_count == 9 == eopt.step_count and smp.state_dict() == esmp.state_dict()
    assert smp.state_dict()["epoch"] == 2 and not np.array_equal(stats[0], stats[1])
    assert int(pl._scratch[:1].view(torch.int32)) == 0      # the reduction's ticket word is back at zero
