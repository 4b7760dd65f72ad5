"""The device rollout buffer on the GPU (gym_usv_amd.rollout.DeviceRollout: usv_rollout_put_obs /
_put_step / _gae) against SB3's RolloutBuffer restated in NumPy float32 (tests/rollout_ref.py), driven with
the same scripted inputs.  Every comparison is bitwise (arrays compared as integers): no tolerance."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import rollout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.99, 0.95
NS = (1, 63, 64, 65, 257)
THREE = 2 * 256 + 70                                    # three chunks of the slot scan, a ragged last one
FLOATS = ("obs", "act", "rew", "val", "logp", "adv", "ret")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def off_by_one_float(t):
    """A contiguous copy of float32 `t` whose base is one float past its allocation."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.flatten()
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


def device_run(sc, n, T, W, A, cap=None, misaligned=False, ro=None, term_val=None, wide=0):
    """The script through a DeviceRollout on the current stream; returns (ro, term_val used).  `wide`:
    the obs rows come from a buffer whose row stride is W + wide floats."""
    from gym_usv_amd.rollout import DeviceRollout
    dev = torch.device("cuda", 0)
    rdt = torch.float64 if sc["rew"].dtype == np.float64 else torch.float32
    if ro is None:
        ro = DeviceRollout(n, T, W, A, dev, rdt, term_cap=cap)
        if misaligned:
            for name in FLOATS + ("term_obs",):
                setattr(ro, name, off_by_one_float(getattr(ro, name)))
            ro._bind()
    give = off_by_one_float if misaligned else (lambda t: t)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in sc.items()}
    for t in range(T):
        obs = give(d["obs"][t])
        if wide:
            buf = torch.full((n, W + wide), float("nan"), device=dev)
            buf[:, 1:W + 1] = d["obs"][t]
            obs = buf[:, 1:W + 1]
        ro.put_obs(t, obs, give(d["act"][t]), give(d["val"][t]), give(d["logp"][t]))
        ro.put_step(t, d["rew"][t] if rdt == torch.float64 else give(d["rew"][t]), d["term"][t], d["trunc"][t],
                    give(d["final"][t]))
    if term_val is None:
        stored, _ = ro.counts()
        term_val = R.value_of(ro.term_obs.cpu().numpy())
        term_val[stored:] = np.nan                      # unreferenced slots must not reach an output
    ro.gae(d["last_val"], torch.from_numpy(term_val).to(dev), GAMMA, LAM)
    return ro, term_val


def compare(ro, ref, key):
    assert ro.counts() == (ref.stored, ref.overflow), key
    for name in FLOATS + ("start", "term_slot"):
        got = getattr(ro, name).cpu().numpy()
        assert (bits(got) == bits(getattr(ref, name))).all(), (key, name)
    s = ref.stored
    assert (bits(ro.term_obs[:s].cpu().numpy()) == bits(ref.term_obs[:s])).all(), (key, "term_obs")
    assert np.isfinite(ro.adv.cpu().numpy()).all() and np.isfinite(ro.ret.cpu().numpy()).all(), key


def check(n, T, W, A, pattern="random", cap=None, f64=False, misaligned=False, wide=0, force=None):
    sc = R.script(n, T, W, A, pattern, f64=f64)
    if force is not None:                               # these envs truncate (and do not terminate) in every step
        sc["trunc"][:, force] = True
        sc["term"][:, force] = False
    ref = R.run(sc, n, T, W, A, term_cap=cap, gamma=GAMMA, gae_lambda=LAM)
    ro, _ = device_run(sc, n, T, W, A, cap=cap, misaligned=misaligned, wide=wide)
    compare(ro, ref, f"n {n} T {T} W {W} A {A} {pattern} cap {cap} f64 {f64} misaligned {misaligned}")
    return ro, ref, sc


@pytest.mark.parametrize("n", NS)
def test_scripted_rollouts_match_rollout_buffer_bit_for_bit(n):
    for T, W, A in ((1, 1, 1), (2, 4, 2), (5, 6, 1), (2, 715, 2)):
        check(n, T, W, A)
    check(n, 5, 6, 2, misaligned=True)                  # every base one float past its allocation
    check(n, 2, 715, 1, misaligned=True)
    check(n, 2, 7, 1, wide=5)                           # a strided source (row stride W + 5)
    check(n, 2, 3, 1, wide=2)


def test_slot_prefix_over_three_chunks():
    """Truncated envs at the first and the last env of each of three chunks, among random ones."""
    edges = [0, 255, 256, 511, 512, THREE - 1]
    _, ref, _ = check(THREE, 5, 6, 2, force=edges)
    assert (ref.term_slot[:, edges] >= 0).all()
    check(THREE, 2, 715, 2, "none", force=edges)


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_done_patterns(pattern):
    _, ref, _ = check(65, 5, 6, 2, pattern)
    if pattern == "all_trunc":
        assert ref.stored == 65 and (ref.term_slot[1] == np.arange(65)).all()   # n slots at once
    if pattern == "both":
        assert ref.stored == 0 and ref.start[2].all()
    check(257, 2, 715, 1, pattern)


def test_f64_rewards():
    for n in (1, 65, 257):
        check(n, 5, 6, 2, f64=True)


def test_side_stream():
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        check(257, 5, 6, 2)
        check(65, 2, 715, 2, "all_trunc")
    s.synchronize()


def test_overflow_with_three_slots():
    for pattern in ("all_trunc", "random", "consecutive"):
        ro, ref, sc = check(65, 5, 6, 2, pattern, cap=3)
        t, e = np.nonzero(sc["trunc"] & ~sc["term"])   # the pairs in (t, env) order
        slots = ro.term_slot.cpu().numpy()
        assert [int(slots[t[i], e[i]]) for i in range(3)] == [0, 1, 2], pattern
        assert (slots[t[3:], e[3:]] == -1).all() and (slots >= 0).sum() == 3, pattern
        assert ro.counts() == (3, len(t) - 3), pattern


def test_unreferenced_term_val_is_never_read():
    """term_val = NaN wherever no pair holds the slot, and an all-NaN term_val with no pair at all."""
    n, T, W, A = 65, 5, 6, 2
    sc = R.script(n, T, W, A, "both")
    ref = R.run(sc, n, T, W, A, gamma=GAMMA, gae_lambda=LAM)
    ro, _ = device_run(sc, n, T, W, A, term_val=np.full(2 * n, np.nan, np.float32))
    compare(ro, ref, "all-NaN term_val")


def test_consecutive_rollouts_carry_episode_starts():
    n, T, W, A = 65, 5, 6, 2
    a, b = R.script(n, T, W, A, "random", seed=1), R.script(n, T, W, A, "random", seed=2)
    ref = R.run(a, n, T, W, A, gamma=GAMMA, gae_lambda=LAM)
    ro, _ = device_run(a, n, T, W, A)
    compare(ro, ref, "first rollout")
    assert (ref.start[0] == ref.start[T]).all() and not ref.start[0].all()
    ref = R.run(b, n, T, W, A, gamma=GAMMA, gae_lambda=LAM, ro=ref)
    ro, _ = device_run(b, n, T, W, A, ro=ro)
    compare(ro, ref, "second rollout")


def test_gae_twice_and_the_script_twice_give_the_same_bits():
    n, T, W, A = 257, 5, 6, 2
    sc = R.script(n, T, W, A, "random")
    ro, tv = device_run(sc, n, T, W, A)
    first = {k: getattr(ro, k).clone() for k in FLOATS + ("start", "term_slot", "term_obs")}
    d = torch.device("cuda", 0)
    ro.gae(torch.from_numpy(sc["last_val"]).to(d), torch.from_numpy(tv).to(d), GAMMA, LAM)
    for k, v in first.items():
        assert torch.equal(bits_t(getattr(ro, k)), bits_t(v)), ("gae twice", k)
    again, _ = device_run(sc, n, T, W, A)
    for k, v in first.items():
        assert torch.equal(bits_t(getattr(again, k)), bits_t(v)), ("script twice", k)


def bits_t(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 1: torch.uint8}[t.element_size()])


def test_ring_window_is_stored_in_place():
    """The real source: DeviceWrappers(k = 5, D = 143).stacked at consecutive j, so that every window
    offset occurs; obs[t] must equal the window seen at action time."""
    from gym_usv_amd.rollout import DeviceRollout
    from gym_usv_amd.wrappers import DeviceWrappers
    dev = torch.device("cuda", 0)
    n, k, D, T = 65, 5, 143, 11
    g = torch.Generator().manual_seed(5)
    frames = torch.randn((T + 1, n, D), generator=g).to(dev)
    wr = DeviceWrappers(n, D, k, dev)
    ro = DeviceRollout(n, T, k * D, 2, dev)
    wr.reset(frames[0])
    z = torch.zeros(n, device=dev)
    seen, offsets = [], set()
    for t in range(T):
        st = wr.stacked
        assert st.stride(0) > k * D and st.stride(1) == 1
        offsets.add(st.storage_offset())
        seen.append(st.clone())
        ro.put_obs(t, st, torch.zeros((n, 2), device=dev), z, z)
        wr.step(frames[t + 1], z, torch.zeros(n, dtype=torch.bool, device=dev))
    assert len(offsets) == k
    assert torch.equal(bits_t(ro.obs), bits_t(torch.stack(seen)))


def test_real_env_rollout_over_the_time_limit():
    """usv-simple, 256 envs, max_episode_steps = 3: every env truncates, also across the rollout boundary.
    The step outputs are recorded on the host and fed to the restatement."""
    import gym_usv_amd
    from gym_usv_amd.rollout import DeviceRollout
    from gym_usv_amd.wrappers import DeviceWrappers
    n, k, T = 256, 5, 8
    env = gym_usv_amd.make_vec("usv-simple", n, seed=3, copy=False, max_episode_steps=3)
    dev, D, A = env.device, env.obs_dim, env.act_dim
    W = k * D
    wr = DeviceWrappers(n, D, k, dev, env.reward.dtype)
    ro = DeviceRollout(n, T, W, A, dev, env.reward.dtype, term_cap=3 * n)   # t = 0, 3, 6 after the boundary
    ref = R.NpRollout(n, T, W, A, term_cap=3 * n)
    obs, _ = env.reset(seed=3)
    wr.reset(obs)
    g = torch.Generator().manual_seed(11)
    lo = torch.as_tensor(env.single_action_space.low, dtype=torch.float32)
    hi = torch.as_tensor(env.single_action_space.high, dtype=torch.float32)
    value = lambda rows: R.value_of(rows) * np.float32(0.01)   # noqa: E731
    bootstraps = 0
    for rollout in range(2):
        for t in range(T):
            st = wr.stacked.cpu().numpy()
            a = (lo + (hi - lo) * torch.rand((n, A), generator=g)).to(dev)
            v = torch.from_numpy(value(st)).to(dev)
            logp = torch.randn(n, generator=g).to(dev)
            ro.put_obs(t, wr.stacked, a, v, logp)
            ref.put_obs(t, st, a.cpu().numpy(), v.cpu().numpy(), logp.cpu().numpy())
            o, rew, term, trunc, info = env.step(a)
            _, final_stack, _ = wr.step(o, rew, info["_final_obs"], info["final_obs"])
            ro.put_step(t, rew, term, trunc, final_stack)
            ref.put_step(t, rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), final_stack.cpu().numpy())
        last = value(wr.stacked.cpu().numpy())
        tv = value(ro.term_obs.cpu().numpy())
        ro.gae(torch.from_numpy(last).to(dev), torch.from_numpy(tv).to(dev), GAMMA, LAM)
        ref.gae(last, tv, GAMMA, LAM)
        compare(ro, ref, f"real env, rollout {rollout}")
        bootstraps += ref.stored
        assert ref.overflow == 0 and ref.stored >= n      # every env hit the limit at least once
    assert bootstraps >= 4 * n
    env.close()


class SyncCounter:
    """Counts the calls of the Tensor methods that wait for the device, on device tensors."""
    NAMES = ("__bool__", "item", "nonzero", "cpu", "tolist")

    def __enter__(self):
        self.calls, self.saved = [], {}
        for name in self.NAMES:
            orig = getattr(torch.Tensor, name)
            self.saved[name] = orig

            def wrapped(t, *a, _orig=orig, _name=name, **kw):
                if t.is_cuda:
                    self.calls.append(_name)
                return _orig(t, *a, **kw)
            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(torch.Tensor, name, orig)


def test_fused_example_trains_and_its_rollout_never_asks_the_host():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "examples")) if p not in sys.path]
    import gym_usv_amd
    from ppo_torch import PPO, train
    hist = train("usv-simple", envs=1024, updates=2, n_steps=8, batch_size=4096, seed=0, log=print, fused=True)
    assert len(hist) == 2 and hist[-1]["env_steps"] == 2 * 8 * 1024
    for h in hist:
        for k in ("policy_loss", "value_loss", "entropy"):
            assert math.isfinite(h[k]), h
    assert sum(h["episodes"] for h in hist) > 0
    for fused in (True, False):
        env = gym_usv_amd.make_vec("usv-simple", 1024, seed=0, copy=False)
        ppo = PPO(env, n_steps=8, batch_size=4096, seed=0, fused=fused)
        with SyncCounter() as c:
            ppo.rollout()
        env.close()
        if fused:
            assert c.calls == [], c.calls
        else:
            assert c.calls, "the counter must see the default rollout's host round trips"
