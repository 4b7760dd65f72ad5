"""The fused VecNormalize on the GPU (DeviceWrappers(normalize=...): usv_wrap_step_norm / usv_wrap_reset_norm)
against SB3's RunningMeanStd / VecNormalize / StackedObservations restated in NumPy
(tests/vecnormalize_ref.py).

Two kinds of comparison:
  statistics  obs_mean, obs_var, ret_var, returns at bounds derived from the arithmetic (the reduction
              combines in another order than NumPy): mean 2 n u max|x|, variance 8 n u max|x|^2, times the
              number of updates; returns 4 T u max|returns|; u = 2^-53.  Counts are exact.
  outputs     every pushed frame, final_stack row and normalised reward is a bit-exact function of the
              statistics the device published: ((x.astype(f64) - mean) * inv).clip(-c, c).astype(f32).
"""
import numpy as np
import pytest
import torch

import vecnormalize_ref as R

pytestmark = pytest.mark.gpu

T = 8
EDGES, THREE = R.edge_sizes()
CLIP = 10.0


def dev():
    return torch.device("cuda", 0)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(u32(a), u32(b))


def host(t):
    return t.detach().cpu().numpy().copy()


def off_by_one_float(t):
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.flatten()
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


_SCRIPTS = {}


def script(n, d, density, rdt=np.float32):
    """obs [T + 1, n, d] (obs[0]: the reset obs), final [T, n, d], rew [T, n], done [T, n].  |x| <= 10 but
    for two 50-sigma outliers (they must clip); d >= 4: one constant column and one of 1.0.  density
    0 / 1: never / every step; "mix": env 0 never, env 1 every step, env 2 on consecutive steps, the
    others at random with 0.25."""
    key = (n, d, density, rdt)
    if key in _SCRIPTS:
        return _SCRIPTS[key]
    rng = np.random.default_rng(100 * n + d)
    obs = np.clip(rng.standard_normal((T + 1, n, d)) * 2.5, -10, 10).astype(np.float32)
    final = np.clip(rng.standard_normal((T, n, d)) * 2.5, -10, 10).astype(np.float32)
    if d >= 4:
        obs[:, :, d - 1] = np.float32(-3.7)
        obs[:, :, d - 2] = 1.0
    # 50 sigma, in the last step, when the statistics have settled.  The obs outlier enters the statistics
    # it is normalised with (one of n values of its batch): it clips for n >= 15, see run().  A final obs
    # enters no statistic: its outlier (another column) clips whenever env 0 is done.
    obs[T, 0, 0], final[T - 1, 0, 1] = 125.0, -125.0
    rew = rng.standard_normal((T, n))
    rew[rng.random((T, n)) < 0.05] -= 20.0                 # the collision term
    rew = rew.astype(rdt)
    if density in (0, 1):
        done = np.full((T, n), bool(density))
    else:
        done = rng.random((T, n)) < 0.25
        done[:, 0] = False
        if n > 1:
            done[:, 1] = True
        if n > 2:
            done[:, 2] = False
            done[2:5, 2] = True
    _SCRIPTS[key] = (obs, final, rew, done)
    return _SCRIPTS[key]


def make(n, d, k, rdt=torch.float32, **cfg):
    from gym_usv_amd.wrappers import DeviceWrappers
    return DeviceWrappers(n, d, k, dev(), rdt, normalize=cfg)


def published(wr):
    return host(wr.obs_mean), host(wr.obs_inv_std), float(host(wr.ret_inv_std)[0])


def check_inv(wr):
    """The published reciprocals are 1 / sqrt(var + eps) of the published variances: a correctly rounded
    square root and division, so within 2 ulp of the NumPy value."""
    for var, inv in ((wr.obs_var, wr.obs_inv_std), (wr.ret_var, wr.ret_inv_std)):
        want = 1.0 / np.sqrt(host(var) + wr.epsilon)
        assert np.all(np.abs(host(inv) - want) <= 2 * np.spacing(want))


def check_stats(wr, ref, n, updates, xmax, rmax, key):
    assert np.abs(host(wr.obs_mean) - ref.obs_rms.mean).max() <= R.mean_bound(n, updates[0], xmax), key
    assert np.abs(host(wr.obs_var) - ref.obs_rms.var).max() <= R.var_bound(n, updates[0], xmax), key
    assert float(host(wr.obs_count)[0]) == ref.obs_rms.count, key
    assert float(host(wr.ret_count)[0]) == ref.ret_rms.count, key
    assert abs(float(host(wr.ret_mean)[0]) - ref.ret_rms.mean) <= R.mean_bound(n, max(updates[1], 1), rmax), key
    assert abs(float(host(wr.ret_var)[0]) - ref.ret_rms.var) <= R.var_bound(n, max(updates[1], 1), rmax), key
    assert np.abs(host(wr.returns) - ref.returns).max() <= 4 * T * R.U * max(rmax, 1e-300), key


def run(n, d, k, density, rdt=np.float32, misaligned=False, record=None, **cfg):
    """Reset + T steps of a normalising DeviceWrappers and an unnormalised one on the same script; checks
    the statistics against the restatement and the outputs bitwise given the published statistics."""
    from gym_usv_amd.wrappers import DeviceWrappers
    obs, final, rew, done = script(n, d, density, rdt)
    tdt = torch.float32 if rdt == np.float32 else torch.float64
    wr = make(n, d, k, tdt, **cfg)
    plain = DeviceWrappers(n, d, k, dev(), tdt)
    if misaligned:
        wr.ring = off_by_one_float(wr.ring)
        wr._bind()

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
        return off_by_one_float(t) if misaligned and t.dim() == 2 else t          # the [n, d] float32 rows
    ref = R.NpVecNormalize(n, d, gamma=wr.gamma, epsilon=wr.epsilon)
    stack = R.NpFrameStack(n, d, k)
    xmax, rmax, clipped = float(np.abs(obs[0]).max()), 0.0, 0
    rec = record if record is not None else []
    st = wr.reset(up(obs[0]))
    plain.reset(up(obs[0]))
    ref.reset(obs[0])
    updates = [1, 0]
    check_stats(wr, ref, n, updates, xmax, rmax, f"n {n} d {d} k {k} reset")
    mean, inv, rinv = published(wr)
    assert same(host(st), stack.reset(R.apply(obs[0], mean, inv, CLIP)))
    for t in range(T):
        key = f"n {n} d {d} k {k} density {density} step {t}"
        stacked, fstack, episode = wr.step(up(obs[t + 1]), up(rew[t]), up(done[t]), up(final[t]))
        _, _, ep_plain = plain.step(up(obs[t + 1]), up(rew[t]), up(done[t]), up(final[t]))
        after = ref.step(obs[t + 1], rew[t], done[t])
        xmax, rmax = max(xmax, float(np.abs(obs[t + 1]).max())), max(rmax, float(np.abs(after).max()))
        updates = [updates[0] + 1, updates[1] + 1]
        check_stats(wr, ref, n, updates, xmax, rmax, key)
        check_inv(wr)
        mean, inv, rinv = published(wr)
        frame = R.apply(obs[t + 1], mean, inv, CLIP)
        want, term = stack.update(frame, done[t], R.apply(final[t], mean, inv, CLIP))
        got = host(stacked)
        assert stacked.shape == (n, k * d) and same(got, want), key
        dn = done[t]
        assert same(host(fstack)[dn], term[dn]), key
        nrew = host(wr.norm_rew)
        assert same(nrew, R.apply(rew[t], 0.0, rinv, CLIP)), key
        clipped += int((np.abs(got[:, -d:]) == CLIP).sum()) + int((np.abs(host(fstack)[dn][:, -d:]) == CLIP).sum())
        assert not host(wr.returns)[dn].any(), key
        # the Monitor sits inside VecNormalize: raw rewards
        assert same(host(episode)[dn], host(ep_plain)[dn]) and same(host(wr.ep_ret), host(plain.ep_ret)), key
        for a in ("cum_ret", "cum_len", "cum_eps", "ep_len"):
            assert torch.equal(getattr(wr, a), getattr(plain, a)), (key, a)
        rec += [got, host(fstack)[dn], nrew, host(wr.obs_mean), host(wr.obs_var), host(wr.obs_inv_std),
                host(wr.ret_mean), host(wr.ret_var), host(wr.ret_inv_std), host(wr.returns), host(wr.obs_count),
                host(wr.ret_count)]
    # the outliers did clip.  (The obs outlier at n = 15: 120 earlier values of variance 6.25 and a batch
    # of 15 with one 125 merge to a variance near 120, so it sits 11 sigma out; fewer envs dilute it less.)
    if n >= 15 or density == 1:
        assert clipped > 0
    return wr


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("d", [143, 6, 3])
@pytest.mark.parametrize("n", [1] + EDGES + [257, THREE])
def test_statistics_and_outputs(n, d, k):
    """Statistics at the derived bounds and outputs bitwise given the published statistics, for done
    scripts never / every step / mixed (never, always, consecutive, random 0.25)."""
    for density in (0, 1, "mix"):
        run(n, d, k, density)


def test_reproducible_bits():
    """The same script twice, and once on a side stream with the ring, obs and final obs one float past
    their allocations: identical bits in every statistic and output."""
    a, b, c = [], [], []
    run(THREE, 143, 5, "mix", record=a)
    run(THREE, 143, 5, "mix", record=b)
    s = torch.cuda.Stream(0)
    s.wait_stream(torch.cuda.current_stream(0))
    with torch.cuda.stream(s):
        run(THREE, 143, 5, "mix", record=c, misaligned=True)
    s.synchronize()
    assert len(a) == len(b) == len(c) == 12 * T
    for x, y, z in zip(a, b, c):
        assert same(x, y) and same(x, z)


STATS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")


def snapshot(wr, names=STATS):
    return {k: host(getattr(wr, k)) for k in names}


def test_training_off_freezes_the_statistics_and_still_normalises():
    n, d, k = 65, 143, 5
    wr = run(n, d, k, "mix")
    obs, final, rew, done = script(n, d, "mix")
    wr.training = False
    before = snapshot(wr)
    mean, inv, rinv = published(wr)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    for t in range(4):
        prev = host(wr.stacked)
        stacked, fstack, _ = wr.step(up(obs[t]), up(rew[t]), up(done[t]), up(final[t]))
        for name, v in snapshot(wr).items():
            assert same(v, before[name]), (t, name)
        assert same(host(stacked)[:, -d:], R.apply(obs[t], mean, inv, CLIP)), t
        assert same(host(wr.norm_rew), R.apply(rew[t], 0.0, rinv, CLIP)), t
        dn = done[t]
        assert same(host(fstack)[dn][:, -d:], R.apply(final[t], mean, inv, CLIP)[dn]), t
        assert same(host(fstack)[dn][:, :-d], prev[dn][:, d:]), t


def test_norm_obs_off_and_norm_reward_off():
    """norm_obs=False: the ring is bitwise the unnormalised ring (and obs_rms stays as initialised);
    norm_reward=False: norm_rew is the raw reward (and ret_rms stays as initialised)."""
    from gym_usv_amd.wrappers import DeviceWrappers
    n, d, k = 65, 143, 5
    obs, final, rew, done = script(n, d, "mix")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    a = make(n, d, k, norm_obs=False)
    b = make(n, d, k, norm_reward=False)
    plain = DeviceWrappers(n, d, k, dev())
    for w in (a, b, plain):
        w.reset(up(obs[0]))
    for t in range(T):
        args = (up(obs[t + 1]), up(rew[t]), up(done[t]), up(final[t]))
        (sa, fa, _), (sb, fb, _), (sp, fp, _) = (w.step(*args) for w in (a, b, plain))
        assert same(host(a.ring), host(plain.ring)) and same(host(fa), host(fp)), t
        assert same(host(b.norm_rew), rew[t]), t
        assert not same(host(sb), host(sp))
    assert float(a.obs_count[0]) == 1e-4 and not a.obs_mean.any() and bool((a.obs_var == 1).all())
    assert float(b.ret_count[0]) == 1e-4 and float(b.ret_var[0]) == 1.0 and not b.returns.any()
    counts = [1e-4]
    for _ in range(T + 1):
        counts.append(counts[-1] + n)
    assert float(a.ret_count[0]) == counts[T] and float(b.obs_count[0]) == counts[T + 1]


def test_state_dict_round_trip_and_masked_reset():
    n, d, k = THREE, 6, 2
    obs, final, rew, done = script(n, d, "mix")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    a = run(n, d, k, "mix")
    sd = a.state_dict()
    assert set(sd) == set(STATS) | {"returns"} and all(v.data_ptr() != getattr(a, k2).data_ptr() for k2, v in sd.items())
    b = make(n, d, k)
    b.load_state_dict(sd)
    for name in STATS + ("returns",):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # masked reset: the masked rows restart with the current statistics, nothing else moves
    mask = torch.from_numpy(np.random.default_rng(3).random(n) < 0.5).to(dev())
    a.returns += 1.5
    before, ring0, ret0 = snapshot(a), host(a.stacked), host(a.returns)
    mean, inv, _ = published(a)
    st = host(a.reset(up(obs[3]), mask))
    m = host(mask)
    for name, v in snapshot(a).items():
        assert same(v, before[name]), name
    want = np.zeros((n, k * d), np.float32)
    want[:, -d:] = R.apply(obs[3], mean, inv, CLIP)
    assert same(st[m], want[m]) and same(st[~m], ring0[~m])
    assert not host(a.returns)[m].any() and same(host(a.returns)[~m], ret0[~m])
    # both go on identically from the same statistics (b: a full reset without training = no update)
    a.training = b.training = False
    a.reset(up(obs[0]))
    b.reset(up(obs[0]))
    for t in range(3):
        args = (up(obs[t + 1]), up(rew[t]), up(done[t]), up(final[t]))
        (sa, _, _), (sb, _, _) = a.step(*args), b.step(*args)
        assert same(host(sa), host(sb)) and same(host(a.norm_rew), host(b.norm_rew)), t
    x = up(obs[2])
    # the cold helpers: the same reciprocal formula
    inv_o, inv_r = host(1.0 / torch.sqrt(a.obs_var + a.epsilon)), host(1.0 / torch.sqrt(a.ret_var + a.epsilon))
    y = host(a.normalize_obs(x))
    assert same(y, R.apply(obs[2], host(a.obs_mean), inv_o, CLIP))
    ok = np.abs(y) < CLIP
    assert np.allclose(host(a.unnormalize_obs(a.normalize_obs(x)))[ok], obs[2][ok], rtol=1e-5, atol=1e-4)
    r = up(rew[0])
    assert same(host(a.normalize_reward(r)), R.apply(rew[0], 0.0, inv_r[0], CLIP))
    assert np.allclose(host(a.unnormalize_reward(a.normalize_reward(r))), np.clip(rew[0], -CLIP / inv_r[0], CLIP / inv_r[0]),
                       rtol=1e-5, atol=1e-5)


def test_without_normalize_nothing_changes():
    """DeviceWrappers(normalize=None) allocates nothing new and equals DeviceFrameStack bitwise on a
    65-env, 143-wide, k = 5 script; Sb3VecEnv(fused=True) equals the unfused adapter."""
    from gym_usv_amd.sb3 import DeviceFrameStack, Sb3VecEnv
    from gym_usv_amd.wrappers import DeviceWrappers
    n, d, k = 65, 143, 5
    obs, final, rew, done = script(n, d, "mix")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    wr, fs = DeviceWrappers(n, d, k, dev()), DeviceFrameStack(n, d, k, dev())
    assert not any(hasattr(wr, a) for a in STATS + ("returns", "norm_rew", "_scratch", "_z"))
    assert same(host(wr.reset(up(obs[0]))), host(fs.reset(up(obs[0]))))
    ep = np.zeros(n)
    for t in range(T):
        stacked, fstack, episode = wr.step(up(obs[t + 1]), up(rew[t]), up(done[t]), up(final[t]))
        want, term = fs.step(up(obs[t + 1]), up(done[t]), up(final[t]))
        assert same(host(stacked), host(want)), t
        ep += rew[t].astype(np.float64)
        if done[t].any():
            assert same(host(fstack)[done[t]], host(term)), t
            assert np.array_equal(host(episode)[done[t], 0], ep[done[t]]), t
        ep[done[t]] = 0
    plain = Sb3VecEnv("usv-simple", num_envs=n, frame_stack=k, seed=4, max_episode_steps=5)
    fused = Sb3VecEnv("usv-simple", num_envs=n, frame_stack=k, seed=4, max_episode_steps=5, fused=True)
    assert fused._wrap._cfg is None and not fused._norm
    assert same(plain.reset(), fused.reset())
    rng = np.random.default_rng(1)
    for t in range(12):
        act = rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32)
        (op, rp, dp, ip), (of, rf, df, inf) = plain.step(act), fused.step(act)
        assert same(op, of) and same(rp, rf) and np.array_equal(dp, df), t
        for a, b in zip(ip, inf):
            assert set(a) == set(b)
            if a:
                assert same(a["terminal_observation"], b["terminal_observation"]) and a["episode"]["r"] == b["episode"]["r"]
    plain.close()
    fused.close()


def test_adapter_with_normalize():
    """make_sb3_vec_env(..., fused=True, normalize={}) against the un-normalised fused adapter with the same
    seed: its raw stream is get_original_obs / get_original_reward; statistics at the derived bounds, obs,
    rewards and terminal_observation bitwise given the device statistics; episode.r raw."""
    import gym_usv_amd
    n, k, d, steps = 256, 5, 143, 40
    raw = gym_usv_amd.make_sb3_vec_env("usv-simple", n, frame_stack=k, seed=2, fused=True, max_episode_steps=7)
    env = gym_usv_amd.make_sb3_vec_env("usv-simple", n, frame_stack=k, seed=2, fused=True, max_episode_steps=7,
                                       normalize={})
    with pytest.raises(ValueError, match="fused"):
        gym_usv_amd.make_sb3_vec_env("usv-simple", n, frame_stack=k, normalize={})
    wr = env._wrap
    assert env.training and env.norm_reward and wr._cfg is not None and not (wr.flags & 1)   # the +0.0 clear
    o_raw, o = raw.reset(), env.reset()
    ref, stack = R.NpVecNormalize(n, d), R.NpFrameStack(n, d, k)
    ref.reset(o_raw[:, -d:])
    assert same(env.get_original_obs(), o_raw[:, -d:])
    mean, inv, rinv = published(wr)
    assert same(o, stack.reset(R.apply(o_raw[:, -d:], mean, inv, CLIP)))
    rng = np.random.default_rng(1)
    xmax, rmax, episodes, updates = float(np.abs(o_raw).max()), 0.0, 0, [1, 0]
    for t in range(steps):
        act = rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32)
        (orw, rrw, drw, irw), (on, rn, dn, inn) = raw.step(act), env.step(act)
        x = orw[:, -d:]
        assert same(env.get_original_obs(), x) and same(env.get_original_reward(), rrw) and np.array_equal(drw, dn), t
        after = ref.step(x, rrw, drw)
        xmax, rmax = max(xmax, float(np.abs(x).max())), max(rmax, float(np.abs(after).max()))
        updates = [updates[0] + 1, updates[1] + 1]
        check_stats(wr, ref, n, updates, xmax, rmax, t)
        rms = env.obs_rms
        assert same(rms.mean, host(wr.obs_mean)) and rms.count == ref.obs_rms.count and env.ret_rms.var == float(wr.ret_var[0])
        mean, inv, rinv = published(wr)
        fin = np.zeros((n, d), np.float32)
        for i in np.flatnonzero(drw):
            fin[i] = irw[i]["terminal_observation"][-d:]
        want, term = stack.update(R.apply(x, mean, inv, CLIP), drw, R.apply(fin, mean, inv, CLIP))
        assert same(on, want) and same(rn, R.apply(rrw, 0.0, rinv, CLIP)), t
        for i in np.flatnonzero(drw):
            episodes += 1
            assert same(inn[i]["terminal_observation"], term[i]), (t, i)
            assert inn[i]["episode"]["r"] == irw[i]["episode"]["r"] and inn[i]["episode"]["l"] == irw[i]["episode"]["l"]
            assert inn[i]["TimeLimit.truncated"] is irw[i]["TimeLimit.truncated"]
    assert episodes >= 5 * n
    env.set_attr("training", False)
    env.norm_reward = False
    assert wr.training is False and wr.norm_reward is False
    before = snapshot(wr)
    act = rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32)
    (_, rrw, _, _), (_, rn, _, _) = raw.step(act), env.step(act)
    assert same(rn, rrw) and all(same(v, before[k2]) for k2, v in snapshot(wr).items())
    raw.close()
    env.close()


def test_adapter_save_and_load(tmp_path):
    import gym_usv_amd
    n = 64
    a = gym_usv_amd.make_sb3_vec_env("usv-simple", n, frame_stack=2, seed=5, fused=True, normalize={})
    a.reset()
    rng = np.random.default_rng(2)
    for _ in range(3):
        a.step(rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32))
    path = str(tmp_path / "vecnormalize.npz")
    a.save(path)
    b = gym_usv_amd.make_sb3_vec_env("usv-simple", n, frame_stack=2, seed=5, fused=True,
                                     normalize=dict(training=False))
    b.load(path)
    for name in STATS + ("returns",):
        assert torch.equal(getattr(a._wrap, name), getattr(b._wrap, name)), name
    a.close()
    b.close()


def test_f64_env_rewards_feed_returns():
    """A precision="f64" env: float64 rewards go into returns unrounded."""
    import gym_usv_amd
    n, k, steps = 65, 5, 8
    env = gym_usv_amd.make_vec("usv-simple", n, seed=3, precision="f64", max_episode_steps=3, copy=False)
    d = env.obs_dim
    assert env.reward.dtype == torch.float64
    wr = make(n, d, k, torch.float64)
    ref, stack = R.NpVecNormalize(n, d), R.NpFrameStack(n, d, k)
    obs, _ = env.reset(seed=3)
    x = host(obs)
    st = wr.reset(obs)
    ref.reset(x)
    mean, inv, rinv = published(wr)
    assert same(host(st), stack.reset(R.apply(x, mean, inv, CLIP)))
    rng = np.random.default_rng(0)
    xmax, rmax, updates, dones = float(np.abs(x).max()), 0.0, [1, 0], 0
    for t in range(steps):
        act = torch.from_numpy(rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32)).to(dev())
        obs, rew, _, _, info = env.step(act)
        x, r, dn, fin = host(obs), host(rew), host(info["_final_obs"]).astype(bool), host(info["final_obs"])
        assert r.dtype == np.float64 and (r != r.astype(np.float32)).any()
        stacked, fstack, _ = wr.step(obs, rew, info["_final_obs"], info["final_obs"])
        after = ref.step(x, r, dn)
        xmax, rmax = max(xmax, float(np.abs(x).max())), max(rmax, float(np.abs(after).max()))
        updates = [updates[0] + 1, updates[1] + 1]
        check_stats(wr, ref, n, updates, xmax, rmax, t)
        mean, inv, rinv = published(wr)
        want, term = stack.update(R.apply(x, mean, inv, CLIP), dn, R.apply(fin, mean, inv, CLIP))
        assert same(host(stacked), want) and same(host(fstack)[dn], term[dn]), t
        assert same(host(wr.norm_rew), R.apply(r, 0.0, rinv, CLIP)), t
        dones += int(dn.sum())
    assert dones >= 2 * n
    env.close()
