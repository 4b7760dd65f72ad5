"""HIP kernel vs CPU oracle parity (run on an MI355X: pytest -m gpu).

Tolerances (fp32 kernel vs float64 oracle, state injected so both start identical):
  * single step:  obs atol 1e-5 + rtol 1e-4 per element, reward atol 1e-4, flags exact except
    envs whose deciding quantity is within 1e-4 of its threshold; lidar rays whose hit/miss
    decision flips at a grazing ray (|r^2 - perp^2| tiny) <= 1e-4 of rays.
  * float64 kernel (usv-simple, usv-asmc-simple): obs equal to the reference's bit for bit, header and
    sensors; reward 2e-14; no flag mismatch and no collision-threshold flip (DESIGN.md's parity table).
    The legacy ids keep float32-rounding bounds: the reference's own float32 rounding is in them.
  * golden trajectories (reference-generated): compared up to each env's first episode end.
"""
import numpy as np
import pytest
import torch

from oracle import usv_oracle as O

pytestmark = pytest.mark.gpu

F32_OBS_ATOL, F32_OBS_RTOL, F32_REW_ATOL = 1e-5, 1e-4, 1e-4


def make(env_id, n, **kw):
    import gym_usv_amd
    return gym_usv_amd.make_vec(env_id, n, device=0, **kw)


def inject(env, orc, elapsed=None, scan_valid=1):
    st = orc.get_state()
    env.set_state(st)
    env.set_field("elapsed", 0 if elapsed is None else elapsed)
    env.set_field("scan_valid", scan_valid)


def golden_state(g):
    p, v, la, ma = g["init_position"], g["init_velocity"], g["init_last_action"], g["init_max_action"]
    return {"x": p[:, 0], "y": p[:, 1], "psi": p[:, 2], "u": v[:, 0], "v": v[:, 1], "r": v[:, 2],
            "last_u": la[:, 0], "last_r": la[:, 2], "progress": g["init_progress"],
            "path_x0": g["init_path_start"][:, 0], "path_y0": g["init_path_start"][:, 1],
            "path_x1": g["init_path_end"][:, 0], "path_y1": g["init_path_end"][:, 1],
            "max_u": ma[:, 0], "max_r": ma[:, 2], "ref_v": g["init_ref_v"],
            "n_obs": g["init_n_obs"], "obs_x": g["init_ox"], "obs_y": g["init_oy"],
            "obs_r": g["init_orad"], "sensor_last": g["init_sensors"], "elapsed": 0,
            "scan_valid": 0, "asmc": 0.0}


def to_np(*ts):
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy() for t in ts]


F64_REW_TOL = 2e-14
# The step's ye multiplies sin / cos of the path angle by the boat's offset from the path start, and the
# reward's slope in ye is at most 1 / 0.075 (exp(-|ye/k|), exp(-(ye/k)^2), k = 0.075).  Two correctly
# working routes to that sin / cos (the reference's sin/cos(atan2) in glibc; dy/|d|, dx/|d| or OCML's
# sin/cos(atan2) in the kernel: both were measured, neither is closer) differ by up to two ulps each, so
# the f64 reward carries 4 * 2^-53 / 0.075 = 5.9e-15 per metre of |x - x0| + |y - y0| on top of 2e-14.
# Measured: 1.0e-16 per metre at worst (2.7e-13 at 200 m), 7.1e-15 in all within 20 m of the path start.
F64_REW_PER_METRE = 4 * 2.0 ** -53 / 0.075


def bits_off(a, b):
    """How many float32 entries differ in their bits (a signed zero or a last-place flip counts)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


# --------------------------------------------------------------------------- golden replay
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("fname,env_id", [("simple_traj.npz", "usv-simple"),
                                          ("simple_traj_tl.npz", "usv-simple"),
                                          ("asmc_simple_traj.npz", "usv-asmc-simple")])
def test_golden_trajectory_replay(golden, fname, env_id, precision):
    """Reference trajectories (generated from gym_usv itself) replayed through the kernel from the
    reference's post-reset state, autoreset off, up to each env's first episode end."""
    g = golden(fname)
    n, T = g["actions"].shape[:2]
    limit = int(g["limit"])
    env = make(env_id, n, precision=precision, autoreset=False, max_episode_steps=max(limit, 0))
    env.set_state(golden_state(g))
    alive = np.ones(n, bool)
    worst = {"hdr": 0.0, "rew": 0.0}
    flips, rays, off = 0, 0, 0
    # f32 trajectories accumulate rounding along the rollout (about 5x the measured worst case:
    # usv-simple header 1.4e-6 / reward 1.3e-5; usv-asmc-simple 2.7e-6 / 3.5e-5 since the f32 ASMC
    # integrates the pose with compensated summation -- 1.0e-4 without it, the reward's ye term
    # amplifying a ~50 m float32 position rounded 20 times per step).  The usv-asmc-simple reward
    # tolerance is SURVEY §8(c)'s 1e-4.
    if precision == "f64":
        hdr_tol, sens_tol, rew_tol = 0.0, 0.0, F64_REW_TOL   # and bit for bit, below
    else:
        hdr_tol, sens_tol, rew_tol = (7e-6, 1e-4, 7e-5) if env_id == "usv-simple" else (1.5e-5, 1e-4, 1e-4)
    for t in range(T):
        a = torch.from_numpy(g["actions"][:, t]).cuda()
        obs, rew, term, trunc, _ = env.step(a)
        obs, rew, term, trunc = to_np(obs, rew, term, trunc)
        m = alive
        if not m.any():
            break
        ref = g["final_obs"][m, t]
        worst["hdr"] = max(worst["hdr"], float(np.abs(obs[m, :15] - ref[:, :15]).max()))
        worst["rew"] = max(worst["rew"], float(np.abs(rew[m] - g["reward"][m, t]).max()))
        off += bits_off(obs[m], ref)
        # a ray grazing an obstacle edge can flip hit/miss under fp32 rounding: count, bound
        flips += int((np.abs(obs[m, 15:] - ref[:, 15:]) > sens_tol).sum())
        rays += int(m.sum()) * 128
        np.testing.assert_array_equal(term[m], g["terminated"][m, t], err_msg=f"t={t}")
        np.testing.assert_array_equal(trunc[m], g["truncated"][m, t], err_msg=f"t={t}")
        alive = alive & ~(g["terminated"][:, t] | g["truncated"][:, t])
    print(f"\n[golden {fname} {precision}] max |hdr| err {worst['hdr']:.3e}, max |rew| err "
          f"{worst['rew']:.3e}, sensor flips {flips}/{rays}, obs entries not bit-equal {off}")
    assert worst["hdr"] <= hdr_tol and worst["rew"] <= rew_tol, worst
    assert precision != "f64" or off == 0, off
    assert flips <= (0 if precision == "f64" else max(2, rays // 10000))
    env.close()


# --------------------------------------------------------------------------- single step @ C2
def _scatter(orc_env, rng):
    """Spread poses over the whole 100 m field, a quarter of them near the corners, so many envs
    see obstacles >= 99 m away (the lidar's max-range test, usv_asmc_ca_env.py:458)."""
    n = orc_env.position.shape[0]
    xy = rng.uniform(0.3, 99.7, size=(n, 2))
    k = n // 4
    xy[:k] = np.clip(rng.choice([1.0, 99.0], size=(k, 2)) + rng.normal(0, 0.5, (k, 2)), 0.05, 99.95)
    orc_env.position[:, :2] = xy
    orc_env.position[:, 2] = rng.uniform(-np.pi, np.pi, n)


def _single_step_round(env_id, n, precision, rounds=4, warm=25, seed=0, scatter=False):
    orc = O.OracleVectorEnv(env_id, n)
    orc.reset(list(range(seed, seed + n)))
    rng = np.random.default_rng(seed)
    for _ in range(warm):
        orc.step(rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32))
    env = make(env_id, n, precision=precision, autoreset=True)
    stats = []
    for _ in range(rounds):
        if scatter:
            _scatter(orc.env, rng)
        inject(env, orc.env, elapsed=orc.elapsed.astype(np.int32))
        a = rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32)
        obs, rew, term, trunc, info = env.step(torch.from_numpy(a).cuda())
        g_obs, g_rew, g_term, g_trunc, g_fobs = to_np(obs, rew, term, trunc, info["final_obs"])
        # oracle: same step without its (PCG64) reset, then compare terminal rows
        sens_before = orc.env.sensors.copy()
        lever = np.abs(orc.env.position[:, :2] - orc.env.path_start).sum(axis=1) + 1.0   # (a step moves < 1 m)
        o_obs, o_rew, o_term, o_trunc, o_fobs, o_done = orc.step(a)
        done = g_term | g_trunc
        stats.append(dict(n=n, term_mis=int((g_term != o_term).sum()), trunc_mis=int((g_trunc != o_trunc).sum()),
                          obs=(g_fobs, g_obs, o_fobs, done & (o_term | o_trunc)),
                          rew=(g_rew, o_rew), lever=lever, flags_ok=(g_term == o_term) & (g_trunc == o_trunc)))
        del sens_before
    env.close()
    return stats


def _check_rows(g_rows, o_rows, atol, rtol, label, bitwise=False):
    hdr_err = np.abs(g_rows[:, :15] - o_rows[:, :15])
    hdr_bad = hdr_err > atol + rtol * np.abs(o_rows[:, :15])
    sens_err = np.abs(g_rows[:, 15:] - o_rows[:, 15:])
    sens_bad = sens_err > atol + rtol * np.abs(o_rows[:, 15:])
    frac = sens_bad.mean()
    print(f"[{label}] header max err {hdr_err.max():.3e} (bad {int(hdr_bad.sum())}), "
          f"sensor max err {sens_err.max():.3e}, grazing-ray flips {int(sens_bad.sum())} ({frac:.2e})")
    assert hdr_bad.sum() == 0, f"{label}: header mismatch"
    assert frac <= 1e-4, f"{label}: too many lidar mismatches"
    if bitwise:
        assert bits_off(g_rows, o_rows) == 0, f"{label}: {bits_off(g_rows, o_rows)} obs entries not bit-equal"


@pytest.mark.parametrize("env_id", ["usv-simple", "usv-asmc-simple"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("scatter", [False, True], ids=["near-start", "scattered"])
def test_single_step_parity_4096(env_id, precision, scatter):
    """One step from oracle-injected states vs the oracle.  `scattered` spreads the poses over
    the field so obstacles beyond the 99 m far threshold occur (lidar max-range test).
    f64 asserts DESIGN.md's parity table: obs bit for bit, no flag mismatch, no collision-threshold flip,
    reward <= 2e-14 plus F64_REW_PER_METRE per metre from the path start (the scattered poses lie up to
    200 m from it; near the start that term is below 2e-14 and the table's figure is what holds)."""
    n = 4096 if env_id == "usv-simple" else 2048
    atol, rtol, ratol = (F32_OBS_ATOL, F32_OBS_RTOL, F32_REW_ATOL) if precision == "f32" else (0.0, 0.0, F64_REW_TOL)
    f64 = precision == "f64"
    flag_slack = 0 if f64 else max(1, n // 2000)          # f64: no flag mismatch, no collision-threshold flip
    # usv-asmc-simple f32 (20 ASMC substeps) holds the same SURVEY §8(c) bounds: r02 measured
    # header 1.7e-6, reward 6.5e-5
    for k, s in enumerate(_single_step_round(env_id, n, precision, scatter=scatter)):
        assert s["term_mis"] <= flag_slack and s["trunc_mis"] <= flag_slack, (s["term_mis"], s["trunc_mis"])
        ok = s["flags_ok"]
        g_fobs, g_obs, o_fobs, both_done = s["obs"]
        g_rew, o_rew = s["rew"]
        not_done = ok & ~both_done
        # envs not done: returned obs must equal the oracle's obs
        # (their stepped state is identical, reset rows differ by RNG stream)
        rows = np.flatnonzero(not_done)
        # the oracle vector env resets done envs, so its obs for not-done envs is the step obs
        from_o = o_fobs  # oracle terminal-or-step obs (before any reset)
        _check_rows(g_obs[rows], from_o[rows], atol, rtol, f"{env_id} {precision} round {k} obs", f64)
        drows = np.flatnonzero(ok & both_done)
        if drows.size:
            _check_rows(g_fobs[drows], from_o[drows], atol, rtol, f"{env_id} {precision} round {k} final_obs", f64)
        rerr = np.abs(g_rew[ok] - o_rew[ok])
        coll_flip = (np.abs(rerr - 20) < 1)       # min sensor within rounding of 0.2
        print(f"[{env_id} {precision} round {k}] reward max err {rerr[~coll_flip].max():.3e}, "
              f"collision-threshold flips {int(coll_flip.sum())}")
        tol = ratol + F64_REW_PER_METRE * s["lever"][ok] if f64 else np.full(rerr.shape, ratol)
        print(f"    reward error over its bound: max {(rerr / tol)[~coll_flip].max():.3f}; lever up to {s['lever'].max():.0f} m")
        assert (rerr <= tol)[~coll_flip].all()
        assert coll_flip.sum() <= flag_slack


# --------------------------------------------------------------------------- resets
def test_reset_distribution_matches_reference():
    """In-kernel Philox resets vs the reference's PCG64 resets (oracle, pinned to the reference):
    two-sample KS per drawn quantity (simple_env.py:228-308)."""
    from scipy import stats
    n = 8192
    env = make("usv-simple", n, seed=123)
    obs, _ = env.reset(seed=123)
    (obs,) = to_np(obs)
    g = env.get_state()
    orc = O.SimpleEnvBatch(n)
    o_obs = orc.reset(seeds=list(range(10_000, 10_000 + n)))
    o = orc.get_state()
    pairs = {
        "path_x0": (g["path_x0"], o["path_x0"]), "psi": (g["psi"], o["psi"]),
        "u": (g["u"], o["u"]), "r": (g["r"], o["r"]), "max_u": (g["max_u"], o["max_u"]),
        "max_r": (g["max_r"], o["max_r"]), "ref_v": (g["ref_v"], o["ref_v"]),
        "path_len": (np.hypot(g["path_x1"] - g["path_x0"], g["path_y1"] - g["path_y0"]),
                     np.hypot(o["path_x1"] - o["path_x0"], o["path_y1"] - o["path_y0"])),
        "path_angle": (np.arctan2(g["path_y1"] - g["path_y0"], g["path_x1"] - g["path_x0"]),
                       np.arctan2(o["path_y1"] - o["path_y0"], o["path_x1"] - o["path_x0"])),
        "obs_angle": (obs[:, 3], o_obs[:, 3]), "obs_dist": (obs[:, 4], o_obs[:, 4]),
    }
    valid_g = np.arange(32)[None] < g["n_obs"][:, None]
    valid_o = np.arange(32)[None] < o["n_obs"][:, None]
    pairs["obs_r"] = (g["obs_r"][valid_g], o["obs_r"][valid_o])
    pairs["obs_x"] = (g["obs_x"][valid_g], o["obs_x"][valid_o])
    for k, (a, b) in pairs.items():
        p = stats.ks_2samp(a, b).pvalue
        print(f"KS {k}: p={p:.3g}")
        assert p > 1e-4, k
    hg = np.bincount(g["n_obs"], minlength=32) / n
    ho = np.bincount(o["n_obs"], minlength=32) / n
    assert 0.5 * np.abs(hg - ho).sum() < 0.05
    # fresh reset obs: zero action features, kinematic constants, stale sensors = zeros, ye = 0
    assert np.all(obs[:, [7, 8, 10, 13]] == 0) and np.all(obs[:, 5] == 0)
    np.testing.assert_allclose(obs[:, [12, 14]], np.tile([0.175, 0.3], (n, 1)), rtol=1e-6)
    assert np.all(obs[:, 15:] == 0)
    assert np.all(g["elapsed"] == 0) and np.all(g["episode"] == 1)
    env.close()


def test_autoreset_semantics_and_time_limit():
    n, T, limit = 1024, 60, 25
    env = make("usv-simple", n, seed=7, max_episode_steps=limit)
    env.reset(seed=7)
    gen = torch.Generator(device="cuda").manual_seed(0)
    lo = torch.tensor([0.2, -1.0], device="cuda")
    span = torch.tensor([0.8, 2.0], device="cuda")
    age = np.zeros(n, np.int64)        # steps since this env's episode started
    ends = 0
    for t in range(T):
        a = torch.rand(n, 2, device="cuda", generator=gen) * span + lo
        obs, rew, term, trunc, info = env.step(a)
        obs, term, trunc, fobs = to_np(obs, term, trunc, info["final_obs"])
        age += 1
        done = term | trunc
        # TimeLimit (gym_usv/__init__.py:27): truncated exactly when elapsed reaches the limit
        assert np.all(trunc[age == limit]), t
        el = env.get_field("elapsed")
        np.testing.assert_array_equal(el[done], 0)
        np.testing.assert_array_equal(el[~done], age[~done])
        if done.any():
            ends += int(done.sum())
            # reset obs keeps the terminal scan (stale sensor_data, simple_env.py:47,302)
            np.testing.assert_array_equal(obs[done, 15:], fobs[done, 15:])
            assert np.all(obs[done, 7:9] == 0)                 # _get_obs(zeros(3))
            assert np.all(obs[done, 5] == 0)                   # ye at path start
            # last_action is NOT reset (reference quirk): the next obs shows it again
            assert np.all(env.get_field("last_u")[done] != 0)
        age[done] = 0
    assert ends > n                                             # every env hit the limit at least once
    env.close()


def test_explicit_reset_mask_and_stale_scan():
    n = 256
    env = make("usv-simple", n, seed=3, autoreset=False)
    obs0, _ = env.reset(seed=3)
    a = torch.full((n, 2), 0.5, device="cuda")
    obs, *_ = env.step(a)
    (obs,) = to_np(obs.clone())
    st_before = env.get_state()
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask[::2] = True
    obs2, _ = env.reset(mask=mask)
    (obs2,) = to_np(obs2)
    st = env.get_state()
    m = np.zeros(n, bool)
    m[::2] = True
    # masked envs: new episode, reset obs carries the scan of the last step
    np.testing.assert_array_equal(obs2[m, 15:], obs[m, 15:])
    assert np.all(st["episode"][m] == 2) and np.all(st["episode"][~m] == 1)
    # unmasked envs untouched
    for k in ("x", "y", "psi", "n_obs"):
        np.testing.assert_array_equal(st[k][~m], st_before[k][~m])
    # a second reset without a step re-serves the same stale scan
    obs3, _ = env.reset(mask=mask)
    (obs3,) = to_np(obs3)
    np.testing.assert_array_equal(obs3[m, 15:], obs[m, 15:])
    env.close()


def test_determinism_and_sharding_invariance():
    """Same (seed, global env id) -> same trajectory, whatever the env partition."""
    T = 40
    a_full = make("usv-simple", 256, seed=11)
    b_half = make("usv-simple", 128, seed=11, env_id_offset=128)
    a_full.reset(seed=11)
    b_half.reset(seed=11)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(T):
        act = torch.rand(256, 2, device="cuda", generator=gen)
        oa, ra, *_ = a_full.step(act)
        ob, rb, *_ = b_half.step(act[128:].contiguous())
        torch.testing.assert_close(oa[128:], ob, rtol=0, atol=0)
        torch.testing.assert_close(ra[128:], rb, rtol=0, atol=0)
    a_full.close()
    b_half.close()


def test_state_blob_roundtrip():
    n = 512
    env = make("usv-asmc-simple", n, seed=2)
    env.reset(seed=2)
    gen = torch.Generator(device="cuda").manual_seed(1)
    acts = [torch.rand(n, 2, device="cuda", generator=gen) for _ in range(6)]
    for a in acts[:3]:
        env.step(a)
    blob = env.state_blob()
    outs1 = []
    for a in acts[3:]:
        o, r, *_ = env.step(a)
        outs1.append((o.clone(), r.clone()))
    env.load_state_blob(blob)
    for (o1, r1), a in zip(outs1, acts[3:]):
        o, r, *_ = env.step(a)
        torch.testing.assert_close(o, o1, rtol=0, atol=0)
        torch.testing.assert_close(r, r1, rtol=0, atol=0)
    env.close()


def test_single_env_api():
    import gym_usv_amd
    env = gym_usv_amd.make("usv-simple")
    obs, info = env.reset(seed=0)
    assert obs.shape == (143,) and obs.dtype == np.float32
    obs, r, term, trunc, info = env.step(np.array([0.5, 0.0], dtype=np.float32))
    assert isinstance(r, float) and isinstance(term, bool) and isinstance(trunc, bool)
    env.close()


@pytest.mark.parametrize("env_id,precision", [("usv-simple", "f32"), ("usv-simple", "f64"),
                                              ("usv-asmc-simple", "f32"), ("usv-asmc-simple", "f64")])
def test_step_variants_bit_identical(env_id, precision):
    """Every step-kernel variant (envs/block, blind-sector skip, unroll, angular-window pair
    expansion) must give bit-identical outputs: pruning only removes pairs that cannot hit."""
    n, T = 2048, 24
    gen = torch.Generator(device="cuda").manual_seed(9)
    acts = [torch.rand(n, 2, device="cuda", generator=gen) * torch.tensor([0.8, 2.0], device="cuda")
            + torch.tensor([0.2, -1.0], device="cuda") for _ in range(T)]
    ref = None
    # block queue: f32 only (lid 263 / 519: obs rows as aligned env-pair spans forced on / off)
    queue = ("128,7,4", "128,7,5", "16,7,5", "128,263,5", "16,263,5", "128,519,5") if precision == "f32" else ()
    if precision == "f32" and env_id == "usv-asmc-simple":
        queue += ("128,7,6", "16,7,6")                # ASMC chain kernel + fused block queue
    if precision == "f64":                            # f64: split scan at 16 envs/wave; block-wide dynamics
        queue = ("64,7,2", "64,7,3", "32,7,3") if env_id == "usv-simple" else ("64,7,2",)
    for v in ("64,7,1", "32,0,1", "32,3,1", "16,7,1", "32,7,1", "16,0,2", "32,3,2", "8,7,2", "16,7,2", "32,7,2") + queue:
        env = make(env_id, n, seed=4, precision=precision, kernel_variant=v)
        env.reset(seed=4)
        outs = []
        for a in acts:
            o, r, te, tr, info = env.step(a)
            outs.append((o.clone(), r.clone(), te.clone(), tr.clone()))
        env.close()
        if ref is None:
            ref = outs
            continue
        for t, (a_, b_) in enumerate(zip(ref, outs)):
            for x, y in zip(a_, b_):
                assert torch.equal(x, y), f"variant {v} differs at step {t}"


@pytest.mark.parametrize("n", [1, 77, 1077])
def test_block_queue_ragged_sizes(n):
    """Block-queue step (kinds 4, 5: 128-env blocks of 16 waves pulling env pairs from an LDS
    counter) on env counts that leave a partial block and an odd last pair: bit-identical to
    the fused wave kernel over a rollout with resets."""
    T = 40
    gen = torch.Generator(device="cuda").manual_seed(5)
    acts = [torch.rand(n, 2, device="cuda", generator=gen) * torch.tensor([0.8, 2.0], device="cuda")
            + torch.tensor([0.2, -1.0], device="cuda") for _ in range(T)]
    ref = None
    for v in ("64,7,1", "128,7,5", "16,7,5", "128,7,4", "16,7,2", "128,263,5", "16,263,5", "128,263,4"):
        env = make("usv-simple", n, seed=6, max_episode_steps=12, kernel_variant=v, copy=False)
        env.reset(seed=6)
        outs = []
        for a in acts:
            o, r, te, tr, info = env.step(a)
            outs.append((o.clone(), r.clone(), te.clone(), tr.clone(), info["final_obs"].clone()))
        env.close()
        if ref is None:
            ref = outs
            continue
        for t, (a_, b_) in enumerate(zip(ref, outs)):
            for x, y in zip(a_, b_):
                assert torch.equal(x, y), f"variant {v} differs at step {t} (n={n})"


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_step_variants_bit_identical_scattered(precision):
    """Variant bit-identity from injected poses spread over the field (far obstacles, envs
    near walls and corners), where the range-checked lidar paths run."""
    n = 4096
    orc = O.OracleVectorEnv("usv-simple", n)
    orc.reset(list(range(100, 100 + n)))
    rng = np.random.default_rng(11)
    _scatter(orc.env, rng)
    far = np.zeros(n, bool)
    for i in range(n):
        m = orc.env.n_obs[i]
        d = np.hypot(orc.env.ox[i, :m] - orc.env.position[i, 0], orc.env.oy[i, :m] - orc.env.position[i, 1])
        far[i] = (d >= 99).any()
    assert far.mean() > 0.1, far.mean()          # the far path is actually exercised
    a = torch.from_numpy(rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32)).cuda()
    ref = None
    queue = ("128,7,4", "128,7,5", "16,7,5", "128,263,5") if precision == "f32" else ("64,7,2", "64,7,3", "32,7,3")
    for v in ("64,7,1", "32,3,1", "32,7,1", "16,0,1", "16,3,2", "8,7,2", "16,7,2") + queue:
        # copy=False: final_obs rows of envs that did not end keep the (identical) buffer contents
        env = make("usv-simple", n, seed=3, precision=precision, kernel_variant=v, copy=False)
        inject(env, orc.env, elapsed=1)
        o, r, te, tr, info = env.step(a)
        out = [x.clone() for x in (o, r, te, tr, info["final_obs"])]
        env.close()
        if ref is None:
            ref = out
            continue
        for x, y in zip(ref, out):
            assert torch.equal(x, y), f"variant {v} differs"


def _window_pairs(e):
    """Host estimate of the window lidar's (obstacle, ray) pairs per env at the current pose: the
    rays (128 over 240 degrees from heading - 120, usv_asmc_ca_env.py:411-427) within asin(r / d) of
    the obstacle's bearing, all 128 when the boat is inside it."""
    res = np.deg2rad(240.0) / 128
    dx, dy = e.ox - e.position[:, :1], e.oy - e.position[:, 1:2]
    d = np.hypot(dx, dy)
    half = np.arcsin(np.clip(e.orad / np.maximum(d, 1e-9), 0, 1))
    ray = e.position[:, 2:3, None] - np.deg2rad(120.0) + res * np.arange(128)[None, None, :]
    diff = np.angle(np.exp(1j * (ray - np.arctan2(dy, dx)[:, :, None])))
    cnt = np.where(d <= e.orad, 128, (np.abs(diff) <= half[:, :, None]).sum(2))
    valid = np.arange(e.ox.shape[1])[None, :] < e.n_obs[:, None]
    return (cnt * valid).sum(1)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_step_variants_bit_identical_crowded(precision):
    """Variant bit-identity where the window lidar's pair list is long: the boat sits next to or
    inside clusters of obstacles, so windows span up to all 128 rays and an env pair's list runs to
    2-4 passes of 64 (the window kernels do passes 0 and 1 together and the rest one at a time);
    brute-force variants are the reference."""
    n = 2048
    orc = O.OracleVectorEnv("usv-simple", n)
    orc.reset(list(range(300, 300 + n)))
    e = orc.env
    rng = np.random.default_rng(23)
    # pull obstacles 1..k around obstacle 0 and park the boat beside it (every 4th env inside it)
    for i in range(n):
        m = int(e.n_obs[i])
        k = min(m - 1, int(rng.integers(2, 8)))
        cx, cy = e.ox[i, 0], e.oy[i, 0]
        ang = rng.uniform(0, 2 * np.pi, k)
        dist = rng.uniform(0.5, 3.0, k)
        e.ox[i, 1:1 + k] = cx + dist * np.cos(ang)
        e.oy[i, 1:1 + k] = cy + dist * np.sin(ang)
        off = 0.0 if i % 4 == 0 else rng.uniform(0.6, 2.5)
        th = rng.uniform(0, 2 * np.pi)
        e.position[i, 0] = np.clip(cx + off * np.cos(th), 0.05, 99.95)
        e.position[i, 1] = np.clip(cy + off * np.sin(th), 0.05, 99.95)
    e.position[:, 2] = rng.uniform(-np.pi, np.pi, n)
    assert (_window_pairs(e).reshape(-1, 2).sum(1) > 128).mean() > 0.3   # >= 3 passes per env pair
    a = torch.from_numpy(rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32)).cuda()
    ref = None
    queue = ("128,7,4", "128,7,5", "16,7,5") if precision == "f32" else ("64,7,2", "64,7,3", "32,7,3")
    for v in ("64,0,1", "32,3,1", "64,7,1", "16,7,2", "8,7,2") + queue:
        env = make("usv-simple", n, seed=3, precision=precision, kernel_variant=v, copy=False)
        inject(env, e, elapsed=1)
        o, r, te, tr, info = env.step(a)
        out = [x.clone() for x in (o, r, te, tr, info["final_obs"])]
        env.close()
        if ref is None:
            ref = out
            # the scenes are what they claim: many readings short of max range
            assert float((out[0][:, 15:] < 0.05).float().mean()) > 0.2
            continue
        for x, y in zip(ref, out):
            assert torch.equal(x, y), f"variant {v} differs"


# --------------------------------------------------------------------------- usv-asmc-v0 (legacy)
def _v0_inject(env, o, first):
    env.set_state({"x": o.position[:, 0], "y": o.position[:, 1], "psi": o.position[:, 2],
                   "u": o.velocity[:, 0], "v": o.velocity[:, 1], "r": o.velocity[:, 2],
                   "v0_last": o.last, "v0_aux": o.aux, "v0_target": o.target,
                   "v0_action_last": o.state[:, 5], "elapsed": np.where(first, 0, 1)})


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_v0_golden_trajectory_replay(golden, precision):
    """Reference usv-asmc-v0 rollouts (usv_asmc_env.py:99-255) replayed from the reference's reset
    state, autoreset off, up to each env's first done."""
    g = golden("asmc_v0_traj.npz")
    n, T = g["actions"].shape
    env = make("usv-asmc-v0", n, precision=precision, autoreset=False)
    o = O.AsmcV0Batch(n)
    o.reset([int(s) for s in g["seeds"]])
    _v0_inject(env, o, np.ones(n, bool))
    alive = np.ones(n, bool)
    worst_o = worst_r = 0.0
    # r02 measured: f64 obs 9.5e-7 (the reference's own float32 rounding), f32 obs 9.5e-7 / reward 1.2e-6
    tol_o, tol_r = (5e-6, 1e-6) if precision == "f64" else (5e-6, 6e-6)
    steps = T if precision == "f64" else 600      # f32 state drifts along chaotic ASMC switches
    for t in range(steps):
        obs, rew, term, trunc, _ = env.step(torch.from_numpy(g["actions"][:, t:t + 1]).cuda())
        obs, rew, term = to_np(obs, rew, term)
        m = alive
        if not m.any():
            break
        worst_o = max(worst_o, float(np.abs(obs[m] - g["final_obs"][m, t]).max()))
        worst_r = max(worst_r, float(np.abs(rew[m] - g["reward"][m, t]).max()))
        np.testing.assert_array_equal(term[m], g["done"][m, t], err_msg=f"t={t}")
        alive = alive & ~g["done"][:, t]
    print(f"\n[golden asmc_v0 {precision}] max |obs| err {worst_o:.3e}, max |rew| err {worst_r:.3e}")
    assert worst_o <= tol_o and worst_r <= tol_r
    env.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_v0_single_step_parity_4096(precision):
    n = 4096
    o = O.AsmcV0Batch(n)
    o.reset(list(range(n)))
    rng = np.random.default_rng(3)
    first = np.ones(n, bool)
    for _ in range(40):
        _, _, dn = o.step(rng.uniform(-np.pi / 2, np.pi / 2, n).astype(np.float32))
        first[:] = False
        if dn.any():
            o.reset(idx=np.flatnonzero(dn))
            first[dn] = True
    env = make("usv-asmc-v0", n, precision=precision, autoreset=True)
    for k in range(3):
        _v0_inject(env, o, first)
        a = rng.uniform(-np.pi / 2, np.pi / 2, n).astype(np.float32)
        obs, rew, term, trunc, info = env.step(torch.from_numpy(a).cuda())
        g_obs, g_rew, g_term, g_fobs = to_np(obs, rew, term, info["final_obs"])
        o_obs, o_rew, o_done = o.step(a)
        first[:] = False
        assert (g_term != o_done).sum() <= 1
        ok = g_term == o_done
        rows = np.where((g_term & ok)[:, None], g_fobs, g_obs)
        tol = 2e-6 if precision == "f64" else 2e-4
        err = np.abs(rows[ok] - o_obs[ok])
        print(f"[v0 {precision} round {k}] obs max err {err.max():.3e}, reward max err "
              f"{np.abs(g_rew[ok] - o_rew[ok]).max():.3e}, done {int(o_done.sum())}")
        assert err.max() <= tol
        assert np.abs(g_rew[ok] - o_rew[ok]).max() <= (1e-6 if precision == "f64" else 1e-3)
        if o_done.any():
            idx = np.flatnonzero(o_done)
            o.reset(idx=idx)
            first[idx] = True
    env.close()


def test_v0_reset_distribution():
    from scipy import stats
    n = 8192
    env = make("usv-asmc-v0", n, seed=5)
    obs, _ = env.reset(seed=5)
    (obs,) = to_np(obs)
    g = env.get_state()
    o = O.AsmcV0Batch(n)
    o_obs = o.reset(list(range(n)))
    tg = g["v0_target"]
    for name, a, b in (("x", g["x"], o.position[:, 0]), ("psi", g["psi"], o.position[:, 2]),
                       ("x0", tg[:, 0], o.target[:, 0]), ("speed", tg[:, 2], o.target[:, 2]),
                       ("x_d", tg[:, 4], o.target[:, 4]), ("ye", obs[:, 3], o_obs[:, 3])):
        p = stats.ks_2samp(a, b).pvalue
        print(f"KS v0 {name}: p={p:.3g}")
        assert p > 1e-4, name
    assert np.all(tg[:, 3] == 0) and np.all(obs[:, [0, 1, 2, 5]] == 0)     # ak == 0 (y_d = y_0)
    env.close()


# --------------------------------------------------------------------------- usv-asmc-ye-int-v0 / usv-pid-v0
LEGACY_F64 = [("usv-asmc-ye-int-v0", "ye_int", "asmc_ye_int_traj.npz"), ("usv-pid-v0", "pid", "pid_traj.npz")]


def _legacy_inject(env, o):
    env.set_state({"x": o.position[:, 0], "y": o.position[:, 1], "psi": o.position[:, 2],
                   "u": o.velocity[:, 0], "v": o.velocity[:, 1], "r": o.velocity[:, 2],
                   "v0_last": o.last[:, :9], "v0_aux": o.aux[:, :3], "v0_target": o.target,
                   "v0_action_last": o.state[:, 5],
                   "v0_ye": np.stack([o.aux[:, 3], o.last[:, 9]], axis=1), "elapsed": 0})


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("env_id,family,fname", LEGACY_F64)
def test_legacy_f64_golden_trajectory_replay(golden, env_id, family, fname, precision):
    """Reference usv-asmc-ye-int-v0 / usv-pid-v0 rollouts (usv_asmc_ye_int_env.py:92-253,
    usv_pid_env.py:89-233) replayed from the reference's reset state, autoreset off, up to each
    env's first done.  f64: the kernel follows the reference's float64 statement order, so only
    libm ulps separate them (obs to 1e-6 over 2000 steps); f32: 600 steps at 2e-3."""
    g = golden(fname)
    n, T = g["actions"].shape
    env = make(env_id, n, precision=precision, autoreset=False)
    o = O.LegacyF64Batch(n, family)
    o.reset([int(s) for s in g["seeds"]])
    _legacy_inject(env, o)
    alive = np.ones(n, bool)
    worst_o = worst_r = 0.0
    # r02 measured f32 (600 steps): obs <= 5.6e-6, reward <= 7.6e-6
    tol_o, tol_r = (1e-6, 1e-8) if precision == "f64" else (3e-5, 4e-5)
    steps = T if precision == "f64" else 600
    for t in range(steps):
        obs, rew, term, trunc, _ = env.step(torch.from_numpy(g["actions"][:, t:t + 1]).cuda())
        obs, rew, term = to_np(obs, rew, term)
        m = alive
        if not m.any():
            break
        worst_o = max(worst_o, float(np.abs(obs[m] - g["final_obs"][m, t]).max()))
        worst_r = max(worst_r, float(np.abs(rew[m] - g["reward"][m, t]).max()))
        np.testing.assert_array_equal(term[m], g["done"][m, t], err_msg=f"t={t}")
        alive = alive & ~g["done"][:, t]
    print(f"\n[golden {env_id} {precision}] max |obs| err {worst_o:.3e}, max |rew| err {worst_r:.3e}")
    assert worst_o <= tol_o and worst_r <= tol_r
    env.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("env_id,family,fname", LEGACY_F64)
def test_legacy_f64_single_step_parity_4096(env_id, family, fname, precision):
    """4096 envs scattered by 60 oracle steps (with resets), state injected, three steps with
    same-step autoreset; terminal rows come from final_obs."""
    n = 4096
    o = O.LegacyF64Batch(n, family)
    o.reset(list(range(n)))
    rng = np.random.default_rng(4)
    bias = np.where(np.arange(n) % 2 == 0, 1.3, -1.3)          # drive half the envs off the path
    for _ in range(60):
        _, _, dn = o.step(np.clip(bias + rng.normal(0, 0.3, n), -np.pi / 2, np.pi / 2).astype(np.float32))
        if dn.any():
            o.reset(idx=np.flatnonzero(dn))
    # every 8th env a few mm inside |ye| = 10 (ak = 0, so ye = y - y_0): episodes end in-kernel
    edge = np.arange(0, n, 8)
    o.target[edge, 1] = o.position[edge, 1] - np.where(edge % 16 == 0, 9.997, -9.997)
    env = make(env_id, n, precision=precision, autoreset=True)
    dones = 0
    for k in range(3):
        _legacy_inject(env, o)
        a = rng.uniform(-np.pi / 2, np.pi / 2, n).astype(np.float32)
        obs, rew, term, trunc, info = env.step(torch.from_numpy(a).cuda())
        g_obs, g_rew, g_term, g_fobs = to_np(obs, rew, term, info["final_obs"])
        o_obs, o_rew, o_done = o.step(a)
        assert (g_term != o_done).sum() <= 1
        ok = g_term == o_done
        rows = np.where((g_term & ok)[:, None], g_fobs, g_obs)
        tol = 1e-6 if precision == "f64" else 2e-4
        err = np.abs(rows[ok] - o_obs[ok])
        rerr = np.abs(g_rew[ok] - o_rew[ok]).max()
        print(f"[{env_id} {precision} round {k}] obs max err {err.max():.3e}, reward max err "
              f"{rerr:.3e}, done {int(o_done.sum())}")
        assert err.max() <= tol
        assert rerr <= (1e-9 if precision == "f64" else 1e-3)
        dones += int(o_done.sum())
        if o_done.any():
            o.reset(idx=np.flatnonzero(o_done))
    assert dones > 0
    env.close()


@pytest.mark.parametrize("env_id,family,fname", LEGACY_F64)
def test_legacy_f64_reset_distribution(env_id, family, fname):
    from scipy import stats
    n = 8192
    env = make(env_id, n, seed=6)
    obs, _ = env.reset(seed=6)
    (obs,) = to_np(obs)
    g = env.get_state()
    o = O.LegacyF64Batch(n, family)
    o_obs = o.reset(list(range(n)))
    tg = g["v0_target"]
    for name, a, b in (("x", g["x"], o.position[:, 0]), ("y", g["y"], o.position[:, 1]),
                       ("psi", g["psi"], o.position[:, 2]), ("x0", tg[:, 0], o.target[:, 0]),
                       ("speed", tg[:, 2], o.target[:, 2]), ("x_d", tg[:, 4], o.target[:, 4]),
                       ("ye", obs[:, 3], o_obs[:, 3])):
        p = stats.ks_2samp(a, b).pvalue
        print(f"KS {env_id} {name}: p={p:.3g}")
        assert p > 1e-4, name
    assert np.all(g["v0_ye"] == 0) and np.all(obs[:, [0, 1, 2, 5]] == 0)
    env.close()


# --------------------------------------------------------------------------- NumPy-exact reset
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("fname,env_id", [("simple_traj.npz", "usv-simple"), ("simple_traj_tl.npz", "usv-simple"),
                                          ("asmc_simple_traj.npz", "usv-asmc-simple")])
def test_np_reset_full_trajectory(golden, fname, env_id, precision):
    """reset_rng="numpy": every env draws its resets from its own Generator(PCG64(SeedSequence(
    seed))) in the reference's order (simple_env.py:228-308), so the reference's rollouts replay
    whole, across TimeLimit truncations and terminations with same-step autoreset.
    f64: the seeded reset state equals the reference's exactly and the full rollout matches it bit for
    bit in every obs row, the sign of a reset row's zero ye included, with the reward within 2e-14; f32: the reset state is the reference's rounded to float32."""
    g = golden(fname)
    n, T = g["actions"].shape[:2]
    limit = int(g["limit"])
    env = make(env_id, n, precision=precision, max_episode_steps=max(limit, 0), reset_rng="numpy")
    obs, _ = env.reset(seed=g["seeds"])
    (obs,) = to_np(obs)
    st = env.get_state()
    ref = golden_state(g)
    keys = ("x", "y", "psi", "u", "v", "r", "path_x0", "path_y0", "path_x1", "path_y1", "max_u",
            "max_r", "ref_v", "obs_x", "obs_y", "obs_r")
    np.testing.assert_array_equal(st["n_obs"], ref["n_obs"])
    for k in keys:
        want = np.asarray(ref[k], dtype=np.float64)
        if precision == "f32":
            want = want.astype(np.float32).astype(np.float64)
        np.testing.assert_array_equal(st[k], want, err_msg=k)
    if precision == "f64":
        np.testing.assert_array_equal(obs, g["obs0"])
        assert bits_off(obs, g["obs0"]) == 0
    else:
        np.testing.assert_allclose(obs, g["obs0"], atol=2e-6, rtol=0)
        env.close()
        return
    worst = {"obs": 0.0, "fobs": 0.0, "rew": 0.0}
    resets = off = 0
    for t in range(T):
        o, r, te, tr, info = env.step(torch.from_numpy(g["actions"][:, t]).cuda())
        o, r, te, tr, fo = to_np(o, r, te, tr, info["final_obs"])
        np.testing.assert_array_equal(te, g["terminated"][:, t], err_msg=f"t={t}")
        np.testing.assert_array_equal(tr, g["truncated"][:, t], err_msg=f"t={t}")
        done = te | tr
        resets += int(done.sum())
        worst["obs"] = max(worst["obs"], float(np.abs(o - g["obs"][:, t]).max()))
        worst["rew"] = max(worst["rew"], float(np.abs(r - g["reward"][:, t]).max()))
        off += bits_off(o, g["obs"][:, t])
        if done.any():
            worst["fobs"] = max(worst["fobs"], float(np.abs(fo[done] - g["final_obs"][done, t]).max()))
            off += bits_off(fo[done], g["final_obs"][done, t])
    print(f"\n[np-reset {fname} {env_id}] {resets} in-kernel resets over {n}x{T} steps; max err {worst}, "
          f"obs entries not bit-equal {off}")
    assert resets > 0
    assert worst["obs"] == 0 and worst["fobs"] == 0 and worst["rew"] <= F64_REW_TOL and off == 0, (worst, off)
    env.close()


def test_np_reset_single_env_api(golden):
    """gym_usv_amd.make(id, reset_rng="numpy") is the reference's env: reset(seed) and the same
    actions give its observations (usv-simple, TimeLimit 500, float64)."""
    import gym_usv_amd
    g = golden("simple_traj.npz")
    env = gym_usv_amd.make("usv-simple", precision="f64", reset_rng="numpy")
    obs, _ = env.reset(seed=int(g["seeds"][2]))
    assert bits_off(obs, g["obs0"][2]) == 0
    for t in range(40):
        obs, r, te, tr, _ = env.step(g["actions"][2, t])
        assert bits_off(obs, g["final_obs"][2, t]) == 0, t
        assert abs(r - g["reward"][2, t]) <= F64_REW_TOL and te == g["terminated"][2, t] and tr == g["truncated"][2, t]
        if te or tr:
            break
    env.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("env_id,fname", [("usv-asmc-v0", "asmc_v0_traj.npz"), ("usv-pid-v0", "pid_traj.npz"),
                                          ("usv-asmc-ye-int-v0", "asmc_ye_int_traj.npz")])
def test_np_reset_legacy_full_trajectory(golden, env_id, fname, precision):
    """Legacy ids with reset_rng="numpy": resets draw np.random.uniform from each env's
    RandomState MT19937 after np.random.seed(seed) (usv_asmc_env.py:258-279), so the reference's
    rollouts replay whole across their episode ends (reset on done).  f64: usv-pid-v0 /
    usv-asmc-ye-int-v0 obs bit-identical, usv-asmc-v0 within its float32-rounding tolerance;
    f32: the first 600 steps."""
    g = golden(fname)
    n, T = g["actions"].shape
    env = make(env_id, n, precision=precision, reset_rng="numpy")
    obs, _ = env.reset(seed=g["seeds"])
    (obs,) = to_np(obs)
    np.testing.assert_allclose(obs, g["obs0"], atol=1e-6 if precision == "f32" else 0, rtol=0)
    exact = precision == "f64" and env_id != "usv-asmc-v0"
    tol_o = 0.0 if exact else (5e-6 if precision == "f64" else 2e-3)
    steps = T if precision == "f64" else 600
    worst, ends = 0.0, 0
    for t in range(steps):
        o, r, te, tr, info = env.step(torch.from_numpy(g["actions"][:, t:t + 1]).cuda())
        o, r, te, fo = to_np(o, r, te, info["final_obs"])
        np.testing.assert_array_equal(te, g["done"][:, t], err_msg=f"t={t}")
        ends += int(te.sum())
        worst = max(worst, float(np.abs(o - g["obs"][:, t]).max()))
        if te.any():
            worst = max(worst, float(np.abs(fo[te] - g["final_obs"][te, t]).max()))
    print(f"\n[np-reset {env_id} {precision}] {ends} resets over {n}x{steps} steps, max |obs| err {worst:.3e}")
    assert worst <= tol_o
    if precision == "f64":
        assert ends == int(g["done"].sum()) > 0
    env.close()


def test_render_rgb_array_from_device_state():
    """render_mode="rgb_array" (simple_env.py:117-131): a frame from the env's device state with
    the boat at its position and the current scan's rays (gym_usv_amd/render.py)."""
    import gym_usv_amd
    env = gym_usv_amd.make("usv-simple", render_mode="rgb_array")
    env.reset(seed=3)
    env.step(np.array([0.6, 0.1], np.float32))
    img = env.render()
    st = env._venv.get_state()
    s = 512 / 20
    x, y, psi = st["x"][0], st["y"][0], st["psi"][0]
    assert img.shape == (512, 512, 3) and img.dtype == np.uint8
    # a boat pixel 9 px behind its centre (clear of the front marker and, unless the path runs
    # there, of the path line)
    col, row = int(round(x * s - 9 * np.cos(psi))), int(round(y * s - 9 * np.sin(psi)))
    assert tuple(img[row, col]) in {(255, 0, 0), (100, 0, 0)}
    assert (img == np.array([0, 255, 0], np.uint8)).all(axis=2).sum() > 100      # lidar rays
    env.close()
