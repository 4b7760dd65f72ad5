"""The directed lidar scenes (tests/lidar_scenes.py) are what they claim, checked on the host: the
clear-ray filter stays small, keys are distinct, the pair lists reach their lengths, the family 1
ratios straddle the window kernels' thresholds, and family 4 has fall-through rays.  No GPU."""
import numpy as np
import pytest

import lidar_scenes as LS


def _unclear_share(name, rows=slice(None)):
    return 1.0 - float(LS.clear_rays(name)[rows].mean())


def test_clear_rule_caps():
    """The rule may remove at most 2 % of a family's rays and 5 % of one ratio group of family 1;
    families 2 and 3 lose none (half-ray bearing offsets keep every ray clear of perpendicular)."""
    shares = {name: _unclear_share(name) for name in LS.BATCHES}
    ratio = LS.batch("sweep")["ratio"]
    groups = {lab: _unclear_share("sweep", ratio == g) for g, (lab, _, _) in enumerate(LS.SWEEP_RATIOS)}
    print("\n[unclear rays] " + ", ".join(f"{k} {100 * v:.2f}%" for k, v in shares.items()))
    print("[unclear rays, sweep by r/d] " + ", ".join(f"{k} {100 * v:.2f}%" for k, v in groups.items()))
    for name, v in shares.items():
        assert v <= 0.02, (name, v)
    for lab, v in groups.items():
        assert v <= 0.05, (lab, v)
    for name in ("lists32", "single32", "lists64"):
        assert shares[name] == 0.0, name


@pytest.mark.parametrize("name", LS.BATCHES)
def test_keys_distinct(name):
    """Keys d - r within an env differ by >= 1e-3 m (an exact tie's winner is unspecified)."""
    key = np.sort(LS.geometry(name)["key"], axis=1)
    with np.errstate(invalid="ignore"):              # inf - inf between padding entries
        gap = np.diff(key, axis=1)
    gap = gap[np.isfinite(gap)]
    assert gap.size == 0 or gap.min() >= 1e-3, gap.min()


@pytest.mark.parametrize("name", LS.BATCHES)
def test_hits_and_max_range_in_every_batch(name):
    ref = LS.reference(name)
    assert (ref < LS.MAX_RANGE).any() and (ref == LS.MAX_RANGE).any()
    sc = LS.batch(name)
    assert np.hypot(sc["pos"][:, 0] - 10, sc["pos"][:, 1] - 10).max() < 10      # poses inside the field
    assert {0.0, -17.3} <= set(sc["pos"][:, 2]) or sc["pos"].shape[0] == 1
    assert sc["pos"].shape[0] <= 41000                 # a launch of milliseconds


def test_sweep_ratios_straddle_the_thresholds():
    """Under the kernel's sizing formula in float32 the `wide` ratios sit either side of hr = 32.0 (f32)
    and 32.5 (f64), the inside ratios either side of d <= 1.001 r, and the smallest ratio's window
    holds at most one ray."""
    hr = {lab: float(LS.hr_f32(np.float32(r) / np.float32(d))) for lab, r, d in LS.SWEEP_RATIOS}
    print("\n[hr, rays] " + ", ".join(f"{k} {v:.3f}" for k, v in hr.items()))
    assert hr["wide32-"] < 32.0 <= hr["wide32+"] < hr["wide64-"] < 32.5 <= hr["wide64+"]
    assert hr["wide32+"] - hr["wide32-"] < 0.5 and hr["wide64+"] - hr["wide64-"] < 0.5   # close to the switch
    assert hr["8.3e-4"] < 0.5 and hr["0.02"] < 1.0 and hr["0.16"] < 32.0 and hr["0.9"] >= 32.5
    geo = {lab: (r, d) for lab, r, d in LS.SWEEP_RATIOS}
    # `wrap`: wide in both precisions, short of 40 rays, and truly wider than the 32.5 rays to the cut
    assert 32.5 <= hr["wrap"] < 40.0 and np.arcsin(geo["wrap"][0] / geo["wrap"][1]) / LS.RES > 33.0
    for prec in (np.float32, np.float64):
        r, d = geo["1/1.002"]
        assert not prec(d) <= prec(r) * prec(1.001)
        r, d = geo["1/1.0005"]
        assert prec(d) <= prec(r) * prec(1.001) and d > r
    r, d = geo["2"]
    assert d < r
    # the sweep reaches the edges it is for: integer bearings, both blind-sector edges, the branch cut
    th = LS.sweep_thetas() % 192.0
    for edge in (0.0, 127.0, 159.5):
        near = np.abs((th - edge + 96.0) % 192.0 - 96.0)
        assert (near <= 1 / 16).sum() >= 3, edge
    assert set(np.arange(128.0)) <= set(th)


def test_list_lengths():
    """Host pair counts: a wave of family 2 holds 128 (kA + kB) pairs, from 0 to 128 passes of 64;
    there is a zero-pair companion, and the interleaved envs' first obstacle has no pairs while their
    wide runs start off multiples of 64."""
    sc = LS.batch("lists32")
    cnt = LS.window_pairs("lists32")
    per_env = cnt.sum(1)
    n2 = len(sc["ka"])
    wave = per_env[:2 * n2].reshape(n2, 2)
    plain = ~sc["inter"]
    np.testing.assert_array_equal(wave[plain, 0], 128 * sc["ka"][plain])
    np.testing.assert_array_equal(wave[plain, 1], 128 * sc["kb"][plain])
    assert wave.sum(1).max() == 128 * 64 and (wave.sum(1) >= 64 * 64).sum() >= 4     # >= 64 passes
    assert set(wave[plain].sum(1) // 64) >= {0, 2, 4, 6, 32, 62, 64, 66, 126, 128}
    assert ((wave[:, 0] == 0) & (wave[:, 1] >= 128 * 31)).any()                       # zero-pair companion
    assert ((wave[:, 1] == 0) & (wave[:, 0] >= 128 * 31)).any()
    assert sc["pos"].shape[0] % 2 == 1 and per_env[-1] == 128 * 32                    # the odd env out
    il = np.repeat(sc["inter"], 2)
    first = cnt[:2 * n2, 0]
    assert (first[il] == 0).all() and (sc["n_obs"][:2 * n2][il] >= 1).all()          # lane 0 has no pairs
    # A wave's list is env A's lanes, then env B's.  Every wide run (128 pairs) that follows a narrow
    # obstacle in it starts off a multiple of 64 (the narrow ones before it hold 1..60 pairs in all),
    # every other one on a multiple; a wave's first wide run can only start at 0.
    c = cnt[:2 * n2].reshape(n2, -1)
    starts = np.cumsum(c, axis=1) - c
    narrow = (c > 0) & (c < 128)
    after_narrow = (np.cumsum(narrow, axis=1) - narrow) > 0
    wide = c == 128
    np.testing.assert_array_equal((starts % 64 != 0)[wide], after_narrow[wide])
    assert not narrow[plain].any()
    k_env = np.stack([sc["ka"], sc["kb"]], axis=1)
    np.testing.assert_array_equal(narrow.reshape(n2, 2, -1).any(2),
                                  sc["inter"][:, None] & (k_env >= 1) & (k_env <= 30))   # lanes left for them
    ka, kb = k_env[:, 0], k_env[:, 1]
    na, nb = (ka >= 1) & (ka <= 30), (kb >= 1) & (kb <= 30)          # the env has narrow obstacles
    expect = sc["inter"] & ((na & ((ka >= 2) | (kb >= 1))) | (~na & nb & (kb >= 2)))
    np.testing.assert_array_equal((wide & after_narrow).any(1), expect)
    assert (sc["n_obs"] <= 32).all() and sc["n_obs"].max() == 32
    one = LS.window_pairs("single32")
    assert one.shape[0] == 1 and one[0, 0] == 0 and one.sum() >= 128 * 24

    sc = LS.batch("lists64")
    cnt = LS.window_pairs("lists64")
    plain = ~sc["inter"]
    np.testing.assert_array_equal(cnt.sum(1)[plain], 128 * sc["k"][plain])
    assert (cnt[~plain, 0] == 0).all() and (cnt.sum(1)[~plain] >= 128 * np.minimum(sc["k"], 63)[~plain]).all()
    assert sc["n_obs"].max() == 64 and (sc["n_obs"] % 2 == 1).any()                   # brute's unroll padding


def test_range_family_falls_through():
    """Family 4 has rays whose min-key geometric hit reads >= 100 while the oracle reads a larger-key
    obstacle below 100 (usv_asmc_ca_env.py:458), on clear rays; and far / near envs alternate in both
    orders within a wave."""
    sc, g, ref = LS.batch("range"), LS.geometry("range"), LS.reference("range")
    geo_hit = g["valid"][:, None, :] & (g["proj"] >= 0) & (g["delta"] >= 0)
    kk = np.where(geo_hit, g["key"][:, None, :], np.inf)
    first = np.argmin(kk, axis=2)
    first_rd = np.take_along_axis(g["reading"], first[:, :, None], axis=2)[:, :, 0]
    fall = geo_hit.any(2) & (first_rd >= LS.MAX_RANGE) & (ref < LS.MAX_RANGE) & LS.clear_rays("range")
    assert fall.sum() >= 8, fall.sum()
    rejected = geo_hit.any(2) & (first_rd >= LS.MAX_RANGE) & (ref == LS.MAX_RANGE) & LS.clear_rays("range")
    assert rejected.sum() >= 4                       # a hit beyond max range with nothing behind it
    far_env = (g["valid"] & (g["d"] >= 99.0)).any(1)         # the envs that set a wave's `far` flag
    assert far_env[sc["is_far"]].sum() >= 24 and not far_env[~sc["is_far"]].any()
    pairs = far_env[:len(far_env) // 2 * 2].reshape(-1, 2)
    assert (pairs[:, 0] & ~pairs[:, 1]).any() and (~pairs[:, 0] & pairs[:, 1]).any()
    d = g["d"][g["valid"]]
    for v in (98.9, 99.1, 100.4, 101.0):
        assert np.isclose(d, v, atol=1e-9).any()


@pytest.mark.parametrize("name", ["sweep", "lists32", "range"])
def test_partner_shuffle_changes_every_partner(name):
    n = LS.batch(name)["pos"].shape[0]
    order = LS.partner_shuffle(n)
    assert sorted(order) == list(range(n))
    pos = np.empty(n, int)
    pos[order] = np.arange(n)                        # env i now sits at pos[i]
    for i in range(n):
        old = i ^ 1 if i ^ 1 < n else -1             # -1: no companion
        new = order[pos[i] ^ 1] if pos[i] ^ 1 < n else -1
        assert new != old, i
    assert (pos % 2 != np.arange(n) % 2).sum() >= n - 1      # and the other half of its wave
