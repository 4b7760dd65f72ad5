"""Directed edge scenes (tests/lidar_scenes.py) through every lidar kernel: obstacles on the window
kernels' branch cut, either side of the `wide` / `inside` thresholds, on the blind sector's edges,
readings that straddle max range, and pair lists of up to 128 passes.  Run on an MI355X: pytest -m gpu.

Step kernels: zero velocity and zero action keep the injected pose bit for bit, so obs[:, 15:] is the
scan of the scene (reading / 100).  Reset kernel: set_state + reset() + sensor_last.

  a. every step variant and the reset kernel give the bits of the brute loop without pruning (lid 0);
  b. a reading does not depend on the env's wave companion (two-env-per-wave kernels);
  c. readings equal the float64 oracle on clear rays (lidar_scenes: the clear-ray rule), no flips;
  d. closed forms that do not go through the oracle: an obstacle on ray k reads d - r on ray k, one
     deep in the blind sector leaves all 128 rays at max range.
"""
import numpy as np
import pytest
import torch

import lidar_scenes as LS

pytestmark = pytest.mark.gpu

BRUTE = "64,0,1"                     # fused wave kernel, brute loop, no blind-sector skip, no unroll
# epb,lid,kind: lidar_brute with / without skip and unroll, lidar_window (cap 64) / lidar_window2 in the
# wave and block-queue kernels (both block shapes, both row-store layouts), lidar_window_d / lidar_wave2_d
VARIANTS = {
    ("f32", 32): (None, "32,3,1", "64,7,1", "16,7,2", "128,7,4", "128,7,5", "16,7,5", "128,263,5"),
    ("f64", 32): (None, "32,3,1", "64,7,1", "64,7,2", "64,7,3", "32,7,3"),
    ("f32", 64): (None, "32,3,1", "64,7,1", "16,7,2"),
    ("f64", 64): (None, "32,3,1", "64,7,1", "16,7,2", "64,7,2"),
}
CASES = [("sweep", 32), ("sweep", 64), ("lists32", 32), ("single32", 32), ("lists64", 64), ("range", 32),
         ("range", 64)]
F64_TOL = 1e-10                      # metres, the f64 figure of test_gpu_r2.py
F32_ATOL, F32_RTOL = 1e-3, 1e-4      # check_readings of test_gpu_r2.py


def make(n, **kw):
    import gym_usv_amd
    return gym_usv_amd.make_vec("usv-simple", n, device=0, autoreset=False, **kw)


def step_scan(name, precision, cap, variant, order=None):
    """obs[:, 15:] (float32, reading / 100) of one zero-action step from the injected scenes."""
    st = LS.scene_state(LS.batch(name), cap, order)
    n = len(st["n_obs"])
    env = make(n, precision=precision, obstacle_cap=cap, max_episode_steps=0, kernel_variant=variant)
    try:
        env.set_state(st)
        obs, *_ = env.step(torch.zeros(n, 2, device="cuda"))
        torch.cuda.synchronize()
        return obs[:, 15:].detach().cpu().numpy().copy()
    finally:
        env.close()


_cache = {}


def brute_scan(name, precision, cap):
    key = ("step", name, precision, cap)
    if key not in _cache:
        _cache[key] = step_scan(name, precision, cap, BRUTE)
        _cache[key].setflags(write=False)
    return _cache[key]


def reset_scan(name, precision, cap):
    """sensor_last (metres, float64 array) after the reset kernel rescanned the injected pose."""
    key = ("reset", name, precision, cap)
    if key not in _cache:
        st = LS.scene_state(LS.batch(name), cap)
        env = make(len(st["n_obs"]), precision=precision, obstacle_cap=cap)
        try:
            env.set_state(st)
            env.reset()
            _cache[key] = env.get_field("sensor_last")
        finally:
            env.close()
        _cache[key].setflags(write=False)
    return _cache[key]


def same_bits(got, ref, name, label, order=None):
    bad = got.view(np.uint32) != ref.view(np.uint32)
    if bad.any():
        j, k = (int(v) for v in np.argwhere(bad)[0])
        i = j if order is None else int(order[j])
        pytest.fail(f"{label}: {int(bad.sum())} of {bad.size} readings differ; first: {100.0 * got[j, k]!r} vs "
                    f"{100.0 * ref[j, k]!r} m; {LS.describe(name, i, k)}")


def close_to(got, want, mask, precision, name, label):
    """got, want [n, 128] metres; every masked ray within the precision's tolerance."""
    err = np.abs(got - want)
    tol = np.full_like(want, F64_TOL) if precision == "f64" else F32_ATOL + F32_RTOL * np.abs(want)
    bad = mask & ~(err <= tol)
    print(f"\n[{label}] {int(mask.sum())} of {mask.size} rays checked, max |err| {err[mask].max():.3e} m, "
          f"mismatches {int(bad.sum())}")
    if bad.any():
        i, k = (int(v) for v in np.argwhere(bad)[0])
        pytest.fail(f"{label}: {int(bad.sum())} rays off; first: {got[i, k]!r} vs {want[i, k]!r} m; "
                    f"{LS.describe(name, i, k)}")


# --------------------------------------------------------------------------- a. bitwise identity
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name,cap", CASES)
def test_variants_bitwise(name, cap, precision):
    """All rays, no exclusions: every variant evaluates the brute loop's per-pair arithmetic, so each
    reproduces its float32 obs bits; and the reset kernel's sensor_last, normalised and rounded as the
    step does it (f32: x * 0.01f; f64: (float)(x / 100)), equals them too."""
    ref = brute_scan(name, precision, cap)
    assert np.isfinite(ref).all() and (ref < 1.0).any() and (ref == 1.0).any()
    for v in VARIANTS[precision, cap]:
        same_bits(step_scan(name, precision, cap, v), ref, name, f"{precision} cap {cap} variant {v or 'default'}")
    last = reset_scan(name, precision, cap)
    if precision == "f32":
        norm = last.astype(np.float32) * np.float32(0.01)
    else:
        norm = (last / 100.0).astype(np.float32)
    same_bits(norm, ref, name, f"{precision} cap {cap} reset kernel")


# --------------------------------------------------------------------------- b. companion invariance
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", ["sweep", "lists32", "range"])
def test_companion_invariance(name, precision):
    """Cap 32, two envs per wave: the batch rotated by one gives every env another companion and the
    other half of the wave; after un-permuting, the readings are the same bits.  Guards the slot
    re-arm, mark / mark2 and the record buffer against leaking between the envs of a wave or between
    consecutive pairs."""
    order = LS.partner_shuffle(LS.batch(name)["pos"].shape[0])
    # f32: both block shapes of the block-queue step by name (the default is one of them, by env count)
    for v in (("16,7,5", "128,7,5") if precision == "f32" else (None,)):
        own = step_scan(name, precision, 32, v)
        moved = step_scan(name, precision, 32, v, order)
        same_bits(moved, own[order], name, f"{precision} variant {v or 'default'} rotated batch", order)


# --------------------------------------------------------------------------- c. the oracle, clear rays
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name,cap", CASES)
def test_oracle_on_clear_rays(name, cap, precision):
    """No mismatch at all on clear rays.  f64 is checked at 1e-10 m on the reset kernel's float64
    sensor_last (the step's obs are float32, tied to it bit for bit by test_variants_bitwise) and at the
    float32 rounding on the step's obs; f32 at atol 1e-3 m + rtol 1e-4 on both."""
    want, clear = LS.reference(name), LS.clear_rays(name)
    last = reset_scan(name, precision, cap)
    obs = brute_scan(name, precision, cap)
    close_to(last, want, clear, precision, name, f"{name} cap {cap} {precision} reset vs oracle")
    if precision == "f64":
        bad = clear & ~(np.abs(obs - (want / 100).astype(np.float32)) <= 6e-8)
        assert not bad.any(), LS.describe(name, *(int(v) for v in np.argwhere(bad)[0]))
    else:
        close_to(obs.astype(np.float64) * 100.0, want, clear, precision, name, f"{name} cap {cap} f32 step vs oracle")


# --------------------------------------------------------------------------- d. closed forms
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("cap", [32, 64])
def test_sweep_closed_forms(cap, precision):
    """Family 1 without the oracle: an obstacle whose bearing is exactly ray k (k in 0..127, r < d)
    reads d - r on ray k; one in the open blind sector, more than its angular half-width + 2 rays from
    rays 0 and 127, leaves all 128 rays at exactly 100.  Pins ray indexing, sweep direction and the
    heading convention."""
    sc = LS.batch("sweep")
    last = reset_scan("sweep", precision, cap)
    obs = brute_scan("sweep", precision, cap)
    r = sc["orad"][:, 0]
    d = np.array([LS.SWEEP_RATIOS[g][2] for g in sc["ratio"]])
    th = sc["theta"] % 192.0
    outside = r < d
    on_ray = outside & (th == np.round(th)) & (th <= 127)
    rows = np.flatnonzero(on_ray)
    assert len(rows) >= 128 * 3 * 8
    k = th[rows].astype(int)
    want = np.full_like(last, np.nan)
    mask = np.zeros(last.shape, bool)
    want[rows, k], mask[rows, k] = (d - r)[rows], True
    close_to(last, np.where(mask, want, 0.0), mask, precision, "sweep", f"sweep cap {cap} {precision} ray k reads d - r")
    if precision == "f32":
        close_to(obs.astype(np.float64) * 100.0, np.where(mask, want, 0.0), mask, precision, "sweep",
                 f"sweep cap {cap} f32 step, ray k reads d - r")
    hw = np.arcsin(np.where(outside, r / d, 1.0)) / LS.RES
    blind = outside & (th - 127.0 > hw + 2.0) & (192.0 - th > hw + 2.0)
    assert blind.sum() >= 1000 and len(set(sc["ratio"][blind])) >= 7
    assert (last[blind] == 100.0).all() and (obs[blind] == 1.0).all()
