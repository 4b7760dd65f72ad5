"""Directed edge states (tests/dynamics_scenes.py) through the step's dynamics: both acceleration and speed
clips, the progress clamp, the four field edges and the TimeLimit, the +-pi cut and the octant folds of
the angle to target, the ye reward's crossover and signed zeros, the f32 heading rebase with psi_d_last,
and the 0.05 m / 0.2 m compares.  Run on an MI355X: pytest -m gpu.

Every run injects the scenes with set_state into an autoreset-free handle and takes T = 3 steps.  Batches
that share a TimeLimit run as one launch (the timelimit batch alone has one); no scene is left out of
any comparison.

  a. every step kind gives the bits of the brute-force wave kernel: obs, reward, flags, info rows;
  b. a scene's outputs do not depend on where in the batch it sits, nor on the batch's size;
  c. f64 against the reference (tests/golden/dynamics_scenes.npz): obs bit for bit, flags exact;
  d. f32 against the reference within SURVEY 8(c), flags exact;
  e. the heading (and psi_d_last) the state interface returns after each step.
"""
import numpy as np
import pytest
import torch

import dynamics_scenes as DS

pytestmark = pytest.mark.gpu

BRUTE = "64,0,1"                     # fused wave kernel, brute loop, no blind-sector skip, no unroll
# epb,lid,kind of test_gpu_lidar_edges.VARIANTS and test_gpu_parity.test_step_variants_bit_identical:
# wave kernels, split scan, block queue in both block shapes and row-store layouts, f64 block-wide
# dynamics (usv-simple), the ASMC chain kernel in front of the block queue (kind 6, f32 usv-asmc-simple)
VARIANTS = {
    ("usv-simple", "f32"): (None, "32,3,1", "64,7,1", "16,7,2", "128,7,4", "128,7,5", "16,7,5", "128,263,5"),
    ("usv-asmc-simple", "f32"): (None, "32,3,1", "64,7,1", "16,7,2", "128,7,4", "128,7,5", "16,7,5", "128,263,5",
                                 "128,7,6", "16,7,6"),
    ("usv-simple", "f64"): (None, "32,3,1", "64,7,1", "64,7,2", "64,7,3", "32,7,3"),
    ("usv-asmc-simple", "f64"): (None, "32,3,1", "64,7,1", "64,7,2"),
}
CASES = [(e, p) for e in DS.ENV_IDS for p in ("f32", "f64")]
SHORT = {"usv-simple": "simple", "usv-asmc-simple": "asmc"}
F32_OBS_ATOL, F32_OBS_RTOL, F32_REW_ATOL = 1e-5, 1e-4, 1e-4      # SURVEY 8(c), as test_gpu_parity.py
ASMC_F32_HDR, ASMC_F32_REW = 1.5e-5, 1e-4                         # its f32 golden replay of usv-asmc-simple
# set from a measurement, 5x it: the angle to a target 1e-3 m away moves by 5e-4 rad with the float32 rounding
# of a 10 m coordinate (measured 6.2e-5 on obs[3] = angle / pi; usv-simple's 1e-5 + 1e-4 |ref| holds there)
ASMC_F32_HDR_FAMILY = {"angle": 3e-4}
F64_REW, F64_INFO = 2e-14, 5e-15                                   # DESIGN.md's parity table
YE_LEVER = 4 * 2.0 ** -53                                          # two ulps each on sin and cos of the path angle
PSI_TOL, PSI_D_TOL = 1e-6, 1e-5                                    # test_f32_heading_turns_roundtrip_and_spin
OUT_KEYS = ("obs", "rew", "term", "trunc", "info")
INFO_COLS = ("x", "y", "psi", "u", "v", "r", "path_x0", "path_y0", "path_x1", "path_y1") + DS.INFO_KEYS


def groups(precision, obstacles=True):
    """The batches of a precision as lists that share a TimeLimit: [(limit, [names])]."""
    by = {}
    for b in DS.batches(precision):
        if obstacles or b not in DS.WITH_OBSTACLES:
            by.setdefault(DS.batch(b)["limit"], []).append(b)
    return sorted(by.items())


def _stack(names, env_id):
    """One state dictionary, the actions and each batch's row slice for the concatenated batches."""
    sts = [DS.scene_state(DS.batch(b), env_id) for b in names]
    st = {k: (v if np.ndim(v) == 0 else np.concatenate([s[k] for s in sts])) for k, v in sts[0].items()}
    acts = np.concatenate([DS.batch(b)["actions"] for b in names])
    ends = np.cumsum([len(DS.batch(b)["x"]) for b in names])
    return st, acts, {b: slice(int(e - len(DS.batch(b)["x"])), int(e)) for b, e in zip(names, ends)}


def run(env_id, precision, limit, names, variant=None, order=None, fields=False, **kw):
    """T steps from the injected scenes (rows in `order`, if given): per output [n, T, ...] arrays."""
    import gym_usv_amd
    st, acts, _ = _stack(names, env_id)
    if order is not None:
        st = {k: (v if np.ndim(v) == 0 else v[order]) for k, v in st.items()}
        acts = acts[order]
    n = len(acts)
    env = gym_usv_amd.make_vec(env_id, n, device=0, precision=precision, autoreset=False, max_episode_steps=limit,
                               kernel_variant=variant, info=True, **kw)
    out = {k: [] for k in OUT_KEYS + (("psi", "psi_d_last") if fields else ())}
    try:
        env.set_state(st)
        for t in range(DS.T):
            obs, rew, term, trunc, _ = env.step(torch.from_numpy(np.ascontiguousarray(acts[:, t])).cuda())
            torch.cuda.synchronize()
            for k, v in zip(OUT_KEYS, (obs, rew, term, trunc, env.info_buf)):
                out[k].append(v.detach().cpu().numpy().copy())
            if fields:
                out["psi"].append(env.get_field("psi"))
                out["psi_d_last"].append(env.get_field("asmc")[:, 0].copy())
    finally:
        env.close()
    return {k: np.stack(v, axis=1) for k, v in out.items()}


_cache = {}


def brute(env_id, precision, limit, names):
    """The reference variant's run of a group, with the heading fields (computed once, read-only)."""
    key = (env_id, precision, limit, tuple(names))
    if key not in _cache:
        _cache[key] = run(env_id, precision, limit, names, BRUTE, fields=True)
        for v in _cache[key].values():
            v.setflags(write=False)
    return _cache[key]


def per_batch(env_id, precision):
    """{batch: the reference variant's outputs for its scenes}."""
    out = {}
    for limit, names in groups(precision):
        res, (_, _, rows) = brute(env_id, precision, limit, names), _stack(names, env_id)
        out.update({b: {k: v[rows[b]] for k, v in res.items()} for b in names})
    return out


def where(names, env_id, j):
    """describe() of row j of the concatenated batches."""
    for b, rows in _stack(names, env_id)[2].items():
        if rows.start <= j < rows.stop:
            return DS.describe(b, j - rows.start)


def same_bits(got, ref, names, env_id, label, order=None, keys=OUT_KEYS):
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k] if order is None else ref[k][order])
        assert a.shape == b.shape and a.dtype == b.dtype, (label, k)
        w = a.dtype.itemsize
        bad = a.view(f"u{w}") != b.view(f"u{w}")
        if bad.any():
            idx = tuple(int(v) for v in np.argwhere(bad)[0])
            j = idx[0] if order is None else int(order[idx[0]])
            pytest.fail(f"{label}: {k}{list(idx[2:])} differs in {int(bad.sum())} of {bad.size} entries; first in step "
                        f"{idx[1] + 1}: {a[idx]!r} vs {b[idx]!r}; {where(names, env_id, j)}")


def fixture(golden, name, env_id):
    g = golden("dynamics_scenes.npz")
    pre = f"{name}__{SHORT[env_id]}__"
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


# --------------------------------------------------------------------------- a. bitwise across kernels
@pytest.mark.parametrize("env_id,precision", CASES)
def test_variants_bitwise(env_id, precision):
    """Every step kind runs the same env_dynamics, so each gives the brute-force wave kernel's bits: obs,
    reward, flags and info rows; so do the scan-free step on the families without obstacles (their one
    obstacle is out of range: sensors 1.0, no penalty, no termination either way) and the vmcnt(0) build."""
    from gym_usv_amd import _lib
    for limit, names in groups(precision):
        ref = brute(env_id, precision, limit, names)
        assert np.isfinite(ref["obs"]).all() and np.isfinite(ref["rew"]).all() and np.isfinite(ref["info"]).all()
        for v in VARIANTS[env_id, precision]:
            same_bits(run(env_id, precision, limit, names, v), ref, names, env_id, f"{env_id} {precision} variant {v or 'default'}")
        same_bits(run(env_id, precision, limit, names, lib_path=_lib.SAFE_LIB_PATH), ref, names, env_id,
                  f"{env_id} {precision} libusvhip_safe.so")
    own = per_batch(env_id, precision)
    for limit, names in groups(precision, obstacles=False):
        ref = {k: np.concatenate([own[b][k] for b in names]) for k in OUT_KEYS}
        assert np.all(ref["obs"][:, :, 15:] == np.float32(1.0)) and not ref["term"].any()
        same_bits(run(env_id, precision, limit, names, ignore_obstacles=True), ref, names, env_id,
                  f"{env_id} {precision} ignore_obstacles")


# --------------------------------------------------------------------------- b. batch-order invariance
@pytest.mark.parametrize("env_id,precision", CASES)
def test_batch_order_invariance(env_id, precision):
    """The scenes permuted, and padded with copies to 64 k + 1 envs: every row gives its scene's bits.  The
    dynamics are lane per env and must not see their neighbours, the wave's other half or a ragged tail."""
    for limit, names in groups(precision):
        own = brute(env_id, precision, limit, names)
        n = own["obs"].shape[0]
        perm = np.random.default_rng(n).permutation(n)
        total = 64 * (n // 64 + 1) + 1
        order = np.concatenate([perm, perm[np.arange(total - n) % n]])
        assert len(order) % 64 == 1 and set(order) == set(range(n))
        for v in ((None, "128,7,5", "16,7,5") if precision == "f32" else (None,)):
            same_bits(run(env_id, precision, limit, names, v, order), own, names, env_id,
                      f"{env_id} {precision} variant {v or 'default'} permuted and padded", order)


# --------------------------------------------------------------------------- c. f64 against the reference
def f64_obs_close(got, ref, info_ref):
    """[n, T, 15] bool: header entries that are the reference's bits, or (obs[3] and obs[5] only) agree with it
    to float64 rounding.  Those two are differences of nearly equal terms, so an ulp that OCML's atan2 / sincos
    round differently from the reference's libm (obs[3]), or the step's dy/|d|, dx/|d| for sin / cos of the
    path angle (obs[5], usv_dynamics.hpp), shows in the float32 where the terms cancel: allowed is one float32
    ulp of the reference's value (two float64 values that agree to rounding round to the same or to
    neighbouring floats) or, where the value itself is a rounding residue, the float64 rounding of its terms:
    2 ulp(pi) / pi for the angle (either atan2 within an ulp), YE_LEVER per metre of |x - x0| + |y - y0| for ye / 10.
    A reference zero has no rounding in it: its sign must match."""
    same = got.view(np.uint32) == ref.view(np.uint32)
    r64 = ref.astype(np.float64)
    lever = np.abs(info_ref[:, :, 0] - info_ref[:, :, 6]) + np.abs(info_ref[:, :, 1] - info_ref[:, :, 7])
    floor = np.zeros(ref.shape)
    floor[:, :, 3] = 2 * np.spacing(np.pi) / np.pi
    floor[:, :, 5] = YE_LEVER * lever / 10.0
    tol = np.maximum(np.spacing(np.abs(ref)).astype(np.float64), floor)
    near = (np.abs(got.astype(np.float64) - r64) <= tol) & (r64 != 0)
    near[:, :, [j for j in range(15) if j not in (3, 5)]] = False
    return same, same | near


@pytest.mark.parametrize("env_id", DS.ENV_IDS)
def test_f64_against_fixture(golden, env_id):
    """obs header bit for bit, signed zeros included, but for obs[3] and obs[5] where their terms cancel
    (f64_obs_close; the entries that differ are counted and printed), the contact batches' sensor rows bit
    for bit; flags exact with no tolerated mismatch; reward <= 2e-14 and info rows <= 5e-15 relative to
    max(1, |ref|), DESIGN.md's own bounds for the f64 build.  The info row's ye gets YE_LEVER per metre of
    |x - x0| + |y - y0| on top (sin and cos of the path angle by either route carry up to two ulps each:
    past the end of a 200 m path that is 1e-13 m), and ye_reward that times its slope.
    Measured: reward 1.5e-14, info 1.8e-15 but ye 2.8e-14 (2.0e-16 per metre) and ye_reward 1.5e-14; obs[3]
    off in 2 scenes (angle 3e-14 pi: 3.5e-17), obs[5] in 1 (ye -7e-16: 1.1e-17), of 343 scenes x 3 steps."""
    fails = []
    for name, got in per_batch(env_id, "f64").items():
        ref = fixture(golden, name, env_id)
        rew = np.abs(got["rew"] - ref["reward"])
        info = np.abs(got["info"] - ref["info"])
        tol = F64_INFO * np.maximum(1.0, np.abs(ref["info"]))
        lever = np.abs(ref["info"][:, :, 0] - ref["info"][:, :, 6]) + np.abs(ref["info"][:, :, 1] - ref["info"][:, :, 7])
        ye, ye_r = ref["info"][:, :, INFO_COLS.index("ye")], ref["info"][:, :, INFO_COLS.index("ye_reward")]
        tol[:, :, INFO_COLS.index("ye")] += YE_LEVER * lever
        tol[:, :, INFO_COLS.index("ye_reward")] += YE_LEVER * lever * np.maximum(1.0, 2 * np.abs(ye / DS.YE_K)) * ye_r / DS.YE_K
        same, close = f64_obs_close(got["obs"][:, :, :15], ref["hdr"], ref["info"])
        bad = [(f"obs[{j}]", ~close[:, :, j]) for j in range(15)]
        if name in DS.WITH_OBSTACLES:
            bad.append(("sensors", got["obs"][:, :, 15:].view(np.uint32) != ref["sensors"].view(np.uint32)))
        else:
            assert np.all(got["obs"][:, :, 15:] == np.float32(1.0))
        bad += [("terminated", got["term"].astype(bool) != ref["terminated"]), ("truncated", got["trunc"].astype(bool) != ref["truncated"]),
                ("reward", rew > F64_REW)] + [(f"info {k}", info[:, :, j] > tol[:, :, j]) for j, k in enumerate(INFO_COLS)]
        rel = info / np.maximum(1.0, np.abs(ref["info"]))
        print(f"[{env_id} f64 {name}] reward max err {rew.max():.2e}, info max rel err {rel.max():.2e} "
              f"({INFO_COLS[int(np.argmax(rel.max(axis=(0, 1))))]}), header entries not bit-equal: "
              + (", ".join(f"obs[{j}] {int((~same[:, :, j]).sum())}" for j in range(15) if not same[:, :, j].all()) or "none"))
        for what, b in bad:
            if b.any():
                idx = np.argwhere(b)[0]
                fails.append(f"{name}: {what} off in {int(b.sum())} of {b.size} entries, first in step {int(idx[1]) + 1}; "
                             f"{DS.describe(name, int(idx[0]))}")
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------------- d. f32 against the reference
@pytest.mark.parametrize("env_id", DS.ENV_IDS)
def test_f32_against_fixture(golden, env_id):
    """Header within SURVEY 8(c) (usv-asmc-simple: the bounds of its f32 golden replay), obs[3] on the
    circle since wrap_angle<float> may land a rounding beyond +-pi, its sign too where the reference's
    |angle| <= pi - 1e-3 (and above the header's own tolerance: the sign of a zero is not an f32 property);
    reward <= 1e-4; flags exact on every scene: the scenes keep their margins for that."""
    fails = []
    for name, got in per_batch(env_id, "f32").items():
        ref = fixture(golden, name, env_id)
        hdr, want = got["obs"][:, :, :15].astype(np.float64), ref["hdr"].astype(np.float64)
        err = np.abs(hdr - want)
        err[:, :, 3] = np.minimum(err[:, :, 3], 2.0 - err[:, :, 3])
        tol = F32_OBS_ATOL + F32_OBS_RTOL * np.abs(want) if env_id == "usv-simple" else np.full_like(want, ASMC_F32_HDR_FAMILY.get(name, ASMC_F32_HDR))
        rerr = np.abs(got["rew"].astype(np.float64) - ref["reward"])
        rtol = F32_REW_ATOL if env_id == "usv-simple" else ASMC_F32_REW
        signed = (np.abs(want[:, :, 3]) <= 1.0 - 1e-3 / np.pi) & (np.abs(want[:, :, 3]) > tol[:, :, 3])
        flips = signed & (np.sign(hdr[:, :, 3]) != np.sign(want[:, :, 3]))
        print(f"[{env_id} f32 {name}] header max err {err.max():.2e} (obs[{int(np.argmax(err.max(axis=(0, 1))))}]), "
              f"reward max err {rerr.max():.2e}, angle sign flips {int(flips.sum())}")
        for what, bad in (("header", err > tol), ("reward", rerr > rtol), ("angle sign", flips),
                          ("terminated", got["term"].astype(bool) != ref["terminated"]),
                          ("truncated", got["trunc"].astype(bool) != ref["truncated"])):
            if bad.any():
                i = int(np.argwhere(bad)[0][0])
                fails.append(f"{name}: {what} off in {int(bad.sum())} entries, first {np.argwhere(bad)[0].tolist()}; "
                             f"{DS.describe(name, i)}")
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------------- e. the heading state
@pytest.mark.parametrize("env_id,precision", CASES)
def test_heading_state_after_each_step(env_id, precision):
    """get_field("psi") is the oracle's unwrapped heading within 1e-6 on the circle with no whole turn between
    them (the f32 build returns phi + 2 pi k: a lost or doubled rebase is a whole turn), and usv-asmc-simple's
    psi_d_last is within 1e-5 of the oracle's."""
    fails = []
    for name, got in per_batch(env_id, precision).items():
        tr = DS.trace(name, env_id)
        d = got["psi"] - tr["psi"]
        turns = np.rint(d / (2 * np.pi))
        err = np.abs(d - 2 * np.pi * turns)
        perr = np.abs(got["psi_d_last"] - tr["psi_d_last"]) if env_id == "usv-asmc-simple" else np.zeros_like(err)
        print(f"[{env_id} {precision} {name}] psi max err {err.max():.2e}, whole turns off {int((turns != 0).sum())}, "
              f"psi_d_last max err {perr.max():.2e}")
        for what, bad in (("whole turns", turns != 0), ("psi", err > PSI_TOL), ("psi_d_last", perr > PSI_D_TOL)):
            if bad.any():
                fails.append(f"{name}: {what} off in {int(bad.sum())} entries; {DS.describe(name, int(np.argwhere(bad)[0][0]))}")
    assert not fails, "\n".join(fails)
