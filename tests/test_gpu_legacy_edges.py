"""Directed edge states (tests/legacy_scenes.py) through the lane-per-env legacy step kernels: usv-asmc-v0
(v0_step_kernel), usv-asmc-ye-int-v0 and usv-pid-v0 (legacy_step_kernel).  Run on an MI355X: pytest -m gpu.

Every run injects the scenes with set_state into a handle with autoreset off and max_episode_steps at the
batch's limit, and takes the batch's steps (3, or 4 where a usv-asmc-v0 scene starts on the float64 reset state).
Batches that share a limit and a step count run as one launch.

  a. f64 build against the reference (tests/golden/legacy_scenes.npz): flags exact on every scene, obs and reward
     within test_gpu_parity.py's single-step bounds, obs entries that are not the reference's bits counted;
  b. f32 build against the reference within the f32 single-step bounds, flags exact;
  c. get_state() after every step against the reference's post-step state;
  d. a scene's bits do not depend on where in the batch it sits, nor on whether its wave takes the all-zero
     shortcut of v0_path_sincos or the libm arm;
  e. the vmcnt(0) build gives the default build's bits;
  f. same-step autoreset: final_obs, the done mask and the reset rows.
"""
import numpy as np
import pytest
import torch

import legacy_scenes as LS

pytestmark = pytest.mark.gpu

CASES = [(e, p) for e in LS.ENV_IDS for p in ("f32", "f64")]
# test_gpu_parity.py's single-step bounds: f64 obs, f64 reward (usv-asmc-v0 carries the reference's float32 rounding)
F64_OBS = {LS.V0: 2e-6, LS.YEINT: 1e-6, LS.PID: 1e-6}
F64_REW = {LS.V0: 1e-6, LS.YEINT: 1e-9, LS.PID: 1e-9}
F32_OBS, F32_REW = 2e-4, 1e-3
# f64 obs entries that are not the reference's float32 bits, per column, over all batches, as measured against the
# reference (test_f64_against_fixture): all three ids are bit-equal everywhere, so that is what is asserted
F64_NOT_BIT_EQUAL = {LS.V0: (0,) * 6, LS.YEINT: (0,) * 6, LS.PID: (0,) * 6}
OUT_KEYS = ("obs", "rew", "term", "trunc")
STATE_FIELDS = ("x", "y", "psi", "u", "v", "r", "v0_aux", "v0_last", "v0_action_last", "v0_ye", "elapsed")


def groups(env_id, precision, only=None):
    """The batches of an id and precision as lists that share a limit and a step count: [((limit, steps), [names])]."""
    by = {}
    for b in LS.batches(precision, env_id):
        if only is None or b in only:
            sc = LS.batch(b, env_id)
            by.setdefault((sc["limit"], sc["steps"]), []).append(b)
    return sorted(by.items())


def _stack(names, env_id):
    """One state dictionary, the actions and each batch's row slice for the concatenated batches."""
    sts = [LS.scene_state(LS.batch(b, env_id), env_id) for b in names]
    st = {k: np.concatenate([s[k] for s in sts]) for k in sts[0]}
    acts = np.concatenate([LS.batch(b, env_id)["actions"] for b in names])
    ends = np.cumsum([len(LS.batch(b, env_id)["x"]) for b in names])
    return st, acts, {b: slice(int(e - len(LS.batch(b, env_id)["x"])), int(e)) for b, e in zip(names, ends)}


def run(env_id, precision, limit, names, order=None, state=False, autoreset=False, **kw):
    """The batch's steps from the injected scenes (rows in `order`, if given): per output [n, S, ...] arrays;
    `state`: also the get_state() fields after every step; `autoreset`: also final_obs and the done mask."""
    import gym_usv_amd
    st, acts, _ = _stack(names, env_id)
    if order is not None:
        st, acts = {k: v[order] for k, v in st.items()}, acts[order]
    n = len(acts)
    env = gym_usv_amd.make_vec(env_id, n, device=0, precision=precision, autoreset=autoreset, max_episode_steps=limit, **kw)
    keys = OUT_KEYS + (("fobs", "done") if autoreset else ()) + (STATE_FIELDS if state else ())
    out = {k: [] for k in keys}
    try:
        env.set_state(st)
        for t in range(acts.shape[1]):
            obs, rew, term, trunc, info = env.step(torch.from_numpy(np.ascontiguousarray(acts[:, t])).cuda())
            torch.cuda.synchronize()
            vals = (obs, rew, term, trunc) + ((info["final_obs"], info["_final_obs"]) if autoreset else ())
            for k, v in zip(keys, vals):
                out[k].append(v.detach().cpu().numpy().copy())
            if state:
                got = env.get_state()
                for k in STATE_FIELDS:
                    out[k].append(got[k].copy())
    finally:
        env.close()
    return {k: np.stack(v, axis=1) for k, v in out.items()}


_cache = {}


def base(env_id, precision, limit, names):
    """The default build's run of a group with its state fields (computed once, read-only)."""
    key = (env_id, precision, limit, tuple(names))
    if key not in _cache:
        _cache[key] = run(env_id, precision, limit, names, state=True)
        for v in _cache[key].values():
            v.setflags(write=False)
    return _cache[key]


def per_batch(env_id, precision):
    """{batch: the default build's outputs and state fields for its scenes}."""
    out = {}
    for (limit, _), names in groups(env_id, precision):
        res, (_, _, rows) = base(env_id, precision, limit, names), _stack(names, env_id)
        out.update({b: {k: v[rows[b]] for k, v in res.items()} for b in names})
    return out


def where(names, env_id, j):
    for b, rows in _stack(names, env_id)[2].items():
        if rows.start <= j < rows.stop:
            return LS.describe(b, env_id, j - rows.start)


def same_bits(got, ref, names, env_id, label, order=None, keys=OUT_KEYS, rows=None):
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k] if order is None else ref[k][order])
        assert a.shape == b.shape and a.dtype == b.dtype, (label, k)
        w = a.dtype.itemsize
        bad = a.view(f"u{w}") != b.view(f"u{w}")
        if rows is not None:
            bad &= rows.reshape(rows.shape + (1,) * (bad.ndim - rows.ndim))
        if bad.any():
            idx = tuple(int(v) for v in np.argwhere(bad)[0])
            j = idx[0] if order is None else int(order[idx[0]])
            pytest.fail(f"{label}: {k}{list(idx[2:])} differs in {int(bad.sum())} of {bad.size} entries; first in step "
                        f"{idx[1] + 1}: {a[idx]!r} vs {b[idx]!r}; {where(names, env_id, j)}")


def _fails(name, env_id, checks):
    out = []
    for what, bad in checks:
        if bad.any():
            idx = np.argwhere(bad)[0]
            out.append(f"{name}: {what} off in {int(bad.sum())} of {bad.size} entries, first {idx[1:].tolist()} (step, column); "
                       f"{LS.describe(name, env_id, int(idx[0]))}")
    return out


def _flag_checks(got, ref):
    return [("terminated", got["term"].astype(bool) != ref["terminated"]), ("truncated", got["trunc"].astype(bool) != ref["truncated"])]


# --------------------------------------------------------------------------- a. f64 against the reference
@pytest.mark.parametrize("env_id", LS.ENV_IDS)
def test_f64_against_fixture(golden, env_id):
    """Flags exact on every scene with no tolerated mismatch; obs and reward within the f64 single-step bounds of
    test_gpu_parity.py (ye-int and pid: 1e-6 / 1e-9; v0: 2e-6 / 1e-6); obs entries that are not the reference's
    float32 bits counted per column and bounded at the measured count (F64_NOT_BIT_EQUAL).
    Measured: obs bit-equal on every scene step of every id (v0 556, ye-int 546, pid 462), which is asserted in place
    of a count; reward v0 1.1e-10, ye-int 3.3e-16, pid 2.2e-16.  No entry sits behind a transcendental that differs."""
    g = golden("legacy_scenes.npz")
    fails, off, total, worst_o, worst_r = [], np.zeros(6, np.int64), 0, 0.0, 0.0
    for name, got in per_batch(env_id, "f64").items():
        ref = LS.fixture(g, name, env_id)
        err = np.abs(got["obs"].astype(np.float64) - ref["obs"].astype(np.float64))
        rerr = np.abs(got["rew"] - ref["reward"])
        ne = got["obs"].view(np.uint32) != ref["obs"].view(np.uint32)
        off += ne.sum(axis=(0, 1))
        total += ne.shape[0] * ne.shape[1]
        worst_o, worst_r = max(worst_o, float(err.max())), max(worst_r, float(rerr.max()))
        print(f"[{env_id} f64 {name}] obs max err {err.max():.2e} (obs[{int(np.argmax(err.max(axis=(0, 1))))}]), reward max err "
              f"{rerr.max():.2e}, not bit-equal per column {ne.sum(axis=(0, 1)).tolist()} of {ne.shape[0] * ne.shape[1]}")
        fails += _fails(name, env_id, [("obs", err > F64_OBS[env_id]), ("reward", (rerr > F64_REW[env_id])[:, :, None])] +
                        [(k, b[:, :, None]) for k, b in _flag_checks(got, ref)])
    print(f"[{env_id} f64 all] obs max err {worst_o:.2e}, reward max err {worst_r:.2e}, not bit-equal per column "
          f"{off.tolist()} of {total} scene steps")
    assert not fails, "\n".join(fails)
    assert (off <= np.array(F64_NOT_BIT_EQUAL[env_id])).all(), (off.tolist(), F64_NOT_BIT_EQUAL[env_id])


# --------------------------------------------------------------------------- b. f32 against the reference
def _circle(err, ref):
    """Angle errors taken on the circle where the reference's |angle| is within 1e-3 of pi."""
    near = np.abs(np.abs(ref) - np.pi) <= 1e-3
    return np.where(near, np.minimum(err, np.abs(2 * np.pi - err)), err)


@pytest.mark.parametrize("env_id", LS.ENV_IDS)
def test_f32_against_fixture(golden, env_id):
    """Flags exact (the scenes keep their margins for that); obs <= 2e-4 and reward <= 1e-3, the f32 single-step
    bounds of test_gpu_parity.py; obs[4] = psi_ak on the circle where the reference's |psi_ak| is within 1e-3 of pi.
    Measured: v0 obs 4.8e-7, reward 1.3e-6; ye-int 9.5e-7, 1.6e-6; pid 4.8e-7, 1.6e-6."""
    g = golden("legacy_scenes.npz")
    fails, worst_o, worst_r = [], 0.0, 0.0
    for name, got in per_batch(env_id, "f32").items():
        ref = LS.fixture(g, name, env_id)
        want = ref["obs"].astype(np.float64)
        err = np.abs(got["obs"].astype(np.float64) - want)
        err[:, :, 4] = _circle(err[:, :, 4], want[:, :, 4])
        rerr = np.abs(got["rew"].astype(np.float64) - ref["reward"])
        worst_o, worst_r = max(worst_o, float(err.max())), max(worst_r, float(rerr.max()))
        print(f"[{env_id} f32 {name}] obs max err {err.max():.2e} (obs[{int(np.argmax(err.max(axis=(0, 1))))}]), "
              f"reward max err {rerr.max():.2e}")
        fails += _fails(name, env_id, [("obs", err > F32_OBS), ("reward", (rerr > F32_REW)[:, :, None])] +
                        [(k, b[:, :, None]) for k, b in _flag_checks(got, ref)])
    print(f"[{env_id} f32 all] obs max err {worst_o:.2e}, reward max err {worst_r:.2e}")
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------------- c. the state after each step
@pytest.mark.parametrize("env_id,precision", CASES)
def test_state_after_each_step(golden, env_id, precision):
    """get_state() after every step against the reference's position, velocity, aux_vars and last (ye_int and
    ye_last among them), at the obs bound of a (f64) or b (f32); the heading on the circle next to the cut;
    v0_action_last is the action; elapsed exactly.  These hold what the observation does not show: Ka_u, Ka_psi,
    e_u_int, Ka_dot_*_last, ye_int, ye_last.
    Measured: f64 v0 6.0e-8 (v0_last, else 0), ye-int 1.3e-15, pid 8.9e-16; f32 v0 1.4e-6, ye-int 3.4e-6, pid 1.9e-6."""
    g = golden("legacy_scenes.npz")
    tol = F64_OBS[env_id] if precision == "f64" else F32_OBS
    fails, worst = [], {}
    for name, got in per_batch(env_id, precision).items():
        ref, sc = LS.fixture(g, name, env_id), LS.batch(name, env_id)
        steps = ref["obs"].shape[1]
        pairs = [("x", ref["position"][:, :, 0]), ("y", ref["position"][:, :, 1]), ("psi", ref["position"][:, :, 2]),
                 ("u", ref["velocity"][:, :, 0]), ("v", ref["velocity"][:, :, 1]), ("r", ref["velocity"][:, :, 2]),
                 ("v0_aux", ref["aux"][:, :, :3]), ("v0_last", ref["last"][:, :, :9]),
                 ("v0_action_last", sc["actions"].astype(np.float64))]
        if env_id == LS.YEINT:
            pairs.append(("v0_ye", np.stack([ref["aux"][:, :, 3], ref["last"][:, :, 9]], axis=2)))
            z = ref["last"][:, :, 9] == 0              # a stored ye of zero keeps the reference's sign: -0.0 where ye came out so
            assert np.array_equal(np.signbit(got["v0_ye"][:, :, 1][z]), np.signbit(ref["last"][:, :, 9][z])), name
            assert name != "ye_int" or np.signbit(ref["last"][:, :, 9][z]).any()
        checks = []
        for k, want in pairs:
            err = np.abs(got[k].astype(np.float64) - want)
            if k == "psi":
                err = _circle(err, want)
            worst[k] = max(worst.get(k, 0.0), float(err.max()))
            checks.append((k, err.reshape(err.shape[0], steps, -1) > tol))
        el = sc["elapsed"][:, None].astype(np.int64) + np.arange(1, steps + 1)
        checks.append(("elapsed", (got["elapsed"] != el)[:, :, None]))
        fails += _fails(name, env_id, checks)
    print(f"[{env_id} {precision} state] max err " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------------- d. batch order and wave layout
@pytest.mark.parametrize("env_id,precision", CASES)
def test_batch_order_invariance(env_id, precision):
    """The scenes permuted, and padded with copies to 64 k + 1 envs: every row gives its scene's bits, outputs
    and state.  The step is lane per env and must not see its neighbours or a ragged last wave."""
    for (limit, _), names in groups(env_id, precision):
        own = base(env_id, precision, limit, names)
        n = own["obs"].shape[0]
        perm = np.random.default_rng(n).permutation(n)
        total = 64 * (n // 64 + 1) + 1
        order = np.concatenate([perm, perm[np.arange(total - n) % n]])
        assert len(order) % 64 == 1 and set(order) == set(range(n))
        same_bits(run(env_id, precision, limit, names, order, state=True), own, names, env_id,
                  f"{env_id} {precision} permuted and padded", order, keys=OUT_KEYS + STATE_FIELDS)


@pytest.mark.parametrize("env_id,precision", CASES)
def test_path_angle_shortcut_and_libm_arm_agree(env_id, precision):
    """v0_path_sincos takes sin = 0, cos = 1 when a wave-wide ballot finds ak == 0 in every lane, else libm in every
    lane.  Layout 1: every ak == 0 scene (either zero's sign) in waves that hold only such scenes, the shortcut;
    layout 2: the same scenes interleaved lane by lane with ak != 0 scenes, the libm arm for the same lanes.  Both
    end in a wave with one live lane, ak zero in the first and non-zero in the second, and both give the bits of
    the scenes' own run."""
    for (limit, _), names in groups(env_id, precision):
        own = base(env_id, precision, limit, names)
        ak = _stack(names, env_id)[0]["v0_target"][:, 3]
        z, nz = np.flatnonzero(ak == 0), np.flatnonzero(ak != 0)
        if not len(nz):
            continue
        assert len(z) and np.signbit(ak[z]).any() == ("path" in names)
        pad = lambda idx: np.concatenate([idx, idx[np.arange(-len(idx) % 64) % len(idx)]])
        alone = np.concatenate([pad(z), pad(nz), z[:1]])
        k = max(len(z), len(nz))
        mixed = np.stack([z[np.arange(k) % len(z)], nz[np.arange(k) % len(nz)]], axis=1).ravel()
        mixed = np.concatenate([mixed, pad(mixed)[len(mixed):], nz[:1]])
        for label, order in (("ak == 0 waves apart", alone), ("ak == 0 lanes interleaved", mixed)):
            assert len(order) % 64 == 1 and set(order) == set(range(len(ak)))
            waves = ak[order[:len(order) - 1]].reshape(-1, 64)
            if label.endswith("apart"):
                assert all((w == 0).all() or (w != 0).all() for w in waves) and ak[order[-1]] == 0
            else:
                assert all((w == 0).any() and (w != 0).any() for w in waves) and ak[order[-1]] != 0
            same_bits(run(env_id, precision, limit, names, order, state=True), own, names, env_id,
                      f"{env_id} {precision} {label}", order, keys=OUT_KEYS + STATE_FIELDS)


# --------------------------------------------------------------------------- e. the safe build
@pytest.mark.parametrize("env_id,precision", CASES)
def test_safe_build_bitwise(env_id, precision):
    """The vmcnt(0) build gives the default build's bits on every batch: outputs and state."""
    from gym_usv_amd import _lib
    for (limit, _), names in groups(env_id, precision):
        same_bits(run(env_id, precision, limit, names, state=True, lib_path=_lib.SAFE_LIB_PATH), base(env_id, precision, limit, names),
                  names, env_id, f"{env_id} {precision} libusvhip_safe.so", keys=OUT_KEYS + STATE_FIELDS)


# --------------------------------------------------------------------------- f. same-step autoreset
@pytest.mark.parametrize("env_id,precision", CASES)
def test_same_step_autoreset(env_id, precision):
    """The bounds and timelimit batches with autoreset on, followed until each row's first done: reward and flags
    are the autoreset-off run's, the done mask is term | trunc, final_obs of the done rows is that run's obs,
    rows that are not done are unchanged bit for bit (outputs and state), and done rows come back with
    elapsed == 0 and the reset's zero velocity, derivatives, integrators and action."""
    seen = 0
    for (limit, _), names in groups(env_id, precision, only=("bounds", "timelimit")):
        off = base(env_id, precision, limit, names)
        on = run(env_id, precision, limit, names, state=True, autoreset=True)
        n, steps = off["obs"].shape[:2]
        alive = np.ones(n, bool)
        for t in range(steps):
            step = lambda d, ks: {k: d[k][:, t:t + 1] for k in ks}
            done = (off["term"][:, t] | off["trunc"][:, t]).astype(bool)
            same_bits(step(on, ("rew", "term", "trunc")), step(off, ("rew", "term", "trunc")), names, env_id,
                      f"{env_id} {precision} autoreset step {t + 1}", keys=("rew", "term", "trunc"), rows=alive[:, None])
            assert np.array_equal(on["done"][alive, t].astype(bool), done[alive])
            same_bits({"obs": on["fobs"][:, t:t + 1]}, step(off, ("obs",)), names, env_id,
                      f"{env_id} {precision} final_obs step {t + 1}", keys=("obs",), rows=(alive & done)[:, None])
            same_bits(step(on, ("obs",) + STATE_FIELDS), step(off, ("obs",) + STATE_FIELDS), names, env_id,
                      f"{env_id} {precision} rows not done, step {t + 1}", keys=("obs",) + STATE_FIELDS, rows=(alive & ~done)[:, None])
            back = alive & done
            seen += int(back.sum())
            for k in ("u", "v", "r", "v0_aux", "v0_last", "v0_action_last", "v0_ye", "elapsed"):
                assert not on[k][back, t].any(), (k, t)
            assert np.all(on["obs"][back, t][:, [0, 1, 2, 5]] == 0)
            alive &= ~done
    assert seen >= 8
