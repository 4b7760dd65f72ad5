"""ignore_obstacles (gym_usv/envs/simple_env.py:49) on the GPU: the scan-free step against the reference's
trajectories, bitwise against the scanning step (both run the same env_dynamics), the row streaming at
awkward shapes, same-step autoreset, the run-time toggle, the scan_valid == 2 bookkeeping and the API.
Run on an MI355X: pytest -m gpu."""
import functools

import numpy as np
import pytest
import torch

from ignore_fixture import FIXTURE_IDS, FIXTURES, block, golden_state
from oracle import usv_oracle as O

pytestmark = pytest.mark.gpu

IDS = ["usv-simple", "usv-asmc-simple"]
PRECISIONS = ["f32", "f64"]
N_BIG, ROUNDS, WARM = 4099, 4, 25


def make(env_id, n, **kw):
    import gym_usv_amd
    return gym_usv_amd.make_vec(env_id, n, device=0, **kw)


def to_np(*ts):
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy() for t in ts]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def rand_actions(n, seed):
    return np.random.default_rng(seed).uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32)


# --------------------------------------------------------------------------- shared oracle states
@functools.lru_cache(maxsize=None)
def oracle_rounds(env_id):
    """The oracle recipe of test_gpu_parity._single_step_round (seeds 0..n-1, 25 warm steps,
    default_rng(0) actions), n = 4099, 4 rounds: per round the state image, elapsed and the action.
    A quarter of the envs sit one step before the TimeLimit and 64 envs outside the [0, 20] field, so both
    truncation causes occur.  Computed once per id; the tests copy what they change."""
    n = N_BIG
    orc = O.OracleVectorEnv(env_id, n)
    orc.reset(list(range(n)))
    rng = np.random.default_rng(0)
    for _ in range(WARM):
        orc.step(rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32))
    limit = O.TIME_LIMITS[env_id]
    out = []
    for _ in range(ROUNDS):
        st = {k: np.array(v, copy=True) for k, v in orc.env.get_state().items()}
        el = orc.elapsed.astype(np.int32).copy()
        el[::4] = limit - 1
        outside = np.arange(64) * (n // 64) + 1
        st["x"][outside[:32]] = 20.5
        st["y"][outside[32:]] = -0.5
        a = rng.uniform([0.2, -1], [1, 1], size=(n, 2)).astype(np.float32)
        for v in st.values():
            v.setflags(write=False)
        out.append((st, el, a))
        orc.step(a)
    return out


def inject(env, st, el, n=None):
    sl = slice(None) if n is None else slice(0, n)
    env.set_state({k: v[sl] for k, v in st.items()})
    env.set_field("elapsed", el[sl])
    env.set_field("scan_valid", 1)


def step_injected(env_id, precision, rnd, ignore, n=None, **kw):
    """One step of a fresh handle from round `rnd`'s state (its first n envs), autoreset off."""
    st, el, a = oracle_rounds(env_id)[rnd]
    nn = N_BIG if n is None else n
    env = make(env_id, nn, precision=precision, autoreset=False, ignore_obstacles=ignore, **kw)
    inject(env, st, el, n)
    obs, rew, term, trunc, info = env.step(torch.from_numpy(a[:nn]).cuda())
    res = dict(zip(("obs", "rew", "term", "trunc", "done"), to_np(obs, rew, term, trunc, info["_final_obs"])))
    if env.info_enabled:
        (res["info"],) = to_np(env.info_buf)
    res["scan_valid"] = env.get_field("scan_valid")
    env.close()
    return res


@functools.lru_cache(maxsize=None)
def ignoring_round0(env_id, precision):
    """The product build's scan-free step on round 0, n = 4099 (shared by the shape and safe-build tests)."""
    return step_injected(env_id, precision, 0, True)


# --------------------------------------------------------------------------- 1. fixture replay
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("fname,prefix,env_id", FIXTURES, ids=FIXTURE_IDS)
def test_fixture_replay(golden, fname, prefix, env_id, precision):
    """The reference's ignore_obstacles trajectories replayed from its post-reset state, autoreset off, up
    to each env's first episode end.  Bounds: those of test_gpu_parity.test_golden_trajectory_replay for
    the same ids and precisions."""
    g = block(golden(fname), prefix)
    n, T = g["actions"].shape[:2]
    limit = int(g["limit"])
    env = make(env_id, n, precision=precision, autoreset=False, max_episode_steps=limit, ignore_obstacles=True)
    env.set_state(golden_state(g))
    if precision == "f64":
        hdr_tol, rew_tol = 2e-6, 1e-8
    else:
        hdr_tol, rew_tol = (7e-6, 7e-5) if env_id == "usv-simple" else (1.5e-5, 1e-4)
    alive = np.ones(n, bool)
    worst = {"hdr": 0.0, "rew": 0.0}
    for t in range(T):
        obs, rew, term, trunc, _ = env.step(torch.from_numpy(g["actions"][:, t]).cuda())
        obs, rew, term, trunc = to_np(obs, rew, term, trunc)
        m = alive
        if not m.any():
            break
        assert np.all(obs[:, 15:] == np.float32(1.0)), f"t={t}"
        assert not term.any(), f"t={t}"
        np.testing.assert_array_equal(trunc[m], g["truncated"][m, t], err_msg=f"t={t}")
        worst["hdr"] = max(worst["hdr"], float(np.abs(obs[m, :15].astype(np.float64) - g["final_obs"][m, t]).max()))
        worst["rew"] = max(worst["rew"], float(np.abs(rew[m] - g["reward"][m, t]).max()))
        alive = alive & ~(g["terminated"][:, t] | g["truncated"][:, t])
    print(f"\n[ignore {fname} {prefix or '-'} {precision}] max |hdr| err {worst['hdr']:.3e}, "
          f"max |rew| err {worst['rew']:.3e}")
    assert worst["hdr"] <= hdr_tol and worst["rew"] <= rew_tol, worst
    env.close()


# --------------------------------------------------------------------------- 2. bitwise vs the scanning step
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("env_id", IDS)
def test_bitwise_against_scanning_step(env_id, precision):
    """Two handles, switch off / on, same injected state and actions: header, truncated and the reward
    apart from the collision term are bit-identical, with no tolerance."""
    rdt = np.float32 if precision == "f32" else np.float64
    pen_total = term_total = bounds = timelimit = 0
    for rnd in range(ROUNDS):
        s = step_injected(env_id, precision, rnd, False)
        g = ignoring_round0(env_id, precision) if rnd == 0 else step_injected(env_id, precision, rnd, True)
        assert same_bits(s["obs"][:, :15], g["obs"][:, :15]), f"round {rnd}: header"
        assert np.all(g["obs"][:, 15:] == np.float32(1.0))
        assert np.array_equal(s["trunc"], g["trunc"]) and not g["term"].any()
        assert np.array_equal(g["done"], g["trunc"])
        assert np.all(g["scan_valid"] == 2) and np.all(s["scan_valid"] == 1)
        assert s["rew"].dtype == g["rew"].dtype == rdt
        # the scanning step's penalty (:153-156: a raw reading < 0.2) as its obs shows it: a reading within
        # 1e-6 relative of the threshold after normalisation may be on either side
        smin = s["obs"][:, 15:].astype(np.float64).min(axis=1) * 100.0
        surely, surely_not = smin < 0.2 * (1 - 1e-6), smin > 0.2 * (1 + 1e-6)
        equal = s["rew"].view(np.uint8).reshape(len(smin), -1) == g["rew"].view(np.uint8).reshape(len(smin), -1)
        equal = equal.all(axis=1)
        shifted = s["rew"] == (rdt(-20) + g["rew"]).astype(rdt)          # R(-20) + partial in the handle's type
        assert np.all(equal[surely_not]), f"round {rnd}: reward of an unpenalised env differs"
        assert np.all(shifted[surely]), f"round {rnd}: penalised reward != -20 + ignoring reward"
        assert np.all(equal | shifted)
        pen_total += int(surely.sum())
        term_total += int(s["term"].sum())
        st, el, _ = oracle_rounds(env_id)[rnd]
        bounds += int(g["trunc"][(st["x"] > 20) | (st["y"] < 0)].sum())
        timelimit += int(g["trunc"][::4].sum())
    print(f"\n[{env_id} {precision}] scanning step: {pen_total} penalised, {term_total} terminated; "
          f"truncated by bounds {bounds}, by TimeLimit {timelimit}")
    assert pen_total >= 10 and term_total >= 1, "the scanning step must exercise the collision paths"
    assert bounds >= ROUNDS * 60 and timelimit >= ROUNDS * (N_BIG // 4)


# --------------------------------------------------------------------------- 3. row streaming shapes
GUARD = -12345.0


def _raw_step(env_id, precision, n, misalign):
    """usv_step into an obs buffer with guard words around it; obs starts 16-B aligned, or 4 B past."""
    st, el, a = oracle_rounds(env_id)[0]
    env = make(env_id, n, precision=precision, autoreset=False, ignore_obstacles=True)
    inject(env, st, el, n)
    lead = 5 if misalign else 4
    buf = torch.full((lead + n * 143 + 7,), GUARD, dtype=torch.float32, device="cuda")
    obs = buf[lead:lead + n * 143].view(n, 143)
    assert obs.data_ptr() % 16 == (4 if misalign else 0)
    rdt = torch.float32 if precision == "f32" else torch.float64
    rew = torch.zeros(n, dtype=rdt, device="cuda")
    term = torch.ones(n, dtype=torch.uint8, device="cuda")
    trunc = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert env.step_raw(torch.from_numpy(a[:n]).cuda(), obs, rew, term, trunc) == 0
    b, r, te, tr = to_np(buf, rew, term, trunc)
    env.close()
    return b, lead, r, te.astype(bool), tr.astype(bool)


@pytest.mark.parametrize("n,misalign", [(1, False), (63, False), (64, False), (65, False), (65, True), (257, False)])
def test_row_streaming_shapes(n, misalign):
    """Ragged last waves, one and several blocks, and an obs pointer 4 B off 16-B alignment (dword
    stores): every row equals the n = 4099 kernel's row for the same env state, and nothing outside the
    obs buffer is written."""
    for env_id, precision in (("usv-simple", "f32"), ("usv-asmc-simple", "f64")):
        big = ignoring_round0(env_id, precision)
        b, lead, r, te, tr = _raw_step(env_id, precision, n, misalign)
        rows = b[lead:lead + n * 143].reshape(n, 143)
        assert same_bits(rows, big["obs"][:n]), (env_id, precision)
        assert np.all(b[:lead] == np.float32(GUARD)) and np.all(b[lead + n * 143:] == np.float32(GUARD))
        assert same_bits(r, big["rew"][:n]) and np.array_equal(tr, big["trunc"][:n]) and not te.any()


# --------------------------------------------------------------------------- 4. same-step autoreset
@pytest.mark.parametrize("reset_rng", ["philox", "numpy"])
@pytest.mark.parametrize("env_id,precision", [("usv-simple", "f32"), ("usv-asmc-simple", "f32"), ("usv-simple", "f64")])
def test_same_step_autoreset(env_id, precision, reset_rng):
    """An autoresetting ignoring handle against a twin with autoreset off that resets explicitly."""
    n, limit, steps = 130, 3, 7
    kw = dict(precision=precision, max_episode_steps=limit, seed=11, reset_rng=reset_rng, ignore_obstacles=True)
    a_env = make(env_id, n, autoreset=True, **kw)
    b_env = make(env_id, n, autoreset=False, **kw)
    oa, _ = a_env.reset(seed=11)
    ob, _ = b_env.reset(seed=11)
    assert same_bits(*to_np(oa, ob))
    stagger = (np.arange(n) % limit).astype(np.int32)       # a third of the envs ends at every step
    a_env.set_field("elapsed", stagger)
    b_env.set_field("elapsed", stagger)
    ends = 0
    for t in range(steps):
        act = torch.from_numpy(rand_actions(n, 100 + t)).cuda()
        oa, ra, tea, tra, info = a_env.step(act)
        ob, rb, teb, trb, _ = b_env.step(act)
        oa, ra, tea, tra, fa, da, ob, rb, teb, trb = to_np(oa, ra, tea, tra, info["final_obs"], info["_final_obs"],
                                                            ob, rb, teb, trb)
        done = trb | teb
        assert not tea.any() and not teb.any()
        assert np.array_equal(tra, trb) and np.array_equal(da, tra) and same_bits(ra, rb), f"t={t}"
        assert same_bits(fa[done], ob[done]), f"t={t}: final_obs != the twin's terminal obs"
        assert same_bits(oa[~done], ob[~done]), f"t={t}"
        assert done.sum() >= n // limit
        ends += int(done.sum())
        ob2, _ = b_env.reset(mask=torch.from_numpy(done).cuda())
        (ob2,) = to_np(ob2)
        assert same_bits(oa, ob2), f"t={t}: returned rows != the twin's reset obs"
        # a fresh episode's header (_get_obs(zeros(3)) at the path start), sensors 1.0 (stale scan)
        assert np.all(oa[done, 15:] == np.float32(1.0))
        assert np.all(oa[done, 7:9] == 0) and np.all(oa[done, 5] == 0)
        assert not same_bits(oa[done, :5], fa[done, :5])
        for env in (a_env, b_env):
            sv, sl, el = env.get_field("scan_valid"), env.get_field("sensor_last"), env.get_field("elapsed")
            assert np.all(sv[done] == 0) and np.all(sv[~done] == 2), f"t={t}"
            assert np.all(sl[done] == 100.0) and np.all(el[done] == 0), f"t={t}"
        for k in ("x", "psi", "max_u", "n_obs", "episode", "obs_x"):
            assert np.array_equal(a_env.get_field(k), b_env.get_field(k)), (k, t)
    assert ends >= 2 * n
    a_env.close()
    b_env.close()


# --------------------------------------------------------------------------- 5. toggle
@pytest.mark.parametrize("env_id,precision", [("usv-simple", "f32"), ("usv-asmc-simple", "f32"),
                                              ("usv-simple", "f64"), ("usv-asmc-simple", "f64")])
def test_toggle_at_run_time(env_id, precision):
    n = 300
    kw = dict(precision=precision, autoreset=False, seed=5)
    a_env, b_env = make(env_id, n, **kw), make(env_id, n, **kw)
    a_env.reset(seed=5)
    b_env.reset(seed=5)
    acts = [torch.from_numpy(rand_actions(n, 200 + t)).cuda() for t in range(3)]
    assert a_env.ignore_obstacles is False
    o1 = a_env.step(acts[0])[0]
    a_env.ignore_obstacles = True
    assert a_env.ignore_obstacles is True
    o2 = a_env.step(acts[1])[0]
    (o1, o2) = to_np(o1, o2)
    assert np.any(o1[:, 15:] != 1.0) and np.all(o2[:, 15:] == np.float32(1.0))
    assert np.all(a_env.get_field("scan_valid") == 2)
    blob = a_env.state_blob()
    a_env.ignore_obstacles = False                       # the installed variant is used again
    ra = to_np(*a_env.step(acts[2])[:4])
    b_env.load_state_blob(blob)                          # B never ignores
    rb = to_np(*b_env.step(acts[2])[:4])
    for x, y in zip(ra, rb):
        assert same_bits(x, y)
    assert np.any(ra[0][:, 15:] != 1.0) and np.all(a_env.get_field("scan_valid") == 1)
    # explicit resets: the stale scan follows the mode of the last step taken
    scan3 = ra[0][:, 15:]
    a_env.ignore_obstacles = True                        # toggled on, but the last step scanned
    (r0,) = to_np(a_env.reset()[0])
    assert same_bits(r0[:, 15:], scan3)
    a_env.step(acts[0])
    (r1,) = to_np(a_env.reset()[0])                      # right after an ignoring step
    assert np.all(r1[:, 15:] == np.float32(1.0))
    assert np.all(a_env.get_field("scan_valid") == 0) and np.all(a_env.get_field("sensor_last") == 100.0)
    a_env.step(acts[1])
    a_env.ignore_obstacles = False                       # toggled off without stepping
    (r2,) = to_np(a_env.reset()[0])
    assert np.all(r2[:, 15:] == np.float32(1.0))
    (r3,) = to_np(a_env.reset()[0])                      # reset again, no step between: the stored scan
    assert np.all(r3[:, 15:] == np.float32(1.0))
    c_env = make(env_id, n, ignore_obstacles=True, **kw)
    (r4,) = to_np(c_env.reset(seed=5)[0])                # a never-stepped env
    assert np.all(r4[:, 15:] == 0)
    for e in (a_env, b_env, c_env):
        e.close()


# --------------------------------------------------------------------------- 6. scan_valid == 2 through the state interface
def test_scan_valid_two_survives_state_exchange():
    n = 70
    kw = dict(precision="f32", autoreset=False, seed=9)
    src = make("usv-simple", n, ignore_obstacles=True, **kw)
    src.reset(seed=9)
    src.step(torch.from_numpy(rand_actions(n, 1)).cuda())
    st, blob = src.get_state(), src.state_blob()
    assert np.all(st["scan_valid"] == 2)
    for how in ("fields", "blob"):
        dst = make("usv-simple", n, **kw)                # a scanning handle: the value alone decides
        if how == "fields":
            dst.set_state(st)
        else:
            dst.load_state_blob(blob)
        assert np.all(dst.get_field("scan_valid") == 2)
        assert np.array_equal(dst.state_blob(), blob)
        (ro,) = to_np(dst.reset()[0])
        assert np.all(ro[:, 15:] == np.float32(1.0))
        assert np.all(dst.get_field("scan_valid") == 0) and np.all(dst.get_field("sensor_last") == 100.0)
        dst.close()
    src.close()


# --------------------------------------------------------------------------- 7. API
def test_api_surface():
    import gym_usv_amd
    from gym_usv_amd.sb3 import Sb3VecEnv
    n = 66
    env = make("usv-simple", n, ignore_obstacles=True)
    assert env.ignore_obstacles is True and env.cfg.flags == 2
    env.ignore_obstacles = False
    assert env.ignore_obstacles is False
    env.close()
    with pytest.raises(gym_usv_amd.UsvLibError):
        make("usv-asmc-v0", 4, ignore_obstacles=True)
    legacy = make("usv-pid-v0", 4)
    with pytest.raises(gym_usv_amd.UsvLibError):
        legacy.ignore_obstacles = True
    assert legacy.ignore_obstacles is False
    legacy.close()
    # the reference's way: an attribute set after make()
    single = gym_usv_amd.make("usv-simple")
    assert single.ignore_obstacles is False
    single.ignore_obstacles = True
    assert single.ignore_obstacles is True
    o0, _ = single.reset(seed=3)
    o1, r1, te, tr, inf = single.step(np.array([0.5, 0.1], dtype=np.float32))
    assert np.all(o0[15:] == 0) and np.all(o1[15:] == np.float32(1.0)) and te is False
    assert inf["reward"] == r1
    single.close()
    single = gym_usv_amd.make("usv-asmc-simple", ignore_obstacles=True)
    assert single.ignore_obstacles is True
    single.close()
    vec = Sb3VecEnv("usv-simple", num_envs=8)
    assert vec.get_attr("ignore_obstacles") == [False] * 8
    vec.set_attr("ignore_obstacles", True)
    assert vec.get_attr("ignore_obstacles", indices=[0, 3]) == [True, True] and vec.venv.ignore_obstacles is True
    vec.reset()
    obs, _, dones, _ = vec.step(rand_actions(8, 2))
    assert np.all(obs[:, 15:] == np.float32(1.0)) and not dones.any()
    vec.close()
    vec = gym_usv_amd.make_sb3_vec_env("usv-simple", 8, ignore_obstacles=True)
    assert vec.get_attr("ignore_obstacles") == [True] * 8
    vec.close()


@pytest.mark.parametrize("env_id", IDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_info_rows_and_done_mask(env_id, precision):
    """info=True rows are the scanning step's rows, bitwise; info['_final_obs'] equals truncated."""
    s = step_injected(env_id, precision, 1, False, n=1030, info=True)
    g = step_injected(env_id, precision, 1, True, n=1030, info=True)
    assert same_bits(s["info"], g["info"]) and np.any(g["info"] != 0)
    assert np.array_equal(g["done"], g["trunc"]) and g["trunc"].sum() >= 1030 // 4


# --------------------------------------------------------------------------- 8. safe build
def test_safe_build_bitwise():
    """libusvhip_safe.so (every hand-counted vmcnt wait a vmcnt(0)) gives the product build's outputs."""
    from gym_usv_amd import _lib
    for env_id in IDS:
        for precision in PRECISIONS:
            prod = ignoring_round0(env_id, precision)
            safe = step_injected(env_id, precision, 0, True, lib_path=_lib.SAFE_LIB_PATH)
            for k in ("obs", "rew", "term", "trunc", "done", "scan_valid"):
                assert same_bits(prod[k], safe[k]), (env_id, precision, k)
