"""The directed legacy scenes (tests/legacy_scenes.py) on the host: the fixture holds the inputs the module
builds, the float64 oracle (AsmcV0Batch, LegacyF64Batch) reproduces the reference's outputs and post-step state
on them (tests/golden/legacy_scenes.npz), every scene does what its label says, every threshold is taken on each
side, and the scenes either side of a discontinuous branch tell its two arms apart.  No GPU.

Measured when the fixture was written: usv-asmc-ye-int-v0 and usv-pid-v0 obs bit-equal, reward 1.1e-16, state
5.9e-16; usv-asmc-v0 obs and float32 state bit-equal, reward 1.1e-16."""
import os

import numpy as np
import pytest

import legacy_scenes as LS

CASES = [(b, e) for e in LS.ENV_IDS for b in LS.BATCHES if len(LS.batch(b, e)["x"])]
# Ten times the f32 build's bounds of tests/test_gpu_legacy_edges.py (obs and state 2e-4, reward 1e-3)
MOVE_OBS, MOVE_REW = 2e-3, 1e-2


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# --------------------------------------------------------------------------- a. the fixture's inputs, the oracle's pin
@pytest.mark.parametrize("name,env_id", CASES)
def test_fixture_inputs_are_the_scenes(golden, name, env_id):
    sc, ref = LS.batch(name, env_id), LS.fixture(golden("legacy_scenes.npz"), name, env_id)
    for k in LS.INPUT_KEYS:
        got = ref["in_" + k]
        assert got.dtype == sc[k].dtype and got.shape == sc[k].shape and np.array_equal(bits(got), bits(sc[k])), k
    assert ref["limit"] == sc["limit"] and ref["steps"] == sc["steps"]
    ak = sc["target"][:, 3]
    assert np.array_equal(ak, ak.astype(np.float32).astype(np.float64))          # as the reference's reset makes it
    if env_id == LS.V0:                              # float32 state once a step has stored it
        st = sc["elapsed"] != 0
        for k in ("x", "y", "psi", "u", "v", "r", "a_last", "last", "aux"):
            assert np.array_equal(sc[k][st], sc[k][st].astype(np.float32).astype(np.float64)), k


@pytest.mark.parametrize("name,env_id", CASES)
def test_oracle_reproduces_the_reference(golden, name, env_id):
    """obs bit for bit as float32, flags exactly, reward to 1e-12, post-step state to 1e-12 relative to
    max(1, |ref|); usv-asmc-v0's post-step state bit for bit after rounding to float32."""
    ref, tr = LS.fixture(golden("legacy_scenes.npz"), name, env_id), LS.trace(name, env_id)
    bad = np.argwhere(bits(tr["obs"]) != bits(ref["obs"]))
    assert bad.size == 0, f"obs[{bad[0][2]}] step {bad[0][1] + 1}: {tr['obs'][tuple(bad[0])]!r} vs " \
                          f"{ref['obs'][tuple(bad[0])]!r}; {LS.describe(name, env_id, int(bad[0][0]))}"
    for k in ("terminated", "truncated"):
        bad = np.argwhere(tr[k] != ref[k])
        assert bad.size == 0, f"{k} step {bad[0][1] + 1}: {LS.describe(name, env_id, int(bad[0][0]))}"
    assert np.abs(tr["reward"] - ref["reward"]).max() <= 1e-12
    for k in LS.STATE_KEYS:
        err = np.abs(tr[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))
        bad = np.argwhere(err > 1e-12)
        assert bad.size == 0, f"{k}{bad[0][2:].tolist()} step {bad[0][1] + 1}: {tr[k][tuple(bad[0])]!r} vs " \
                              f"{ref[k][tuple(bad[0])]!r}; {LS.describe(name, env_id, int(bad[0][0]))}"
        if env_id == LS.V0:
            assert np.array_equal(bits(tr[k].astype(np.float32)), bits(ref[k].astype(np.float32))), k


# --------------------------------------------------------------------------- b. the labels
@pytest.mark.parametrize("name,env_id", CASES)
def test_scenes_do_what_their_labels_say(name, env_id):
    """The labelled quantity lies on the named side of its threshold in the named step by at least the
    scene's margin (side 0: exactly on it), and the flags follow from the quantities with the reference's
    strict inequalities."""
    sc, tr = LS.batch(name, env_id), LS.trace(name, env_id)
    for i, q in enumerate(sc["q"]):
        assert q in LS.QUANTITIES, q
        t, side, v = int(sc["step"][i]) - 1, int(sc["side"][i]), tr[q][i]
        msg = f"{q} = {v.tolist()}; {LS.describe(name, env_id, i)}"
        assert np.sign(v[t]) == side, msg
        assert abs(v[t]) >= sc["margin"][i] if side else v[t] == 0, msg
        if name not in LS.F64_ONLY and side and q not in ("wrap_d", "tl", "first", "adot"):
            assert sc["margin"][i] >= 0.9 * LS.MARGIN or "N" in sc["note"][i], msg       # newtons: 0.04
        if sc["pair"][i] is not None:
            assert (int(np.sign(tr["ye"][i, 0])), int(np.sign(tr["ye_last"][i, 0]))) == sc["pair"][i], msg
    out = tr["ye10"] > 0
    out |= ((tr["x_hi"] > 0) | (tr["x_lo"] < 0)) if env_id == LS.V0 else (tr["x_min"] < 0)
    assert np.array_equal(tr["terminated"], out)
    assert np.array_equal(tr["truncated"], ~out & (tr["tl"] >= 0))
    assert np.array_equal(tr["first"][:, 0] > 0, sc["elapsed"] == 0) if env_id == LS.V0 else np.isnan(tr["first"]).all()


# --------------------------------------------------------------------------- c. coverage
def _sides(name, env_id, q):
    """The signs the scenes labelled q take in their step."""
    sc, tr = LS.batch(name, env_id), LS.trace(name, env_id)
    rows = np.flatnonzero(np.array(sc["q"]) == q)
    return set(np.sign(tr[q][rows, sc["step"][rows] - 1]).astype(int))


@pytest.mark.parametrize("env_id", LS.ENV_IDS)
def test_every_threshold_is_taken_on_each_side(env_id):
    both, three = {-1, 1}, {-1, 0, 1}
    v0, asmc = env_id == LS.V0, env_id != LS.PID
    assert _sides("drag", env_id, "drag") == three
    sc, tr = LS.batch("drag", env_id), LS.trace("drag", env_id)
    assert {(int(np.sign(u)), int(s)) for u, s in zip(sc["u"], sc["side"])} == {(a, b) for a in (-1, 1) for b in (-1, 0, 1)}
    assert ((tr["drag"][:, 0] > 0) & (tr["drag"][:, -1] < 0)).any()              # crosses within the steps
    if asmc:
        for q in ("ka_u", "ka_psi"):
            assert _sides("gains", env_id, q) == three, q
        sc, tr = LS.batch("gains", env_id), LS.trace("gains", env_id)
        for q, sg, ka in (("sig_u", "sigma_u", "ka_u"), ("sig_psi", "sigma_psi", "ka_psi")):
            rows = np.flatnonzero(np.array(sc["q"]) == q)
            assert (tr[ka][rows, 0] > 0).all()                                   # the gain above its minimum
            got = {(int(np.sign(tr[sg][i, 0])), int(np.sign(tr[q][i, 0]))) for i in rows}
            assert got >= {(a, b) for a in (-1, 1) for b in (-1, 1)}, q
        assert _sides("gains", env_id, "sig_psi") == both and _sides("gains", env_id, "sigma_psi") == {0}
        assert _sides("exact64", env_id, "sig_psi") == {0}           # np.sign(0) = 0
    else:
        sc = LS.batch("pid", env_id)
        assert (sc["last"][:, 6] != 0).all() and (sc["aux"][:, 0] != 0).any() and len(LS.batch("gains", env_id)["x"]) == 0
    for q in ("tport_hi", "tport_lo", "tstbd_hi", "tstbd_lo"):
        assert _sides("thrust", env_id, q) == both, q
    tr = LS.trace("thrust", env_id)
    assert (((tr["tport_hi"] > 0) & (tr["tstbd_lo"] < 0)) | ((tr["tport_lo"] < 0) & (tr["tstbd_hi"] > 0)))[:, 0].any()
    sc, tr = LS.batch("wrap", env_id), LS.trace("wrap", env_id)
    aks = sc["target"][:, 3]
    assert {(int(np.sign(np.cos(a))), int(np.sign(np.sin(a)))) for a in aks if a} == {(1, 1), (-1, 1), (-1, -1), (1, -1)}
    for q in ("wrap_d", "wrap_e", "wrap_psi", "wrap_ak"):
        rows = np.flatnonzero(np.array(sc["q"]) == q)
        for zero in (True, False):
            r = rows[(aks[rows] == 0) == zero]
            want = {-1} if (q == "wrap_ak" and zero) else both                   # |psi| <= pi: psi - 0 cannot pass the cut
            assert set(np.sign(tr[q][r, 0]).astype(int)) == want, (q, zero)
    f = float(np.float32(np.pi))
    assert {f, -f} <= set(sc["actions"][:, 0].astype(np.float64)) and f > np.pi
    sc, tr = LS.batch("path", env_id), LS.trace("path", env_id)
    z = sc["target"][:, 3] == 0
    assert np.signbit(sc["target"][z, 3]).any() and not np.signbit(sc["target"][z, 3]).all()
    assert _sides("path", env_id, "ye") == both and _sides("path", env_id, "ye1") == {-1}
    live = (~z) & (np.abs(np.abs(sc["target"][:, 3]) - np.pi / 2) > 0.1)
    sa, ca = np.sin(sc["target"][:, 3]), np.cos(sc["target"][:, 3])
    t1, t2 = -(sc["x"] - sc["target"][:, 0]) * sa, (sc["y"] - sc["target"][:, 1]) * ca
    assert (np.minimum(np.abs(t1), np.abs(t2))[live] > 0.5).all() and live.sum() >= 12      # both terms of ye live
    assert _sides("reward", env_id, "rew_ak") == both and _sides("reward", env_id, "ye1") == both
    assert _sides("reward", env_id, "adot") == {0, 1} and LS.trace("reward", env_id)["adot"].max() >= 299
    if env_id == LS.YEINT:
        sc = LS.batch("ye_int", env_id)
        assert {p for p in sc["pair"]} == {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)}
        assert (np.abs(sc["ye2"][:, 0]) >= 50).all() and np.signbit(sc["ye2"][sc["ye2"][:, 1] == 0, 1]).any()
        tr = LS.trace("ye_int", env_id)
        zero = tr["ye"][:, 0] == 0                   # the computed ye as -0.0 and as +0.0, both against a stored +0.0
        last0 = (sc["ye2"][:, 1] == 0) & ~np.signbit(sc["ye2"][:, 1])
        assert np.array_equal(np.signbit(tr["ye"][:, 0]) & zero, sc["negzero"]) and sc["negzero"].sum() >= 2
        assert (zero & last0 & sc["negzero"]).any() and (zero & last0 & ~sc["negzero"]).any()
        assert (tr["aux"][sc["negzero"], :, 3] == sc["ye2"][sc["negzero"], :1]).all()          # no restart: ye_int kept
    for name in ("bounds", "bounds64"):
        assert _sides(name, env_id, "ye10") == three, name
        for q in (("x_hi", "x_lo") if v0 else ("x_min",)):
            assert _sides(name, env_id, q) == both, (name, q)
        sc, tr = LS.batch(name, env_id), LS.trace(name, env_id)
        far = {float(x): bool(t) for x, t in zip(sc["x"], tr["terminated"][:, 0]) if x in (-15.0, 35.0)}
        assert far == ({-15.0: False, 35.0: True} if v0 else {-15.0: True, 35.0: False}), far
    assert np.abs(LS.trace("bounds64", env_id)["ye10"][:, 0]).min() == 0 and \
        np.sort(np.abs(LS.trace("bounds64", env_id)["ye10"][:, 0]))[2] < 2e-9
    assert _sides("timelimit", env_id, "tl") == {0} and _sides("timelimit0", env_id, "tl") == {-1}
    tr = LS.trace("timelimit", env_id)
    due = tr["tl"] == 0
    assert (due & tr["terminated"] & ~tr["truncated"]).any() and (due & tr["truncated"]).any()
    assert ((tr["tl"] == -1) & ~tr["terminated"] & ~tr["truncated"]).any()
    assert (due[:, 1] & tr["terminated"][:, 1] & ~tr["terminated"][:, 0]).any()  # falls due on the very step it ends
    assert not LS.trace("timelimit0", env_id)["truncated"].any()
    if v0:
        assert _sides("first", env_id, "first") == both and LS.batch("first", env_id)["steps"] == LS.T + 1
        sc = LS.batch("first", env_id)
        f64 = sc["elapsed"] == 0
        assert (sc["u"][f64] != sc["u"][f64].astype(np.float32)).all()
        assert np.array_equal(sc["u"][~f64], sc["u"][f64].astype(np.float32).astype(np.float64))


# --------------------------------------------------------------------------- d. discrimination
@pytest.mark.parametrize("env_id", LS.ENV_IDS)
def test_scenes_tell_the_arms_of_a_branch_apart(env_id):
    """Every scene next to a discontinuous branch (drag switch, gain arms, thrust clips, ye_int restart, reward
    arm), re-run through the oracle with that one comparison forced the other way in every step: obs or the
    post-step state moves by >= 2e-3 or the reward by >= 1e-2, ten times the f32 build's bounds.  The thrust
    scenes used sit 20 N either side of a clip, so a clip taken off a saturated thrust and a clip put on a free one
    both show (the pairs 0.05 N either side move nothing that large)."""
    seen = set()
    for name in LS.BATCHES:
        sc = LS.batch(name, env_id)
        flips = np.array([f or "" for f in sc["flip"]])
        for arm in sorted(set(flips) - {""}):
            rows = flips == arm
            tr, forced = LS.trace(name, env_id), LS.run_oracle(name, env_id, {arm: rows})
            moved = np.zeros(len(rows))
            for k in ("obs",) + LS.STATE_KEYS:
                moved = np.maximum(moved, np.abs(forced[k].astype(np.float64) - tr[k].astype(np.float64)).reshape(len(rows), -1).max(axis=1))
            rew = np.abs(forced["reward"] - tr["reward"]).max(axis=1)
            ok = (moved >= MOVE_OBS) | (rew >= MOVE_REW)
            assert ok[rows].all(), f"{arm}: " + "; ".join(LS.describe(name, env_id, int(i)) for i in np.flatnonzero(rows & ~ok))
            assert not (moved[~rows] > 0).any()      # the forced comparison touches no other scene
            sides = set(sc["side"][rows])
            assert sides == {-1, 1} or arm == "ye_restart", (arm, sides)           # both sides of the pair
            seen.add(arm)
    want = {"drag", "tport_hi", "tport_lo", "tstbd_hi", "tstbd_lo", "rew_ak"}
    want |= {"ka_u", "ka_psi", "sig_u", "sig_psi"} if env_id != LS.PID else set()
    want |= {"ye_restart"} if env_id == LS.YEINT else set()
    assert seen == want


def test_float32_state_compares_against_float32_constants(golden):
    """usv-asmc-v0 on stored float32 state: u = float32(1.2) is not above 1.2 and Ka = float32(kmin) is not above
    kmin, because NumPy compares a float32 scalar with a Python float in float32 (the reference's |u| > 1.2 and
    Ka > kmin); on the float64 reset state the same values are above.  The fixture shows which arm ran."""
    for name, q, col in (("drag", "drag", None), ("gains", "ka_u", 7), ("gains", "ka_psi", 8)):
        sc, tr = LS.batch(name, LS.V0), LS.trace(name, LS.V0)
        ref = LS.fixture(golden("legacy_scenes.npz"), name, LS.V0)
        rows = np.flatnonzero((np.array(sc["q"]) == q) & (sc["side"] == 0) & (sc["elapsed"] != 0))
        assert rows.size >= 1 and (tr[q][rows, 0] == 0).all()
        if col is not None:                          # Ka_dot_last is kmin itself on the arm at or below the minimum
            kmin = {7: 0.05, 8: 0.2}[col]
            assert np.array_equal(ref["last"][rows, 0, col], np.full(rows.size, np.float64(np.float32(kmin))))
    sc = LS.batch("drag", LS.V0)
    u = sc["u"][(sc["side"] == 0)]
    assert (np.abs(u) > 1.2).all() and (np.abs(u).astype(np.float32) == np.float32(1.2)).all()


def test_size_and_fixture_limits():
    """A few hundred envs in all, and a fixture no larger than the dynamics scenes'."""
    n = sum(len(LS.batch(b, e)["x"]) for b in LS.BATCHES for e in LS.ENV_IDS)
    assert 300 <= n <= 700, n
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    size = os.path.getsize(os.path.join(here, "legacy_scenes.npz"))
    assert size < 112 * 1024 and size <= os.path.getsize(os.path.join(here, "dynamics_scenes.npz"))
