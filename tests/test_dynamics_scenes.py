"""The directed dynamics scenes (tests/dynamics_scenes.py) on the host: the float64 oracle reproduces
the reference's outputs on them (tests/golden/dynamics_scenes.npz), every scene does what its label
says, and every branch the scenes are for is taken on each side.  No GPU."""
import os

import numpy as np
import pytest

import dynamics_scenes as DS

SHORT = {"usv-simple": "simple", "usv-asmc-simple": "asmc"}
CASES = [(b, e) for b in DS.BATCHES for e in DS.ENV_IDS]


def fixture(golden, name, env_id):
    g = golden("dynamics_scenes.npz")
    pre = f"{name}__{SHORT[env_id]}__"
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}, g


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# --------------------------------------------------------------------------- a. the oracle's pin
@pytest.mark.parametrize("name,env_id", CASES)
def test_oracle_reproduces_the_reference(golden, name, env_id):
    """obs bits (signed zeros included), flags exactly, reward to 1e-12, info to 1e-12 relative to
    max(1, |ref|); the fixture's inputs are the bits this module builds."""
    ref, g = fixture(golden, name, env_id)
    sc, tr = DS.batch(name), DS.trace(name, env_id)
    for k in DS.INPUT_KEYS:
        assert g[f"{name}__{k}"].dtype == sc[k].dtype and np.array_equal(bits(g[f"{name}__{k}"]), bits(sc[k])), k
    assert int(g[f"{name}__limit"]) == sc["limit"] and bool(g["sensors_all_one"])
    bad = np.argwhere(bits(tr["hdr"]) != bits(ref["hdr"]))
    assert bad.size == 0, f"obs[{bad[0][2]}] step {bad[0][1] + 1}: {tr['hdr'][tuple(bad[0])]!r} vs " \
                          f"{ref['hdr'][tuple(bad[0])]!r}; {DS.describe(name, int(bad[0][0]))}"
    if name in DS.WITH_OBSTACLES:
        assert np.array_equal(bits(tr["sensors"]), bits(ref["sensors"]))
    else:
        assert np.all(tr["sensors"] == np.float32(1.0))
    for k in ("terminated", "truncated"):
        bad = np.argwhere(tr[k] != ref[k])
        assert bad.size == 0, f"{k} step {bad[0][1] + 1}: {DS.describe(name, int(bad[0][0]))}"
    assert np.abs(tr["reward"] - ref["reward"]).max() <= 1e-12
    assert (np.abs(tr["info"] - ref["info"]) / np.maximum(1.0, np.abs(ref["info"]))).max() <= 1e-12
    if env_id == "usv-asmc-simple":
        assert (np.abs(tr["psi_d_last"] - ref["psi_d_last"]) / np.maximum(1.0, np.abs(ref["psi_d_last"]))).max() <= 1e-12


def test_parked_second_quadrant_scene_reads_minus_zero(golden):
    """The reference returns obs[5] = -0.0 for a boat parked on the start of a path into the second
    quadrant (ye = -0 * sin + 0 * cos with sin > 0 > cos), and +0.0 in the other directions."""
    sc = DS.batch("ye")
    rows = np.flatnonzero(sc["negzero"])
    zero = np.flatnonzero(np.array(sc["q"]) == "ye")
    assert rows.size >= 1 and zero.size >= 8
    for env_id in DS.ENV_IDS:
        ref, _ = fixture(golden, "ye", env_id)
        assert np.all(ref["hdr"][zero, :, 5] == 0)
        np.testing.assert_array_equal(np.signbit(ref["hdr"][zero, 0, 5]), sc["negzero"][zero])


# --------------------------------------------------------------------------- b. the labels
def _parked(sc):
    """Scenes that usv-asmc-simple leaves where they are (zero velocity and action, psi_d_last = psi)."""
    z = (sc["u"] == 0) & (sc["r"] == 0) & (sc["last_u"] == 0) & (sc["last_r"] == 0) & (sc["asmc0"] == sc["psi"])
    return z & (sc["actions"] == 0).all(axis=(1, 2))


@pytest.mark.parametrize("name,env_id", CASES)
def test_scenes_do_what_their_labels_say(name, env_id):
    """The labelled quantity lies on the named side of its threshold in the named step by at least the
    scene's margin (side 0: exactly on it).  usv-simple: every scene.  usv-asmc-simple runs UsvAsmc first,
    so there the labels hold for the parked scenes and for the asmc_wrap ones."""
    sc, tr = DS.batch(name), DS.trace(name, env_id)
    q = np.array(sc["q"])
    rows = np.arange(len(q)) if env_id == "usv-simple" else np.flatnonzero(_parked(sc) | (q == "asmc_wrap"))
    if name in DS.WITH_OBSTACLES or name.startswith("timelimit"):
        assert len(rows) >= len(q) // 2
    for i in rows:
        assert q[i] in DS.QUANTITIES, q[i]
        t, side, v = int(sc["step"][i]) - 1, int(sc["side"][i]), tr[q[i]][i]
        msg = f"{q[i]} = {v.tolist()}; {DS.describe(name, int(i))}"
        if q[i] == "rebase":
            want = np.zeros(DS.T)
            want[t] = side
            assert np.array_equal(v, want), msg
            continue
        assert np.sign(v[t]) == side, msg
        assert abs(v[t]) >= sc["margin"][i] if side else v[t] == 0, msg
        if t > 0:                                    # a step-2 scene raises no flag in step 1
            assert not tr["truncated"][i, :t].any(), msg
        if sc["negzero"][i]:
            assert np.signbit(v).all(), msg
        if q[i] == "tl":
            first = np.flatnonzero(tr["truncated"][i])
            assert (first.size and first[0] == t) if sc["limit"] else first.size == 0, msg
    # the flags follow from the quantities, with the reference's strict inequalities
    out = (tr["x_lo"] < 0) | (tr["x_hi"] > 0) | (tr["y_lo"] < 0) | (tr["y_hi"] > 0) | (tr["tl"] >= 0)
    assert np.array_equal(tr["truncated"], out) and np.array_equal(tr["terminated"], tr["key"] < 0)


def test_contact_scenes_read_d_minus_r():
    """An obstacle dead ahead on ray k reads d - r on it (test_sweep_closed_forms' closed form), so the on-ray
    scenes' collision quantity is their termination quantity moved by 0.15; off-centre the reading is larger."""
    for name in DS.WITH_OBSTACLES:
        sc, tr = DS.batch(name), DS.trace(name, "usv-simple")
        on = np.array(["on ray 63.5" not in s for s in sc["note"]])
        assert on.sum() == 2 * (~on).sum() > 0
        assert np.abs((tr["coll"] + 0.2) - (tr["key"] + 0.05))[on].max() <= 1e-13
        assert ((tr["coll"] + 0.2) - (tr["key"] + 0.05))[~on].min() > 1e-6


# --------------------------------------------------------------------------- c. coverage
def _sides(name, q, env_id="usv-simple"):
    """The signs the scenes labelled q take in their step."""
    sc, tr = DS.batch(name), DS.trace(name, env_id)
    rows = np.flatnonzero(np.array(sc["q"]) == q)
    return set(np.sign(tr[q][rows, sc["step"][rows] - 1]).astype(int))


def test_every_branch_is_taken_on_each_side():
    both, three = {-1, 1}, {-1, 0, 1}
    for ch in ("u", "r"):
        for q in (f"acc_{ch}_lo", f"acc_{ch}_hi", f"spd_{ch}_lo", f"spd_{ch}_hi"):
            assert _sides("clips", q) == both, q
    sc, tr = DS.batch("clips"), DS.trace("clips", "usv-simple")
    a = sc["actions"][:, 0]
    assert {-5.0, 5.0} <= set(a.ravel()) and np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()
    assert (sc["u"] < 0).any() and ((tr["acc_u_hi"][:, 0] > 0) & (tr["spd_u_hi"][:, 0] > 0)).any()   # both clips at once
    assert _sides("progress", "prog_lo") == three and _sides("progress", "prog_hi") == {1}
    tr = DS.trace("progress", "usv-simple")
    assert ((tr["prog_lo"][:, 0] > 0) & (tr["prog_hi"][:, 0] < 0)).any()                               # inside (progress, 1)
    sc = DS.batch("progress")
    d = np.stack([sc["path_x1"] - sc["path_x0"], sc["path_y1"] - sc["path_y0"]], axis=1)
    assert {(int(a), int(b)) for a, b in np.sign(d)} == {(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)}
    assert {1.0, 100.0, 110.0, 200.0} <= set(np.round(np.hypot(d[:, 0], d[:, 1]), 9))
    for q in ("oct_dx", "oct_dy", "oct_diag"):
        assert _sides("angle", q) == three, q
    sc, tr = DS.batch("angle"), DS.trace("angle", "usv-simple")
    oct_rows = np.flatnonzero([s.startswith("oct") for s in sc["q"]])
    tgt = np.stack([tr["oct_dx"][oct_rows, 0], tr["oct_dy"][oct_rows, 0]], axis=1)
    assert len({(int(a), int(b), int(c)) for (a, b), c in zip(np.sign(tgt), np.sign(tr["oct_diag"][oct_rows, 0]))}) == 16   # the 8 boundaries and the 8 open octants
    assert _sides("angle", "cut") == both and _sides("angle", "dist") == {-1}
    cut = np.flatnonzero(np.array(sc["q"]) == "cut")
    near_pi = tr["info"][cut, 0, 13]                  # angle to target / pi, wrapped: both signs next to the cut
    assert (near_pi > 0.99).sum() >= 4 and (near_pi < -0.99).sum() >= 4
    assert _sides("ye", "ye_k") == both and _sides("ye", "ye") == {0}
    sc, tr = DS.batch("ye"), DS.trace("ye", "usv-simple")
    k = np.flatnonzero(np.array(sc["q"]) == "ye_k")
    assert {(int(a), int(b)) for a, b in zip(np.sign(tr["ye"][k, 0]), np.sign(tr["ye_k"][k, 0]))} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    assert sc["negzero"].sum() >= 1 and np.abs(tr["ye"]).max() > 19.9
    for ax in ("x", "y"):
        assert _sides("bounds", f"{ax}_lo") == three and _sides("bounds", f"{ax}_hi") == three, ax
    sc = DS.batch("bounds")
    assert {1, 2} <= set(sc["step"]) and np.signbit(sc["x"][sc["x"] == 0]).any() and np.signbit(sc["y"][sc["y"] == 0]).any()
    assert _sides("timelimit", "tl") == {0} and _sides("timelimit0", "tl") == {-1}
    assert {1, 2} <= set(DS.batch("timelimit")["step"])
    for env_id in DS.ENV_IDS:                         # the rebase fires both ways under either id
        r = DS.trace("heading", env_id)["rebase"]
        assert (r == 1).sum() >= 10 and (r == -1).sum() >= 10 and (r == 0).all(axis=1).sum() >= 10, env_id
    assert _sides("heading", "rebase") == three and _sides("heading", "asmc_wrap") == both
    sc = DS.batch("heading")
    assert {0, 1, -1, 40, -40, 256, -256, 257, -257, 100000, -100000} <= set(np.rint(sc["psi"] / (2 * np.pi)).astype(int))
    assert (sc["asmc0"] != 0).all()
    for name in DS.WITH_OBSTACLES:
        assert _sides(name, "key") == both and _sides(name, "coll") == both, name


def test_size_and_fixture_limits():
    """A few hundred envs in all, and a fixture well inside the limit for a committed file."""
    n = sum(len(DS.batch(b)["x"]) for b in DS.BATCHES)
    assert 200 <= n <= 500, n
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dynamics_scenes.npz")
    assert os.path.getsize(path) < 512 * 1024
