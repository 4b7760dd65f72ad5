"""The host state interface on the GPU: usv_get_field / usv_set_field / usv_get_state / usv_set_state
(gym-usv_amd/csrc/usv_kernels.hip, driven by the field table of usv_layout.hpp).

* Every field of every env id, in both precisions, written with a pattern and read back, at shapes where
  the SoA row stride differs from N and the obstacle plane stride from cap: a wrong base, stride or
  width, or a write that reaches a neighbour, shows as a changed value somewhere.
* The state blob as the fields in order, and the f32 heading frame (phi + 2 pi k) behind "psi" and ASMC row 0.
  (The blob as checkpoint of a rollout: test_state_blob_roundtrip in test_gpu_parity.py.)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENV_IDS = ("usv-simple", "usv-asmc-simple", "usv-asmc-v0", "usv-asmc-ye-int-v0", "usv-pid-v0")
SHAPES = ((1, 32), (64, 32), (77, 29), (77, 33))     # (N, cap): f32 fstride 64, 64, 128, 128; ostride 32, 32, 32, 36


def make(env_id, n, **kw):
    import gym_usv_amd
    return gym_usv_amd.make_vec(env_id, n, device=0, **kw)


def to_np(*ts):
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy() for t in ts]


def pattern(env, name, cap):
    """Values distinct per (field, env, component) and exact in float32: 0.25 m with m < 2^21 (ints: m
    itself).  n_obs stays within [0, cap]; the headings ("psi", and ASMC row 0,
    UsvAsmc's psi_d_last) are multiples of 1/32 within (-3, 3), so the f32 turn frame holds zero whole
    turns and both round-trip exactly."""
    f, per, isint = env._fields[name]
    n = env.num_envs
    e, c = np.meshgrid(np.arange(n), np.arange(per), indexing="ij")
    m = (f * 80 + e) * 640 + c + 1                   # n <= 80 envs, per <= 640 values, 32 fields: < 2^21
    if name == "n_obs":
        m = (3 + 5 * e) % (cap + 1)
    v = m.astype(np.int32) if isint else 0.25 * m
    if name == "psi":
        v = (e - 38) / 16.0
    if name == "asmc":
        v[:, 0] = (38 - e[:, 0]) / 16.0 + 1 / 32
    return v.reshape(n) if per == 1 else v


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n,cap", SHAPES)
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("env_id", ENV_IDS)
def test_every_field_set_get_exact_and_isolated(env_id, precision, n, cap):
    """After a reset, each field in index order is set to its pattern and the whole state read back: the
    written field equals the pattern exactly and every other field keeps its previous bits.  Then the
    blob is the fields' host arrays in field order, and loading it into the re-reset env reproduces them."""
    env = make(env_id, n, precision=precision, obstacle_cap=cap, seed=5)
    env.reset(seed=5)
    names = env.field_names
    assert len(names) == 32
    state = env.get_state()
    for name in names:
        pat = pattern(env, name, cap)
        env.set_field(name, pat)
        new = env.get_state()
        for other in names:
            want = pat.astype(state[other].dtype) if other == name else state[other]
            assert same_bits(new[other], want), f"after set_field({name!r}): {other!r} " + \
                ("is not the pattern" if other == name else "changed")
        state = new
    blob = env.state_blob()
    assert blob.tobytes() == b"".join(state[k].tobytes() for k in names)
    env.reset(seed=6)
    assert not same_bits(env.get_field("x"), state["x"])
    env.load_state_blob(blob)
    back = env.get_state()
    for k in names:
        assert same_bits(back[k], state[k]), f"load_state_blob: {k!r} differs"
    env.close()


@pytest.mark.parametrize("env_id", ["usv-simple", "usv-asmc-simple"])
def test_f32_heading_turns_roundtrip_and_spin(env_id):
    """The f32 state holds the heading as phi + 2 pi k: a heading of ~400 rad set through the state
    interface reads back to float precision of phi (not float32's 3e-5 at 400 rad), psi_d_last
    keeps its value across a frame change (usv-asmc-simple), and a usv-simple rollout spinning at
    full yaw (the heading passing tens of turns) keeps the f32 obs header within 2e-5 of the f64
    kernel's."""
    n = 64
    envs = {p: make(env_id, n, precision=p, autoreset=False, reset_rng="numpy", max_episode_steps=0)
            for p in ("f32", "f64")}
    for e in envs.values():
        e.reset(seed=list(range(900, 900 + n)))
    e32 = envs["f32"]
    psi = np.linspace(-400.3, 400.7, n)
    e32.set_field("psi", psi)
    assert np.abs(e32.get_field("psi") - psi).max() < 1e-6
    if env_id == "usv-asmc-simple":
        st = e32.get_field("asmc")
        st[:, 0] = psi + 0.25
        e32.set_field("asmc", st)
        e32.set_field("psi", psi + 12.0)                 # a new frame: psi_d_last keeps its value
        assert np.abs(e32.get_field("asmc")[:, 0] - (psi + 0.25)).max() < 1e-5
        e32.set_field("psi", psi)
        e32.set_field("asmc", np.zeros((n, 16)))
    if env_id != "usv-simple":          # (the ASMC's switching law makes f32 and f64 rollouts part ways)
        for e in envs.values():
            e.close()
        return
    envs["f64"].set_state(e32.get_state())
    a = torch.tensor([[0.3, 1.0]] * n, device="cuda")
    alive = np.ones(n, bool)
    worst = 0.0
    for t in range(300):
        o32, _, te, tr, _ = e32.step(a)
        o64, _, te64, tr64, _ = envs["f64"].step(a)
        o32, o64, te, tr, te64, tr64 = to_np(o32, o64, te, tr, te64, tr64)
        alive &= ~(te | tr | te64 | tr64)
        if not alive.any():
            break
        worst = max(worst, float(np.abs(o32[alive, :15] - o64[alive, :15]).max()))
    spin = np.abs(e32.get_field("psi") - psi).max()
    print(f"\n[{env_id} heading turns] |psi| up to {np.abs(e32.get_field('psi')).max():.1f} rad "
          f"(moved {spin:.1f} rad), f32 vs f64 obs header max err {worst:.2e}, {int(alive.sum())} envs alive")
    assert alive.sum() >= n // 4 and spin > 20
    assert worst <= 2e-5, worst
    for e in envs.values():
        e.close()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 1e11])
def test_heading_set_rejects_unrepresentable_turns(bad):
    """The f32 build stores the heading as phi + 2 pi k with k an int32 (DESIGN 'Heading in the f32
    build'): a non-finite heading or one whose turn count overflows int32 is refused
    and leaves the state untouched."""
    import gym_usv_amd
    env = make("usv-simple", 64, seed=3)
    env.reset(seed=3)
    before = env.get_field("psi").copy()
    psi = before.copy()
    psi[5] = bad
    with pytest.raises(gym_usv_amd.UsvLibError):
        env.set_field("psi", psi)
    np.testing.assert_array_equal(env.get_field("psi"), before)
    psi[5] = 1e9                                       # large but representable: exact round trip of k
    env.set_field("psi", psi)
    got = env.get_field("psi")
    assert abs(got[5] - 1e9) <= 2 * np.pi * 2 ** -23 * 4   # phi in [-pi, pi] rounded to f32
    env.close()
