"""The block-queue step's pair loop ("Pair-loop trims"): its stores in scalar-base form, the
single mark write of the two-pass lidar, and the full-pair copy of the loop that blocks with an even
env count run (a block with an odd count runs the general body with the lone-env case).

Yardsticks that share no code with the pair loop: the wave-per-env kernel (kind 1, "16,7,1") for whole
steps, the brute lidar ("64,0,1") and the float64 oracle for readings.  Every comparison between
kernels is bitwise.  Under test: the 128-env block shape ("128,7,5") and the 16-env one ("16,7,5"), the
span row layout forced on and off (lid bits 0x100 / 0x200), the DONE / INFO instantiations.
"""
import functools

import numpy as np
import pytest
import torch

import lidar_scenes as LS

gpu = pytest.mark.gpu

KIND1 = "16,7,1"
BRUTE = "64,0,1"
SHAPES = ("128,7,5", "16,7,5")
SPAN_ON, SPAN_OFF = "128,263,5", "128,519,5"     # lid 7 | 0x100, 7 | 0x200
F32_ATOL, F32_RTOL = 1e-3, 1e-4                  # the float32 figures of tests/test_gpu_lidar_edges.py
OBS = 143


def make(n, **kw):
    import gym_usv_amd
    return gym_usv_amd.make_vec("usv-simple", n, device=0, **kw)


def bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint8).copy()


def same(a, b, what):
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {int((a != b).sum())} bytes differ"


def actions(n, T, seed=5):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    lo = torch.tensor([0.2, -1.0], device="cuda")
    return [torch.rand(n, 2, device="cuda", generator=gen) * torch.tensor([0.8, 2.0], device="cuda") + lo
            for _ in range(T)]


def buffers(n):
    obs = torch.zeros(n, OBS, device="cuda")
    return (obs, torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
            torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros_like(obs))


def snapshot(obs, rew, term, trunc, fobs):
    """One step's outputs as bytes; final_obs rows of the envs that ended only (the others are unspecified)."""
    dn = (term | trunc).bool()
    return bits(obs), bits(rew), bits(term), bits(trunc), bits(fobs[dn])


# --------------------------------------------------------------------------- 1. lone env and block edges
@functools.lru_cache(maxsize=None)
def plain_rollout(n, variant, T=3):
    env = make(n, seed=23, kernel_variant=variant, copy=False)
    try:
        env.reset(seed=23)
        out = buffers(n)
        steps = []
        for a in actions(n, T):
            assert env.step_raw(a, *out) == 0
            steps.append(snapshot(*out))
        torch.cuda.synchronize()
        return steps, env.state_blob()
    finally:
        env.close()


@gpu
@pytest.mark.parametrize("n", (1, 2, 3, 127, 128, 129, 255))
@pytest.mark.parametrize("shape", SHAPES)
def test_lone_env_and_block_edges(shape, n):
    """3 steps from a seeded reset.  128-env blocks: n = 1, 3 run only the general body, 128 only the
    full-pair one, 129 and 255 both in one launch; 16-env blocks split the same counts elsewhere."""
    ref, rblob = plain_rollout(n, KIND1)
    got, blob = plain_rollout(n, shape)
    for t, (x, y) in enumerate(zip(ref, got)):
        for name, p, q in zip(("obs", "reward", "terminated", "truncated", "final_obs"), x, y):
            same(q, p, f"n={n} {shape} step {t} {name}")
    same(blob, rblob, f"n={n} {shape} state")


# --------------------------------------------------------------------------- 2. row layouts, obs alignment
SENTINEL = np.int32(-0x21524111)                   # 0xDEADBEEF


def offset_step(variant, k, n=130, limit=4):
    """One step with obs and final_obs at dword offset k of a 32-B sector, in sentinel-filled buffers.
    Envs 0, 1, 64 and the last reach the time limit, so their final_obs rows are written too."""
    env = make(n, seed=31, kernel_variant=variant, copy=False, max_episode_steps=limit)
    try:
        env.reset(seed=31)
        el = np.zeros(n, np.int32)
        el[[0, 1, 64, n - 1]] = limit - 1
        env.set_field("elapsed", el)
        pad, m = 8 + k, n * OBS
        big = [torch.full((m + 32,), int(SENTINEL), dtype=torch.int32, device="cuda") for _ in range(2)]
        obs, fobs = (b.view(torch.float32)[pad:pad + m].view(n, OBS) for b in big)
        assert (obs.data_ptr() // 4) % 8 == k and (fobs.data_ptr() // 4) % 8 == k
        _, rew, term, trunc, _ = buffers(n)
        assert env.step_raw(actions(n, 1)[0], obs, rew, term, trunc, fobs) == 0
        torch.cuda.synchronize()
        assert trunc[[0, 1, 64, n - 1]].all()
        for b, name in zip(big, ("obs", "final_obs")):
            h = b.cpu().numpy()
            assert (h[:pad] == SENTINEL).all(), f"{variant} offset {k}: dwords before the {name} rows were written"
            assert (h[pad + m:] == SENTINEL).all(), f"{variant} offset {k}: dwords after the {name} rows were written"
        return snapshot(obs, rew, term, trunc, fobs)
    finally:
        env.close()


@gpu
@pytest.mark.parametrize("n", (130, 129))
@pytest.mark.parametrize("variant", (SPAN_ON, SPAN_OFF))
def test_row_layouts_at_every_obs_alignment(variant, n):
    """n = 130 (a full block and a block of one pair) and 129 (a full block and a lone env, whose row a
    SPAN kernel stores in pieces, header included): the span shift takes every value 0..7."""
    ref = offset_step(variant, 0, n)
    for name, p, q in zip(("obs", "reward", "terminated", "truncated", "final_obs"), offset_step(KIND1, 0, n), ref):
        same(q, p, f"{variant} n={n} against the wave kernel: {name}")
    for k in range(1, 8):
        for name, p, q in zip(("obs", "reward", "terminated", "truncated", "final_obs"), ref, offset_step(variant, k, n)):
            same(q, p, f"{variant} n={n} offset {k} {name}")


# --------------------------------------------------------------------------- 3. DONE and INFO variants
def api_rollout(variant, mode, n=129, T=4, limit=3):
    """mode "plain": usv_step; "done": usv_step_ex with the done mask; "info": also with info rows."""
    env = make(n, seed=41, kernel_variant=variant, copy=False, max_episode_steps=limit, info=mode == "info")
    try:
        env.reset(seed=41)
        out = buffers(n)
        steps = []
        for a in actions(n, T):
            if mode == "plain":
                assert env.step_raw(a, *out) == 0
                steps.append(snapshot(*out))
            else:
                o, r, te, tr, info = env.step(a)
                assert torch.equal(info["_final_obs"], te | tr), "done mask != terminated | truncated"
                steps.append(snapshot(o, r, te.to(torch.uint8), tr.to(torch.uint8), info["final_obs"]))
        torch.cuda.synchronize()
        return steps, env.state_blob()
    finally:
        env.close()


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_done_and_info_variants(shape):
    ref, rblob = api_rollout(shape, "plain")
    assert any(s[3].any() for s in ref), "no env reached the time limit"
    for mode in ("done", "info"):
        got, blob = api_rollout(shape, mode)
        for t, (x, y) in enumerate(zip(ref, got)):
            for name, p, q in zip(("obs", "reward", "terminated", "truncated", "final_obs"), x, y):
                same(q, p, f"{shape} {mode} step {t} {name}")
        same(blob, rblob, f"{shape} {mode} state")


# --------------------------------------------------------------------------- 4. same-step reset, both bodies
@functools.lru_cache(maxsize=None)
def reset_rollout(variant, n=129, limit=5):
    env = make(n, seed=53, kernel_variant=variant, copy=False, max_episode_steps=limit)
    try:
        env.reset(seed=53)
        el = np.zeros(n, np.int32)
        el[[0, 1, 127, n - 1]] = limit - 1
        env.set_field("elapsed", el)
        out = buffers(n)
        steps = []
        for a in actions(n, 2):
            assert env.step_raw(a, *out) == 0
            steps.append(snapshot(*out) + (out[3].cpu().numpy().copy(),))
        torch.cuda.synchronize()
        return steps, env.state_blob()
    finally:
        env.close()


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_same_step_reset_through_both_loop_versions(shape):
    """n = 129, 128-env blocks: envs 0, 1 (one pair) and 127 (an env B) are reset from the full-pair
    body, the lone env 128 from the general one."""
    ref, rblob = reset_rollout(KIND1)
    got, blob = reset_rollout(shape)
    assert ref[0][5][[0, 1, 127, 128]].all()
    for t, (x, y) in enumerate(zip(ref, got)):
        for name, p, q in zip(("obs", "reward", "terminated", "truncated", "final_obs"), x, y):
            same(q, p, f"{shape} step {t} {name}")
    same(blob, rblob, f"{shape} state")


# --------------------------------------------------------------------------- 5. mark placement
def _narrow(cnt, ray, j):
    """An obstacle whose window and hits are exactly rays ray .. ray + cnt - 1 (true half-width 0.3 / 0.8 /
    1.3 rays about their middle, so the next ray on either side is >= 0.2 ray outside the sized window)."""
    d = 6.0 + 0.5 * j
    return (ray + 0.5 * (cnt - 1), d, d * np.sin((0.3, 0.8, 1.3)[cnt - 1] * LS.RES))


def _row(cnts, ray0=2):
    """Narrow obstacles of the given pair counts in lane order, on rays ray0, ray0 + 3, ..."""
    return [_narrow(c, ray0 + 3 * j, j) for j, c in enumerate(cnts)]


# contains the boat (128 pairs); bears into the blind sector, so it hits rays 64..127 and rays 0..63 stay
# with the narrow obstacles of its env
_INSIDE = (159.5, 0.2, 1.7)
_TO63 = [3] * 21 + [1]                             # 63 pairs, then a run that starts at pair 63
# (env A's counts, env B's counts or None for the wide obstacle first) per pair; (class, starts to find)
PAIRS = (
    (_TO63, "blind", 0, (63,)),                              # W = 64: one pass, full
    (_TO63 + [3], [2] * 10, 1, (63, 64)),                    # W = 87
    ("inside", [], 1, ()),                                   # W = 128: the boat inside, env B empty
    (_TO63 + [3] * 10, [3] * 11 + [1, 3] + [2] * 5, 2, (63, 64, 127, 128)),   # W = 141
    ("inside+", [2] * 10, 2, (128,)),                        # W = 157: wide first, runs from 128 on
    ([2] * 10, _TO63 + [3], 1, ()),                          # W = 87: env B's run across pass 1's start
    ([], _TO63 + [3], 1, (63, 64)),                          # W = 67: env A empty
    ([2] * 32, [3] + [2] * 31, 2, (64, 127)),                # W = 129: pass 0 filled exactly, one pair in pass 2
)
LONE = _TO63 + [3] * 10                                      # W = 94, no env B (the general body, two passes)


def _lanes(spec):
    if spec == "blind":
        return [LS._BLIND]
    if spec == "inside":
        return [_INSIDE]
    if spec == "inside+":
        return [_INSIDE] + _row([3, 3, 3])
    return _row(spec)


@functools.lru_cache(maxsize=None)
def scene():
    envs = []
    for p, (a, b, _, _) in enumerate(PAIRS):
        envs += [(LS.PSIS[p % 3], _lanes(a)), (LS.PSIS[p % 3], _lanes(b))]
    envs.append((LS.PSIS[1], _lanes(LONE)))
    return LS._scene(envs, family=2)


@functools.lru_cache(maxsize=None)
def geometry():
    """Per (env, ray, obstacle) float64 geometry of the scene, as the oracle computes it (lidar_scenes.geometry
    for a batch that is not one of its named ones)."""
    sc = scene()
    px, py, psi = sc["pos"][:, 0], sc["pos"][:, 1], sc["pos"][:, 2]
    valid = np.arange(sc["ox"].shape[1])[None, :] < sc["n_obs"][:, None]
    dx, dy = sc["ox"] - px[:, None], sc["oy"] - py[:, None]
    ang = (LS.START + np.arange(128) * LS.RES)[None, :] + psi[:, None]
    c, s = np.cos(ang)[:, :, None], np.sin(ang)[:, :, None]
    proj = c * dx[:, None, :] + s * dy[:, None, :]
    perp = s * dx[:, None, :] - c * dy[:, None, :]
    return dict(valid=valid, dx=dx, dy=dy, d=np.hypot(dx, dy), proj=proj, delta=sc["orad"][:, None, :] ** 2 - perp * perp)


def clear_rays():
    """lidar_scenes' clear-ray rule: every valid obstacle is a clear hit or a clear miss on the ray."""
    sc, g = scene(), geometry()
    d, r2 = g["d"][:, None, :], (sc["orad"] ** 2)[:, None, :]
    miss = (g["proj"] <= -1e-3 * d) | (g["delta"] <= -1e-2 * r2)
    hit = (g["proj"] >= 1e-3 * d) & (g["delta"] >= 1e-2 * r2)
    return (miss | hit | ~g["valid"][:, None, :]).all(axis=2)


def oracle_readings():
    from oracle import usv_oracle as O
    sc = scene()
    return O.lidar(sc["pos"][:, 0], sc["pos"][:, 1], sc["pos"][:, 2], sc["ox"], sc["oy"], sc["orad"], sc["n_obs"])[1]


def geometric_counts():
    """Pairs per (env, obstacle): the rays within asin(r / d) of the bearing, all 128 with the boat inside
    (lidar_scenes.window_pairs)."""
    sc, g = scene(), geometry()
    half = np.arcsin(np.clip(sc["orad"] / np.maximum(g["d"], 1e-9), 0, 1))
    ray = sc["pos"][:, 2:3, None] + LS.START + LS.RES * np.arange(128)[None, None, :]
    diff = np.angle(np.exp(1j * (ray - np.arctan2(g["dy"], g["dx"])[:, :, None])))
    return np.where(g["d"] <= sc["orad"], 128, (np.abs(diff) <= half[:, :, None]).sum(2)) * g["valid"]


def kernel_counts():
    """Pairs per (env, obstacle) by lidar_window2's float32 window sizing (hr_f32), from the float64 bearing."""
    sc, g = scene(), geometry()
    pr = (np.arctan2(g["dy"], g["dx"]) - sc["pos"][:, 2:3] - LS.START) / LS.RES
    pr = (pr + 32.5) % 192.0 - 32.5
    hr = LS.hr_f32(sc["orad"] / np.maximum(g["d"], 1e-9)).astype(np.float64)
    lo = np.where(hr >= 32.0, 0, np.maximum(0, np.ceil(pr - hr)))
    hi = np.where(hr >= 32.0, 127, np.minimum(127, np.floor(pr + hr)))
    return (np.maximum(0, hi - lo + 1) * g["valid"]).astype(int)


def check_scene_classes():
    """Each pair's expanded list has the intended size class and run starts, by the geometric pair count
    and by the kernel's own window sizing alike."""
    geo, ker = geometric_counts(), kernel_counts()
    assert np.array_equal(geo, ker), "window sizing and geometric pair counts disagree"
    cnt = np.zeros((len(PAIRS) + 1, 64), int)
    for e in range(geo.shape[0]):
        cnt[e // 2, 32 * (e % 2):32 * (e % 2) + geo.shape[1]] = geo[e]
    for p, (_, _, cls, starts) in enumerate(PAIRS + ((LONE, [], 1, (63, 64)),)):
        W = int(cnt[p].sum())
        assert (W <= 64, 64 < W <= 128, W > 128)[cls], f"pair {p}: W = {W}"
        run_starts = set((np.cumsum(cnt[p]) - cnt[p])[cnt[p] > 0].tolist())
        assert set(starts) <= run_starts, f"pair {p}: runs start at {sorted(run_starts)}"
    assert 128 in cnt                                # one obstacle holds all 128 rays
    return cnt


def test_scene_classes_on_the_cpu():
    cnt = check_scene_classes()
    assert [int(c.sum()) for c in cnt] == [64, 87, 128, 141, 157, 87, 67, 129, 94]


def scan(variant, order=None):
    st = LS.scene_state(scene(), 32, order)
    n = len(st["n_obs"])
    env = make(n, autoreset=False, max_episode_steps=0, kernel_variant=variant)
    try:
        env.set_state(st)
        obs, *_ = env.step(torch.zeros(n, 2, device="cuda"))
        torch.cuda.synchronize()
        return obs[:, 15:].detach().cpu().numpy().copy()
    finally:
        env.close()


@functools.lru_cache(maxsize=None)
def brute_scan():
    a = scan(BRUTE)
    a.setflags(write=False)
    return a


@gpu
def test_brute_scan_matches_oracle_on_clear_rays():
    check_scene_classes()
    want, clear = oracle_readings(), clear_rays()
    assert clear.mean() >= 0.9
    got = brute_scan().astype(np.float64) * 100.0
    bad = clear & ~(np.abs(got - want) <= F32_ATOL + F32_RTOL * np.abs(want))
    if bad.any():
        i, k = (int(v) for v in np.argwhere(bad)[0])
        pytest.fail(f"{int(bad.sum())} clear rays off; first: env {i} ray {k}: {got[i, k]!r} vs oracle {want[i, k]!r} m")
    assert (got < 100.0).any() and (got == 100.0).any()


@gpu
@pytest.mark.parametrize("variant", SHAPES + (SPAN_ON,))
def test_mark_placement(variant):
    """All 17 envs (128-env blocks: the general body; 16-env blocks: a full block, then the lone env) and
    the first 16 alone (an even count: the full-pair body in either shape)."""
    check_scene_classes()
    ref = brute_scan()
    for order in (None, np.arange(16)):
        got = scan(variant, order)
        want = ref if order is None else ref[order]
        bad = got.view(np.uint32) != want.view(np.uint32)
        if bad.any():
            i, k = (int(v) for v in np.argwhere(bad)[0])
            pytest.fail(f"{variant}, {got.shape[0]} envs: {int(bad.sum())} readings differ from the brute lidar; "
                        f"first: env {i} ray {k}: {100.0 * got[i, k]!r} vs {100.0 * want[i, k]!r} m")
