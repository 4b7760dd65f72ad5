"""Deterministic edge scenes for the 128-ray lidar, and the clear-ray rule (plain numpy, no GPU).

One env is one scene: a pose inside the 20 m field and obstacles placed by bearing and distance.
A bearing `theta` is measured in rays from ray 0 (ray 0 looks along psi - 120 deg, ray i along
psi - 120 deg + i * RES; 192 rays make a full turn, rays 0..127 exist, (127, 192) is the blind sector).

Families (batch names in brackets):
  1 [sweep]    one obstacle swept over the full turn, finely around the blind-sector edges (rays 0
               and 127) and the window kernels' branch cut (159.5 rays), at r/d ratios on either side
               of every threshold of the window sizing (SWEEP_RATIOS);
  2 [lists32]  cap 32, envs 2i / 2i+1 hold kA / kB obstacles that contain the boat (128 pairs each in
               the two-env-per-wave kernels: 0 to 128 passes of 64 per wave), plain and with narrow
               obstacles interleaved in lane order; [single32] is one such env on its own (n = 1);
  3 [lists64]  the same at cap 64 (one env per wave), k in 33..64;
  4 [range]    obstacles either side of max range (100 m) and of the `far` switch at 99 m, among them
               pairs where the min-key obstacle's off-centre ray reads >= 100 and the reading falls
               through to a larger-key obstacle (usv_asmc_ca_env.py:458), far and near scenes as
               neighbouring envs.

The clear-ray rule.  The float32 kernels may legitimately flip hit / miss on a ray that grazes an
obstacle's edge or is perpendicular to its bearing, so the comparison with the float64 oracle runs
on *clear* rays only.  Per (ray, obstacle), with proj, perp and delta = r^2 - perp^2 as in the oracle
and d the centre distance:
    clear miss:  proj <= -1e-3 d   or   delta <= -1e-2 r^2
    clear hit:   proj >=  1e-3 d   and  delta >=  1e-2 r^2
                 (family 4 also: |reading - 100| >= 1e-2, so the max-range test cannot flip)
and a ray is clear if every valid obstacle is a clear hit or a clear miss on it.  Why 1e-2: the
float32 error of perp is about 6 * 2^-24 * d (the rounded coordinates, the rotation into the ray-0
frame and the ray table), which moves delta by at most 2 |perp| * 3.6e-7 d <= 7e-7 d r.  With
delta >= 1e-2 r^2 the square root moves by at most 7e-7 d r / (2 * 0.1 r) = 3.6e-6 d: 3.6e-4 m at
d = 100 m, inside the 1e-3 m tolerance of the float32 comparison.  A flip of the hit test itself
needs 7e-7 d r >= 1e-2 r^2, i.e. r / d < 7e-5, and the smallest ratio used here is 8.3e-4.  The rule
is a filter, so tests/test_lidar_scenes.py caps what it may remove (2 % of a family's rays, 5 % of a
ratio group of family 1).
"""
import functools

import numpy as np

from oracle import usv_oracle as O

RES = O.SENSOR_RES                  # one ray, rad
START = O.SENSOR_START              # ray 0 relative to the heading (-120 deg)
MAX_RANGE = O.SENSOR_MAX_RANGE
POSE_XY = (7.0, 11.0)               # inside the 20 m field
PSIS = (0.0, 2.4, -17.3)            # 0, a generic heading, and one beyond two turns
WIN_MARGIN = 0.05                   # kWinMargin of usv_lidar.hpp, rays


# --------------------------------------------------------------------------- the kernel's window sizing
def hr_f32(x):
    """Half-width of the ray window in rays, as lidar_window2 / lidar_window_d size it in float32:
    (x + (pi/2 - 1) x^3 + margin) / res, an upper bound of asin(x) plus the margin (x = min(r/d, 1))."""
    x = np.minimum(np.float32(x), np.float32(1.0))
    margin = np.float32(WIN_MARGIN * RES)
    inv = np.float32(1.0 / RES)
    c = np.float32(np.float32(np.pi / 2 - 1) * x)
    poly = np.float32(np.float64(c) * np.float64(np.float32(x * x)) + np.float64(x))   # the fma
    return np.float32(np.float32(poly + margin) * inv)


def _hr(x):
    return (x + (np.pi / 2 - 1) * x ** 3) / RES + WIN_MARGIN


def ratio_at_hr(hr):
    """r/d at which the sizing formula gives `hr` rays (bisection on the float64 formula)."""
    lo, hi = 0.0, 1.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _hr(mid) < hr else (lo, mid)
    return 0.5 * (lo + hi)


# The `wide` switches: hr >= 32.0 (f32, lidar_window2) and hr >= 32.5 (f64, lidar_window_d /
# lidar_wave2_d).  Solved from the kernel's own formula: r/d = 0.7776 and 0.7856 (not the round
# 0.8 one would guess from asin alone: the cubic bound overshoots asin by ~5 rays there).
X_WIDE32 = ratio_at_hr(32.0)
X_WIDE64 = ratio_at_hr(32.5)
_DX = 0.002                          # (X_WIDE64 - X_WIDE32 = 0.008: the four ratios stay ordered)
# Why the switches must sit where they do: phi is taken in [-32.5, 159.5) rays, so a window that is not
# `wide` loses the rays it would reach across that cut.  That is harmless while the obstacle's true
# half-width asin(r/d) stays below 32.5 rays (r/d < 0.874, where the formula gives hr = 37.7).  The ratio
# below has a true half-width of 33.5 rays at hr = 39.5: wide today, and the first to lose rays 0 / 127
# for bearings next to the cut if a switch moved up.
X_WRAP = ratio_at_hr(39.5)

# (label, r, d).  hr by the formula above: 8.3e-4 -> 0.08 rays (a window of 0 or 1 ray), 0.02 -> 0.66
# (1 or 2 rays), 0.16 -> 5.01, the four `wide` ratios -> 31.87 / 32.13 (f32 switch at 32.0) and
# 32.37 / 32.63 (f64 switch at 32.5), X_WRAP -> 39.5 and 0.9 -> 40.3 (wide in both), d = 1.002 r and
# 1.0005 r either side of `inside` (d <= 1.001 r; both wide), and d = r / 2 with the boat inside the obstacle.
SWEEP_RATIOS = (
    ("8.3e-4", 0.05, 60.0),
    ("0.02", 1.0, 50.0),
    ("0.16", 1.0, 6.25),
    ("wide32-", 1.0, 1.0 / (X_WIDE32 - _DX)),
    ("wide32+", 1.0, 1.0 / (X_WIDE32 + _DX)),
    ("wide64-", 1.0, 1.0 / (X_WIDE64 - _DX)),
    ("wide64+", 1.0, 1.0 / (X_WIDE64 + _DX)),
    ("wrap", 1.0, 1.0 / X_WRAP),
    ("0.9", 1.0, 1.0 / 0.9),
    ("1/1.002", 1.0, 1.002),
    ("1/1.0005", 1.0, 1.0005),
    ("2", 1.0, 0.5),
)


def sweep_thetas():
    """Bearings of family 1 in rays, in [-96, 96): quarter-ray steps over the full turn, 1/16-ray steps
    within 6 rays of rays 0 and 127 and within 3 rays of the branch cut at 159.5 (all exact in binary)."""
    t = [np.arange(-96.0, 96.0, 0.25)]
    for c in (0.0, 127.0):
        t.append(c + np.arange(-96, 97) / 16.0)
    t.append(159.5 + np.arange(-48, 49) / 16.0)
    t = (np.concatenate(t) + 96.0) % 192.0 - 96.0
    return np.unique(t)


# --------------------------------------------------------------------------- scene assembly
def _scene(envs, **meta):
    """envs: list of (psi, [(theta, d, r), ...]) -> arrays like tests/golden/lidar.npz."""
    n = len(envs)
    m = max(1, max(len(obs) for _, obs in envs))
    pos = np.zeros((n, 3))
    pos[:, 0], pos[:, 1] = POSE_XY
    ox, oy, orad = np.zeros((n, m)), np.zeros((n, m)), np.zeros((n, m))
    n_obs = np.zeros(n, np.int32)
    for i, (psi, obs) in enumerate(envs):
        pos[i, 2] = psi
        n_obs[i] = len(obs)
        if obs:
            th, d, r = (np.array(v, dtype=np.float64) for v in zip(*obs))
            ang = psi + START + th * RES
            ox[i, :len(obs)] = POSE_XY[0] + d * np.cos(ang)
            oy[i, :len(obs)] = POSE_XY[1] + d * np.sin(ang)
            orad[i, :len(obs)] = r
    sc = dict(pos=pos, ox=ox, oy=oy, orad=orad, n_obs=n_obs, **meta)
    for v in sc.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc


def build_sweep():
    th = sweep_thetas()
    envs, ratio, theta = [], [], []
    for psi in PSIS:
        for g, (_, r, d) in enumerate(SWEEP_RATIOS):
            for t in th:
                envs.append((psi, [(t, d, r)]))
                ratio.append(g)
                theta.append(t)
    return _scene(envs, family=1, ratio=np.array(ratio), theta=np.array(theta))


# Families 2 and 3.  Wide obstacle j contains the boat: centre offset d <= 0.4 <= 0.5 r, at a bearing on
# a half-ray offset (so every ray is >= 0.5 ray = 0.016 rad from perpendicular to it: proj is clear),
# keys d - r = -(1 + 0.01 * a permutation of j): distinct by 0.01 m and not in lane order.
def _wide(j):
    key = -(1.0 + 0.01 * ((37 * j) % 64))
    d = 0.1 + 0.3 * ((11 * j) % 64) / 64.0
    return (((29 * j) % 192) - 96 + 0.5, d, d - key)


# Narrow obstacle i covers exactly 1, 2 or 3 rays: centred on a ray (or between two) with a true
# half-width of 0.3 / 0.8 / 1.3 rays, so its hit rays sit well inside the disc and the next ones well
# outside (clear either way); keys (about 0.96 d) are distinct and above every wide key.
def _narrow(i):
    nr = 1 + i % 3
    hw = (0.3, 0.8, 1.3)[i % 3]
    d = 5.0 + 0.25 * i
    return ((5 + 7 * i) % 120 + (0.5 if nr == 2 else 0.0), d, d * np.sin(hw * RES))


_BLIND = (150.0, 10.07, 0.2)         # wholly inside the blind sector: no ray, no pair


def list_env(k, cap, interleaved):
    """Lane-ordered obstacles of one long-list env with k wide obstacles.  Interleaved: a blind-sector
    obstacle at lane 0 (no pairs, so pair 0's owner is a later lane), then the wide ones with a narrow
    one after each while lanes last (runs then start off multiples of 64); the wide count is cut to
    cap - 1 and the narrow ones to the lanes left, so k = cap gives the blind one and cap - 1 wide."""
    if not interleaved:
        return [_wide(j) for j in range(k)]
    kw = min(k, cap - 1)
    extras = min(cap - 1 - kw, kw)
    lanes = [_BLIND]
    for j in range(kw):
        lanes.append(_wide(j))
        if j < extras:
            lanes.append(_narrow(j))
    return lanes


LIST_K32 = (0, 1, 2, 3, 16, 31, 32)
LIST_K64 = (33, 48, 63, 64)


def build_lists32():
    envs, ka, kb, inter = [], [], [], []
    for il in (False, True):
        for a in LIST_K32:
            for b in LIST_K32:
                psi = PSIS[len(envs) // 2 % 3]
                envs += [(psi, list_env(a, 32, il)), (psi, list_env(b, 32, il))]
                ka.append(a), kb.append(b), inter.append(il)
    envs.append((PSIS[2], list_env(32, 32, False)))          # odd length: the last env has no companion
    return _scene(envs, family=2, ka=np.array(ka), kb=np.array(kb), inter=np.array(inter))


def _arc_env(narrow):
    """A row whose 24 wide obstacles all bear into the 72 rays around the blind sector's centre (theta
    = (29 j) % 192 - 95.5 with the residue in 28..99, i.e. in [-67.5, 3.5]), so rays 52..76 face away from every one of them and keep max-range and
    narrow-obstacle readings (with 31 or more wide ones every ray reads the inside of a disc): the
    blind obstacle, then the wide ones with the given narrow ones after them, one each while they last,
    the rest at the end."""
    js = [j for j in range(64) if 28 <= (29 * j) % 192 < 100][:24]      # the first 24 of 26
    assert len(js) == 24
    narrow = list(narrow)
    lanes = [_BLIND]
    for j in js:
        lanes.append(_wide(j))
        if narrow:
            lanes.append(_narrow(narrow.pop(0)))
    return lanes + [_narrow(i) for i in narrow]


def build_single32():
    """n = 1: a full row of 32 (48 passes, and no env B in the wave)."""
    return _scene([(PSIS[2], _arc_env(range(5, 12)))], family=2)       # narrow ones on rays 40 .. 82


def build_lists64():
    envs = [(PSIS[i % 3], list_env(k, 64, il)) for il in (False, True) for i, k in enumerate(LIST_K64)]
    envs.append((PSIS[1], _arc_env(range(39))))              # a full row of 64 with max-range rays left
    return _scene(envs, family=3, k=np.array(LIST_K64 * 2 + (24,)),
                  inter=np.repeat([False, True], [len(LIST_K64), len(LIST_K64) + 1]))


def build_range():
    far = []
    # one obstacle either side of the `far` switch (d >= 99) and of max range: on a ray (reads d - r),
    # and 0.27 / 0.454 ray off one, where r = 1 / r = 1.6 read just below 100 at d = 100.4 and above at 101
    for d in (98.9, 99.1, 100.4, 101.0):
        for r in (1.0, 1.6):
            for th in (40.0, 70.27, 90.454):
                far.append([(th, d, r)])
    # fall-through: the min-key obstacle's off-centre ray reads >= 100 (101 / 1.6 at 0.454 ray: 100.43;
    # 104 / 6 at 1.5 rays: 100.7) and a larger-key obstacle (99.9 / 0.3, reads 99.6) lies on that ray
    for k in (30, 100):
        a = [(k + 0.454, 101.0, 1.6), (float(k), 99.9, 0.3)]
        b = [(k + 0.5, 104.0, 6.0), (k + 2.0, 99.9, 0.3)]
        far += [a, a[::-1], b, b[::-1]]
    near = [[(20.5 + i, 12.0, 1.0), (60.0 + i, 30.0, 2.0), _BLIND] for i in range(len(far))]
    envs, is_far = [], []
    fi = ni = 0
    for i in range(2 * len(far)):                # F N N F F N N F ...: far as env A and as env B
        f = i % 4 in (0, 3)
        envs.append((PSIS[i % 3], far[fi] if f else near[ni]))
        is_far.append(f)
        fi, ni = fi + f, ni + (not f)
    envs.append((PSIS[0], far[-1]))              # odd length
    is_far.append(True)
    return _scene(envs, family=4, is_far=np.array(is_far))


_BUILDERS = {"sweep": build_sweep, "lists32": build_lists32, "single32": build_single32,
             "lists64": build_lists64, "range": build_range}
BATCHES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def batch(name):
    """The named batch (read-only arrays, built once)."""
    return _BUILDERS[name]()


def scene_state(sc, cap, order=None):
    """Env state for a zero-velocity injection of the scenes (in `order`, if given)."""
    o = np.arange(sc["pos"].shape[0]) if order is None else np.asarray(order)
    p = sc["pos"][o]
    n = len(o)
    st = {"x": p[:, 0], "y": p[:, 1], "psi": p[:, 2], "u": 0.0, "v": 0.0, "r": 0.0, "last_u": 0.0,
          "last_r": 0.0, "progress": 0.0, "path_x0": 0.0, "path_y0": 0.0, "path_x1": 100.0, "path_y1": 0.0,
          "max_u": 3.0, "max_r": 3.0, "ref_v": 1.0, "n_obs": sc["n_obs"][o].astype(np.int32),
          "elapsed": 1, "scan_valid": 1}
    for k, f in (("obs_x", "ox"), ("obs_y", "oy"), ("obs_r", "orad")):
        a = np.zeros((n, cap))
        a[:, :sc[f].shape[1]] = sc[f][o]
        st[k] = a
    return st


# --------------------------------------------------------------------------- float64 geometry
@functools.lru_cache(maxsize=None)
def geometry(name):
    """Per (env, ray, obstacle) float64 geometry of a batch, as the oracle computes it."""
    sc = batch(name)
    px, py, psi = sc["pos"][:, 0], sc["pos"][:, 1], sc["pos"][:, 2]
    valid = np.arange(sc["ox"].shape[1])[None, :] < sc["n_obs"][:, None]
    dx, dy = sc["ox"] - px[:, None], sc["oy"] - py[:, None]
    d = np.hypot(dx, dy)
    ang = (START + np.arange(128) * RES)[None, :] + psi[:, None]
    c, s = np.cos(ang)[:, :, None], np.sin(ang)[:, :, None]
    proj = c * dx[:, None, :] + s * dy[:, None, :]
    perp = s * dx[:, None, :] - c * dy[:, None, :]
    delta = sc["orad"][:, None, :] ** 2 - perp * perp
    reading = proj - np.sqrt(np.maximum(delta, 0.0))
    return dict(valid=valid, d=d, key=np.where(valid, d - sc["orad"], np.inf), proj=proj, delta=delta,
                reading=reading)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle's readings [n, 128] of a batch (computed once, read-only)."""
    sc = batch(name)
    _, rd = O.lidar(sc["pos"][:, 0], sc["pos"][:, 1], sc["pos"][:, 2], sc["ox"], sc["oy"], sc["orad"], sc["n_obs"])
    rd.setflags(write=False)
    return rd


@functools.lru_cache(maxsize=None)
def clear_rays(name):
    """[n, 128] bool: the rays on which a float32 kernel cannot legitimately differ (module docstring)."""
    sc, g = batch(name), geometry(name)
    d, r2 = g["d"][:, None, :], (sc["orad"] ** 2)[:, None, :]
    miss = (g["proj"] <= -1e-3 * d) | (g["delta"] <= -1e-2 * r2)
    hit = (g["proj"] >= 1e-3 * d) & (g["delta"] >= 1e-2 * r2)
    if sc["family"] == 4:
        hit &= np.abs(g["reading"] - MAX_RANGE) >= 1e-2
    ok = (miss | hit | ~g["valid"][:, None, :]).all(axis=2)
    ok.setflags(write=False)
    return ok


def window_pairs(name):
    """Host count of (obstacle, ray) pairs per (env, obstacle), as _window_pairs of test_gpu_parity.py
    does it: the rays within asin(r / d) of the obstacle's bearing, all 128 when the boat is inside."""
    sc, g = batch(name), geometry(name)
    dx, dy = sc["ox"] - sc["pos"][:, :1], sc["oy"] - sc["pos"][:, 1:2]
    half = np.arcsin(np.clip(sc["orad"] / np.maximum(g["d"], 1e-9), 0, 1))
    ray = sc["pos"][:, 2:3, None] + START + RES * np.arange(128)[None, None, :]
    diff = np.angle(np.exp(1j * (ray - np.arctan2(dy, dx)[:, :, None])))
    cnt = np.where(g["d"] <= sc["orad"], 128, (np.abs(diff) <= half[:, :, None]).sum(2))
    return cnt * g["valid"]


def partner_shuffle(n):
    """A fixed order of n envs (n >= 3) in which every env has another wave partner (envs 2i, 2i+1
    share a wave) and the other half of the wave: the batch rotated by one."""
    return np.roll(np.arange(n), 1)


def describe(name, i, k):
    """One line naming env i's obstacles that geometrically hit ray k (for failure messages)."""
    sc, g = batch(name), geometry(name)
    hits = [f"#{j} d={g['d'][i, j]:.6g} r={sc['orad'][i, j]:.6g} key={g['key'][i, j]:.6g} "
            f"reads {g['reading'][i, k, j]:.9g}"
            for j in range(int(sc["n_obs"][i]))
            if g["proj"][i, k, j] >= 0 and g["delta"][i, k, j] >= 0]
    extra = "".join(f" {m}={sc[m][i]}" for m in ("theta", "ratio") if m in sc)
    return (f"batch {name} env {i} ray {k}: psi={sc['pos'][i, 2]} n_obs={int(sc['n_obs'][i])}{extra}; "
            f"oracle {reference(name)[i, k]:.9g}; geometric hits: " + ("; ".join(hits) or "none"))
