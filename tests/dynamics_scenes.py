"""Deterministic edge states for the step's dynamics, reward and flag compares (plain numpy, no GPU).

One env is one scene: an injected state next to one branch or cut of env_dynamics (csrc/usv_dynamics.hpp),
of the f32 heading frame (csrc/usv_state.hpp) or of the termination / collision compares, and its
actions for T = 3 steps.  Step 1 takes the edge (a few scenes take it in step 2); the later steps consume
what it stored: the rebased heading, the clamped progress, the filtered action.

Every scene is labelled with the deciding quantity it sits next to (`q`, a row of trace()), the side it
must fall on (`side`: the sign of that quantity, 0 = exactly on the threshold), the step (`step`, from 1)
and the distance it keeps from the threshold (`margin`).  All quantities are written as value minus
threshold, so the threshold is always 0:

  acc_u_lo / acc_u_hi   (a3 - vel)[surge] + 1.75 / - 1.75           (simple_env.py:320)
  acc_r_lo / acc_r_hi   (a3 - vel)[yaw]   + 3.0  / - 3.0
  spd_u_lo / spd_u_hi   (vel + dv)[surge] + max_action / - max_action (:321); spd_r_* likewise
  prog_lo / prog_hi     projected a + lookahead, minus progress / minus 1 (:147)
  x_lo, x_hi, y_lo, y_hi  position minus 0 / minus 20 (:336, strict inequalities)
  tl                    elapsed - limit after the step (TimeLimit: truncated when >= 0)
  oct_dx, oct_dy, oct_diag  target - position: dx, dy, |dy| - |dx| (the octant folds of fx_atan2)
  cut                   |atan2(target - position) - psi| - pi before wrapping (:69)
  dist                  distance to target minus 2e-3
  ye_k                  |ye| - 0.075: the crossover of exp(-|ye/k|) and exp(-(ye/k)^2) (:167-170)
  ye                    ye itself (side 0: exactly zero; `negzero` scenes: the zero is -0.0)
  rebase                the whole turns the f32 heading frame moves into k after the step (+-1, else 0)
  asmc_wrap             |yaw action| - pi: the arm of usv_asmc.py:120 (usv-asmc-simple; v = 0 at the start)
  key                   min(d - r) - 0.05 (:334);  coll: min reading - 0.2 (:155)

Batches (`limit` is the handle's max_episode_steps, 0 = none): clips, progress, angle, ye, bounds,
timelimit (limit 3) and timelimit0 (the same scenes, limit 0), heading, contact, and contact64 (the contact
scenes 1e-9 m from their thresholds: f64 build only).  Every scene has one obstacle; where the family is
not about obstacles it lies 150 m away, beyond max range from every pose, so all 128 rays read 100.

Not covered: non-finite actions, a zero-length path and max_action[0] = 0, where the reference itself
returns NaN.
"""
import functools

import numpy as np

from oracle import usv_oracle as O

T = 3
PI = np.pi
CAP = 32
YE_K = 0.075
F32 = np.float32

_DEF = dict(x=10.0, y=10.0, psi=0.3, u=0.0, r=0.0, last_u=0.0, last_r=0.0, progress=0.0,
            path=(10.0, 10.0, 110.0, 10.0), max_u=2.0, max_r=4.0, ref_v=1.0, elapsed=1, asmc0=None,
            obst=None, actions=((0.0, 0.0),) * T, q="", side=0, step=1, margin=0.0, note="", negzero=False)


def _S(**kw):
    s = dict(_DEF)
    bad = set(kw) - set(s)
    assert not bad, bad
    s.update(kw)
    return s


def _path(x0, y0, theta, length):
    """Path from (x0, y0) along theta; axis and diagonal directions get exact components."""
    c, s = np.cos(theta), np.sin(theta)
    for v in (0.0, 1.0, -1.0, np.sqrt(0.5), -np.sqrt(0.5)):
        c = v if abs(c - v) < 1e-12 else c
        s = v if abs(s - v) < 1e-12 else s
    if abs(abs(c) - abs(s)) < 1e-12:                 # a diagonal: |dx| == |dy| exactly
        c, s = np.sign(c) * 0.75, np.sign(s) * 0.75
    return (x0, y0, x0 + length * c, y0 + length * s)


def _on_path(p, s, lateral=0.0):
    """The point s metres along path p and `lateral` metres to its left."""
    d = np.array([p[2] - p[0], p[3] - p[1]])
    d = d / np.hypot(*d)
    return p[0] + s * d[0] - lateral * d[1], p[1] + s * d[1] + lateral * d[0]


# --------------------------------------------------------------------------- families
def build_clips():
    sc = []
    acts = (-5.0, -1.0, -0.0, 0.0, 1.0, 5.0)

    def chan(ch, mx, acc):
        out, i = [], 0
        d = 0.01
        # (vel, a3 - vel): the acceleration clip below / inside / above either bound, the speed inside
        cases = [(0.1, v, f"acc_{ch}_lo", np.sign(v + acc), min(abs(v + acc), 0.3)) for v in (-acc - 0.75, -acc - d, -acc + d)]
        cases += [(0.1, v, f"acc_{ch}_hi", np.sign(v - acc), min(abs(v - acc), 0.3)) for v in (0.3, acc - d, acc + d, acc + 0.75)]
        # the speed clip below / inside / above either bound (negative speeds among them)
        for sg in (1.0, -1.0):
            name = f"spd_{ch}_{'hi' if sg > 0 else 'lo'}"
            cases += [(sg * (mx - 0.1), sg * dv, name, sg * np.sign(dv - 0.1), min(abs(dv - 0.1), 0.3)) for dv in (0.5, 0.099, 0.101)]
            cases += [(sg * (mx - 1.5), sg * (acc + 0.01), name, sg, acc - 1.5)]     # both clips at once
        cases += [(-1.0, 0.2, f"spd_{ch}_lo", 1, 0.5)]
        for vel, dv, q, side, margin in cases:
            a = acts[i % len(acts)]
            i += 1
            last = (dv + vel - 0.2 * mx * a) / 0.8
            out.append((vel, last, a, q, int(side), 0.9 * margin))
        return out

    for vel, last, a, q, side, margin in chan("u", 2.0, O.MAX_ACC[0]):
        sc.append(_S(u=vel, last_u=last, r=0.2, last_r=0.2, actions=((a, 0.05), (-a, 0.3), (0.5, -0.5)),
                     q=q, side=side, margin=margin, note=f"surge action {a!r}"))
    for vel, last, a, q, side, margin in chan("r", 4.0, O.MAX_ACC[2]):
        sc.append(_S(r=vel, last_r=last, u=0.5, last_u=0.5, actions=((0.25, a), (0.3, -a), (0.5, -0.5)),
                     q=q, side=side, margin=margin, note=f"yaw action {a!r}"))
    return sc, 0


_DIRS = tuple(np.deg2rad(v) for v in (0.0, 90.0, 180.0, 270.0, 30.0, 120.0, 210.0, 300.0))
_LENGTHS = (1.0, 100.0, 110.0, 200.0)


def build_progress():
    sc = []
    for j, th in enumerate(_DIRS):
        for i, ln in enumerate(_LENGTHS if j % 4 == 0 else (_LENGTHS[j % 4],)):
            p = _path(10.0, 10.0, th, ln)
            f = 0.3 if ln == 1.0 else 0.02           # the boat's station along the path, as a fraction
            mv = dict(u=0.5, last_u=0.5, psi=th + 0.2, actions=((0.25, 0.1),) * T)
            x, y = _on_path(p, f * ln, 0.4)
            sc.append(_S(x=x, y=y, path=p, progress=0.5, q="prog_lo", side=-1, margin=0.05, note="clamp holds", **mv))
            sc.append(_S(x=x, y=y, path=p, progress=0.0, q="prog_lo", side=1, margin=0.01, note="inside", **mv))
            sc.append(_S(x=p[0], y=p[1], path=p, progress=O.LOOKAHEAD, psi=th, q="prog_lo", side=0,
                         note="a + lookahead == progress"))
            x, y = _on_path(p, 1.2 * ln, -0.3)
            sc.append(_S(x=x, y=y, path=p, progress=0.2, q="prog_hi", side=1, margin=0.1, note="past the path end", **mv))
            sc.append(_S(x=x, y=y, path=p, progress=1.0, q="prog_hi", side=1, margin=0.1, note="past the end, progress 1", **mv))
    return sc, 0


def build_angle():
    sc = []
    # the target 1 m ahead of a boat parked on the path start, the path on an octant boundary or 1e-3 rad off it
    for k in range(8):
        for off in (0.0, 1e-3, -1e-3):
            th = k * PI / 4 + off
            p = _path(10.0, 10.0, th, 100.0) if off == 0.0 else (10.0, 10.0, 10.0 + 100.0 * np.cos(th), 10.0 + 100.0 * np.sin(th))
            q = ("oct_dy", "oct_diag", "oct_dx", "oct_diag")[k % 4]
            # which way the quantity moves with theta on this boundary (|dy| - |dx| grows in quadrants 1 and 3)
            grow = {"oct_dy": np.cos(k * PI / 4), "oct_dx": -np.sin(k * PI / 4), "oct_diag": 1.0 if k in (1, 5) else -1.0}[q]
            sc.append(_S(path=p, q=q, side=int(np.sign(off) * np.sign(grow)), margin=0.5e-3 if off else 0.0,
                         note=f"target bearing {45 * k} deg {off:+g} rad"))
    # the angle to target either side of the +-pi cut (path along +x, target dead east of the boat)
    for sg in (1.0, -1.0):
        for d in (1e-2, 1e-3):
            for beyond in (-1.0, 1.0):
                sc.append(_S(psi=-sg * (PI + beyond * d), q="cut", side=int(beyond), margin=0.9 * d,
                             note=f"atan2 - psi = {sg:+g} (pi {beyond * d:+g})"))
    # 1e-3 m from the target: the path end of a 1 m path, progress clamped to 1
    for th in (0.0, np.deg2rad(120.0)):
        p = _path(10.0, 10.0, th, 1.0)
        x, y = _on_path(p, 1.0 - 1e-3)
        sc.append(_S(x=x, y=y, path=p, q="dist", side=-1, margin=0.5e-3, note="1e-3 m from the target"))
    return sc, 0


def build_ye():
    sc = []
    dirs = [np.deg2rad(v) for v in (0.0, 90.0, 180.0, 270.0, 40.0, 135.0, 220.0, 310.0)]
    for j, th in enumerate(dirs):
        p = _path(10.0, 10.0, th, 100.0 if j % 2 else 110.0)
        quadrant2 = np.sin(th) > 0 and np.cos(th) < 0
        sc.append(_S(path=p, psi=th, q="ye", side=0, negzero=bool(quadrant2),
                     note="parked on the path start" + (", second quadrant: ye = -0.0" if quadrant2 else "")))
    i = 0
    for sg in (1.0, -1.0):
        for ye, side, margin in ((YE_K * (1 - 1e-2), -1, 6e-4), (YE_K * (1 + 1e-2), 1, 6e-4), (1.0, 1, 0.5), (20.0, 1, 5.0)):
            for moving in (False, True):
                th = dirs[i % len(dirs)]
                i += 1
                p = _path(10.0, 10.0, th, 100.0)
                x, y = _on_path(p, 1.5, sg * ye)
                mv = dict(u=0.5, last_u=0.5, actions=((0.25, 0.0),) * T) if moving else {}
                sc.append(_S(x=x, y=y, psi=th, path=p, q="ye_k", side=side, margin=margin, note=f"ye = {sg * ye:+.6g}", **mv))
    return sc, 0


def build_bounds():
    sc = []
    hi = F32(O.BOUND_HI)
    edge = [(float(hi), "hi", 0), (float(np.nextafter(hi, F32(np.inf))), "hi", 1), (float(np.nextafter(hi, F32(-np.inf))), "hi", -1),
            (0.0, "lo", 0), (-0.0, "lo", 0), (-1.1754944e-38, "lo", -1)]
    for v, which, side in edge:                      # parked: the position is kept bit for bit
        sc.append(_S(x=v, q=f"x_{which}", side=side, note=f"parked at x = {v!r}"))
        sc.append(_S(y=v, q=f"y_{which}", side=side, note=f"parked at y = {v!r}"))
    # moving at 1 m/s (0.04 m a step) straight at an edge: across it by 2e-4 m in step 1 or 2, or short of it
    mv = dict(u=1.0, last_u=1.0, actions=((0.5, 0.0),) * T)
    for ax, which, psi in (("x", "hi", 0.0), ("x", "lo", PI), ("y", "hi", PI / 2), ("y", "lo", -PI / 2)):
        out = 1.0 if which == "hi" else -1.0
        e = O.BOUND_HI if which == "hi" else 0.0
        for step in (1, 2):
            for over in (2e-4, -2e-4):
                pos = e - out * (0.04 * step - over)
                sc.append(_S(**{ax: pos}, psi=psi, q=f"{ax}_{which}", side=int(np.sign(over) * out), step=step, margin=1e-4,
                             note=f"{ax} {'across' if over > 0 else 'short of'} {e:g} by 2e-4 m in step {step}", **mv))
    return sc, 0


def _timelimit(limit):
    sc = []
    for el, step in ((limit - 2, 2), (limit - 1, 1)) if limit else ((1, 2), (2, 1), (1000, 1)):
        for moving in (False, True):
            mv = dict(u=0.5, last_u=0.5, actions=((0.25, 0.1),) * T) if moving else {}
            sc.append(_S(elapsed=el, q="tl", side=0 if limit else -1, step=step, note=f"elapsed {el}, limit {limit}", **mv))
    return sc, limit


def build_heading():
    sc = []
    ks = (0, 1, -1, 40, -40, 256, -256, 257, -257, 100000, -100000)
    i = 0
    for k in ks:
        for phi, step in ((0.0, 0), (PI - 0.1, 1), (-(PI - 0.1), 1), (PI - 1e-3, 1), (-(PI - 1e-3), 1), (PI - 0.3, 2), (-(PI - 0.3), 2)):
            for inward in ((False, True) if (k in (0, 257) and phi) else (False,)):
                sg = (1.0 if phi >= 0 else -1.0) * (-1.0 if inward else 1.0)
                if phi == 0.0:
                    sg = 1.0 if i % 2 else -1.0
                i += 1
                psi = phi + 2 * PI * k
                side = 0 if (inward or phi == 0.0) else int(sg)
                sc.append(_S(psi=psi, r=sg * 6.0, last_r=sg * 6.0, max_r=6.0, u=0.5, last_u=0.5, asmc0=psi + 0.05,
                             actions=((0.25, sg),) * T, q="rebase", side=side, step=max(step, 1),
                             note=f"phi = {phi:+.4g}, k = {k}, yaw rate {sg * 6:+g}"))
    for a in (PI - 0.2, -(PI - 0.2), PI + 0.2, -(PI + 0.2)):
        for k in (0, 40):
            psi = 0.5 + 2 * PI * k
            sc.append(_S(psi=psi, asmc0=psi - 0.02, u=0.3, last_u=0.3, actions=((0.15, a),) * T, q="asmc_wrap",
                         side=int(np.sign(abs(a) - PI)), margin=0.19, note=f"yaw action {a:+.4g}"))
    return sc, 0


POSE = (7.0, 11.0)


def _offcentre_d(r, want):
    """Centre distance at which an obstacle of radius r, half a ray off a ray, reads `want` on it."""
    dl = 0.5 * O.SENSOR_RES
    lo, hi = r, r + 1.0
    for _ in range(200):
        d = 0.5 * (lo + hi)
        lo, hi = (d, hi) if d * np.cos(dl) - np.sqrt(r * r - (d * np.sin(dl)) ** 2) < want else (lo, d)
    return 0.5 * (lo + hi)


def _contact(m):
    sc = []
    r = 0.5
    for psi in (0.0, 2.4):
        for ray in (17.0, 100.0, 63.5):
            for thr, q in ((0.05, "key"), (0.2, "coll")):
                for sg in (-1, 1):
                    gap = thr + sg * m
                    d = r + gap if (q == "key" or ray == int(ray)) else _offcentre_d(r, gap)
                    ang = psi + O.SENSOR_START + ray * O.SENSOR_RES
                    sc.append(_S(x=POSE[0], y=POSE[1], psi=psi, obst=(POSE[0] + d * np.cos(ang), POSE[1] + d * np.sin(ang), r),
                                 q=q, side=sg, margin=0.5 * m,
                                 note=f"obstacle on ray {ray:g}, {'d - r' if q == 'key' else 'reading'} = {thr:g} {sg * m:+g}"))
    return sc, 0


_BUILDERS = {"clips": build_clips, "progress": build_progress, "angle": build_angle, "ye": build_ye,
             "bounds": build_bounds, "timelimit": lambda: _timelimit(3), "timelimit0": lambda: _timelimit(0),
             "heading": build_heading, "contact": lambda: _contact(2e-3), "contact64": lambda: _contact(1e-9)}
BATCHES = tuple(_BUILDERS)
F64_ONLY = ("contact64",)                            # 1e-9 m from the thresholds: below float32's resolution
WITH_OBSTACLES = ("contact", "contact64")
ENV_IDS = ("usv-simple", "usv-asmc-simple")


def batches(precision):
    return tuple(b for b in BATCHES if precision == "f64" or b not in F64_ONLY)


_FAR = (150.0 * np.cos(1.0), 150.0 * np.sin(1.0), 0.3)     # offset of the default obstacle: out of range


@functools.lru_cache(maxsize=None)
def batch(name):
    """The named batch as read-only arrays (one row per scene) plus `limit` and the labels."""
    scenes, limit = _BUILDERS[name]()
    n = len(scenes)
    col = lambda k: np.array([s[k] for s in scenes], dtype=np.float64)
    out = {k: col(k) for k in ("x", "y", "psi", "u", "r", "last_u", "last_r", "progress", "max_u", "max_r", "ref_v")}
    path = np.array([s["path"] for s in scenes], dtype=np.float64)
    for j, k in enumerate(("path_x0", "path_y0", "path_x1", "path_y1")):
        out[k] = path[:, j].copy()
    out["elapsed"] = np.array([s["elapsed"] for s in scenes], dtype=np.int32)
    out["asmc0"] = np.array([s["psi"] if s["asmc0"] is None else s["asmc0"] for s in scenes])
    ob = np.array([s["obst"] if s["obst"] else (s["x"] + _FAR[0], s["y"] + _FAR[1], _FAR[2]) for s in scenes])
    out["ox"], out["oy"], out["orad"] = ob[:, 0].copy(), ob[:, 1].copy(), ob[:, 2].copy()
    out["actions"] = np.array([s["actions"] for s in scenes], dtype=np.float32).reshape(n, T, 2)
    out["side"] = np.array([s["side"] for s in scenes], dtype=np.int64)
    out["step"] = np.array([s["step"] for s in scenes], dtype=np.int64)
    out["margin"] = col("margin")
    out["negzero"] = np.array([s["negzero"] for s in scenes], dtype=bool)
    for v in out.values():
        v.setflags(write=False)
    out.update(q=tuple(s["q"] for s in scenes), note=tuple(s["note"] for s in scenes), limit=limit, name=name)
    return out


INPUT_KEYS = ("x", "y", "psi", "u", "r", "last_u", "last_r", "progress", "max_u", "max_r", "ref_v", "path_x0",
              "path_y0", "path_x1", "path_y1", "elapsed", "asmc0", "ox", "oy", "orad", "actions")


def scene_state(sc, env_id, order=None):
    """The set_state dictionary (field names of SimpleEnvBatch.get_state) of the scenes, in `order` if given."""
    o = np.arange(len(sc["x"])) if order is None else np.asarray(order)
    n = len(o)
    st = {k: sc[k][o] for k in ("x", "y", "psi", "u", "r", "last_u", "last_r", "progress", "path_x0", "path_y0",
                                "path_x1", "path_y1", "max_u", "max_r", "ref_v")}
    st["v"] = np.zeros(n)
    st["n_obs"] = np.ones(n, np.int32)
    for k, f in (("obs_x", "ox"), ("obs_y", "oy"), ("obs_r", "orad")):
        a = np.zeros((n, CAP))
        a[:, 0] = sc[f][o]
        st[k] = a
    st["sensor_last"] = np.zeros((n, O.SENSOR_COUNT))
    st["elapsed"] = sc["elapsed"][o]
    st["scan_valid"] = 1
    asmc = np.zeros((n, O.ASMC_N))
    if env_id == "usv-asmc-simple":
        asmc[:, 0] = sc["asmc0"][o]
    st["asmc"] = asmc
    return st


def describe(name, i):
    """What scene i of a batch targets, in words (for failure messages)."""
    sc = batch(name)
    side = {-1: "below", 0: "on", 1: "above"}[int(sc["side"][i])]
    return (f"batch {name} env {i}: {sc['note'][i]}; deciding quantity {sc['q'][i]} {side} its threshold in step "
            f"{int(sc['step'][i])} (margin {sc['margin'][i]:.3g}); pose ({sc['x'][i]!r}, {sc['y'][i]!r}, {sc['psi'][i]!r}), "
            f"velocity ({sc['u'][i]!r}, {sc['r'][i]!r}), actions {sc['actions'][i].tolist()}")


# --------------------------------------------------------------------------- the oracle on the scenes
INFO_KEYS = ("action0", "action1", "ye", "angle_to_target", "ye_reward", "angle_to_target_reward", "delta_action_reward",
             "delta_action", "velocity_track_reward", "reference_velocity", "reward_velocity", "reference_velocity_error")
QUANTITIES = ("acc_u_lo", "acc_u_hi", "acc_r_lo", "acc_r_hi", "spd_u_lo", "spd_u_hi", "spd_r_lo", "spd_r_hi", "prog_lo",
              "prog_hi", "x_lo", "x_hi", "y_lo", "y_hi", "tl", "oct_dx", "oct_dy", "oct_diag", "cut", "dist", "ye_k", "ye",
              "rebase", "asmc_wrap", "key", "coll")


def info_rows(info):
    """The oracle's / reference's step info as [n, 22] rows in the library's column order."""
    cols = [info["position"][:, 0], info["position"][:, 1], info["position"][:, 2], info["velocity"][:, 0],
            info["velocity"][:, 1], info["velocity"][:, 2], info["path_start"][:, 0], info["path_start"][:, 1],
            info["path_end"][:, 0], info["path_end"][:, 1]] + [info[k] for k in INFO_KEYS]
    return np.stack([np.asarray(c, dtype=np.float64) for c in cols], axis=1)


def _oracle_env(sc, env_id):
    n = len(sc["x"])
    env = O.SimpleEnvBatch(n, CAP) if env_id == "usv-simple" else O.SimpleAsmcEnvBatch(n, CAP)
    z = np.zeros(n)
    env.position = np.stack([sc["x"], sc["y"], sc["psi"]], axis=1)
    env.velocity = np.stack([sc["u"], z, sc["r"]], axis=1)
    env.last_action = np.stack([sc["last_u"], z, sc["last_r"]], axis=1)
    env.max_action = np.stack([sc["max_u"], z, sc["max_r"]], axis=1)
    env.ref_v, env.progress = sc["ref_v"].copy(), sc["progress"].copy()
    env.path_start = np.stack([sc["path_x0"], sc["path_y0"]], axis=1)
    env.path_end = np.stack([sc["path_x1"], sc["path_y1"]], axis=1)
    env.n_obs[:] = 1
    env.ox[:, 0], env.oy[:, 0], env.orad[:, 0] = sc["ox"], sc["oy"], sc["orad"]
    if env_id != "usv-simple":
        env.asmc.state[:, 0] = sc["asmc0"]
    return env


@functools.lru_cache(maxsize=None)
def trace(name, env_id):
    """The float64 oracle stepped T times from the batch's states (computed once, read-only): its outputs
    per step (hdr [n, T, 15] float32, sensors [n, T, 128] float32, reward, terminated, truncated, info
    [n, T, 22], psi, psi_d_last) and every deciding quantity of the module docstring as [n, T]."""
    sc = batch(name)
    n, limit = len(sc["x"]), sc["limit"]
    env = _oracle_env(sc, env_id)
    out = {k: np.zeros((n, T)) for k in QUANTITIES + ("reward", "psi", "psi_d_last")}
    out.update(hdr=np.zeros((n, T, 15), F32), sensors=np.zeros((n, T, 128), F32), info=np.zeros((n, T, 22)),
               terminated=np.zeros((n, T), bool), truncated=np.zeros((n, T), bool))
    el = sc["elapsed"].astype(np.int64).copy()
    turns = np.rint(sc["psi"] / (2 * PI))            # the f32 frame's k
    for t in range(T):
        act = sc["actions"][:, t].astype(np.float64)
        out["asmc_wrap"][:, t] = np.abs(act[:, 1]) - PI
        if env_id != "usv-simple":
            for _ in range(2):
                env.position, env.velocity = env.asmc.compute(act, env.position, env.velocity)
            act = np.zeros((n, 2))
        a3 = 0.8 * env.last_action + 0.2 * (env.max_action * np.stack([act[:, 0], np.zeros(n), act[:, 1]], axis=1))
        dv = a3 - env.velocity
        sv = env.velocity + np.clip(dv, -O.MAX_ACC, O.MAX_ACC)
        for ch, j in (("u", 0), ("r", 2)):
            out[f"acc_{ch}_lo"][:, t], out[f"acc_{ch}_hi"][:, t] = dv[:, j] + O.MAX_ACC[j], dv[:, j] - O.MAX_ACC[j]
            out[f"spd_{ch}_lo"][:, t], out[f"spd_{ch}_hi"][:, t] = sv[:, j] + env.max_action[:, j], sv[:, j] - env.max_action[:, j]
        a3k = env.kinematics(act)
        assert np.array_equal(a3k, a3)
        p, d = env.position, env.path_end - env.path_start
        a_raw = (d[:, 1] * (p[:, 1] - env.path_start[:, 1]) + d[:, 0] * (p[:, 0] - env.path_start[:, 0])) / (d ** 2).sum(1) + O.LOOKAHEAD
        out["prog_lo"][:, t], out["prog_hi"][:, t] = a_raw - env.progress, a_raw - 1.0
        obs, rew, term, trunc = env._finish_step(a3)
        el += 1
        out["tl"][:, t] = el - limit if limit else -1.0
        if limit:
            trunc = trunc | (el >= limit)
        out["x_lo"][:, t], out["x_hi"][:, t] = p[:, 0], p[:, 0] - O.BOUND_HI
        out["y_lo"][:, t], out["y_hi"][:, t] = p[:, 1], p[:, 1] - O.BOUND_HI
        tg = env.target - p[:, :2]
        out["oct_dx"][:, t], out["oct_dy"][:, t] = tg[:, 0], tg[:, 1]
        out["oct_diag"][:, t] = np.abs(tg[:, 1]) - np.abs(tg[:, 0])
        out["cut"][:, t] = np.abs(np.arctan2(tg[:, 1], tg[:, 0]) - p[:, 2]) - PI
        out["dist"][:, t] = np.hypot(tg[:, 0], tg[:, 1]) - 2e-3
        ye = env.ye()
        out["ye"][:, t], out["ye_k"][:, t] = ye, np.abs(ye) - YE_K
        nt = np.rint((p[:, 2] - 2 * PI * turns) / (2 * PI))
        out["rebase"][:, t] = nt
        turns = turns + nt
        keys = np.hypot(env.ox[:, 0] - p[:, 0], env.oy[:, 0] - p[:, 1]) - env.orad[:, 0]
        out["key"][:, t], out["coll"][:, t] = keys - 0.05, env.sensors.min(axis=1) - 0.2
        out["hdr"][:, t], out["sensors"][:, t] = obs[:, :15], obs[:, 15:]
        out["reward"][:, t], out["terminated"][:, t], out["truncated"][:, t] = rew, term, trunc
        out["info"][:, t] = info_rows(env.info)
        out["psi"][:, t] = p[:, 2]
        if env_id != "usv-simple":
            out["psi_d_last"][:, t] = env.asmc.state[:, 0]
    for v in out.values():
        v.setflags(write=False)
    return out
