"""Deterministic edge states for the lane-per-env legacy step kernels (plain numpy, no GPU):
usv-asmc-v0 (v0_step_kernel), usv-asmc-ye-int-v0 and usv-pid-v0 (legacy_step_kernel, csrc/usv_legacy.hpp).

One env is one scene: an injected state (x, y, psi, u, v, r, last[9], aux[3], target[6], a_last, elapsed and,
for the two float64 ids, ye2 = (ye_int, ye_last)) next to one branch of the step, and its actions for T = 3
steps.  A usv-asmc-v0 batch that holds a scene with elapsed = 0 takes a fourth step, so the step on the
float64 reset state and the steps on the stored float32 state are both in it.  usv-asmc-v0's state is rounded
to float32 where elapsed != 0, as the reference's own step stores it (`target` stays float64 there, with a
float32-representable path angle ak, as the reference's reset makes it); the two float64 ids keep float64.

Every scene is labelled with the deciding quantity it sits next to (`q`, a row of trace()), the side it must
fall on (`side`: the sign of the quantity, 0 = exactly on the threshold), the step (`step`, from 1) and the
distance it keeps (`margin`).  Quantities are value minus threshold, evaluated as the reference does:

  drag                   |u| - 1.2 before the step (usv-asmc-v0 on float32 state: against float32(1.2))
  ka_u, ka_psi           Ka - kmin (usv-asmc-v0 on float32 state: against float32(kmin))
  sig_u, sig_psi         |sigma| - mu, the argument of np.sign in Ka_dot; sigma_u, sigma_psi: sigma itself
  tport_hi / tport_lo    unclipped port thrust - 36.5 / + 30; tstbd_hi / tstbd_lo likewise
  wrap_d, wrap_e         |a + ak| - pi, |psi_d - psi| - pi
  wrap_psi, wrap_ak      |integrated psi| - pi, |psi - ak| - pi
  rew_ak, ye1            |psi_ak| - pi/2, |ye| - 1 (the reward's arms)
  ye10                   |ye| - 10;  x_hi, x_lo: x - 30, x + 30 (usv-asmc-v0);  x_min: x + 10 (the other two)
  ye, ye_last            the cross-track error and the stored one it is compared with (ye_int restart)
  adot                   |action - action_last| / h
  tl                     elapsed - limit after the step (truncated when >= 0 and not terminated)
  first                  +1: the step runs on the float64 reset state, -1: on the stored float32 state

Families (`BATCHES`): drag, gains, pid, thrust, wrap, path, reward, ye_int, bounds, bounds64 (the bounds scenes
1e-9 from their thresholds, f64 build only), timelimit (limit 3), timelimit0 (the same scenes, no limit), first
and exact64 (|sigma_psi| = mu_psi exactly, f64 build only).  batch(name, env_id) is empty where a family does not apply to an id.

Measured on an MI355X (tests/test_gpu_legacy_edges.py): f64 usv-asmc-ye-int-v0 and usv-pid-v0 obs bit-equal to the
reference on every scene step, reward 3.3e-16; usv-asmc-v0 obs bit-equal on every scene step too, reward 1.1e-10;
f32 obs 9.5e-7, reward 1.6e-6; flags exact throughout.

ye_int holds the computed ye as +0.0 and as -0.0 (ak in the second quadrant with the boat held on (x0, y0) = (2^50, 2^50),
where a step's motion is below half an ulp in float32 and float64 alike), each against a stored +0.0, and +0.0 against -0.0.
x cannot be held still on |x| = 30 or x = -10 (the surge controller always accelerates), so the strict
inequalities are taken exactly on the threshold for |ye| = 10 only.
"""
import functools

import numpy as np

from oracle import usv_oracle as O

T = 3
PI = np.pi
F32 = np.float32
ENV_IDS = ("usv-asmc-v0", "usv-asmc-ye-int-v0", "usv-pid-v0")
SHORT = {"usv-asmc-v0": "v0", "usv-asmc-ye-int-v0": "yeint", "usv-pid-v0": "pid"}
V0, YEINT, PID = ENV_IDS
MARGIN = 1e-3                                        # metres / radians kept from a threshold
OFF = 2e-3                                           # where the scenes are put: twice the margin
AKS = tuple(float(F32(v)) for v in (0.7, 2.4, -2.4, -0.7))          # one path angle per quadrant


def f32r(v):
    return np.asarray(v, dtype=np.float64).astype(F32).astype(np.float64)


A0, A1, A2 = (float(F32(v)) for v in (0.05, 0.06, 0.04))   # actions are float32

_DEF = dict(x=2.0, y=0.3, psi=0.1, u=0.8, v=0.02, r=0.01,
            last=(0.8, 0.08, 0.01, 0.05, 0.0, 0.0, 0.0, 0.05, 0.2), aux=(0.02, 0.03, 0.1),
            target=(0.0, 0.0, 1.4, 0.0, 20.0, 0.0), a_last=A0, elapsed=1, ye2=(0.0, 0.0),
            actions=(A0, A1, A2), q="", side=0, step=1, margin=0.0, note="", flip=None, pair=None, negzero=False)


def _S(**kw):
    s = dict(_DEF)
    bad = set(kw) - set(s)
    assert not bad, bad
    s.update(kw)
    return s


def _target(ak=0.0, x0=0.0, y0=0.0, ds=1.4):
    return (x0, y0, ds, ak, x0 + 20.0 * np.cos(ak), y0 + 20.0 * np.sin(ak))


def _arrays(scenes, env_id):
    """The scenes of one id as arrays; usv-asmc-v0's state float32-rounded where elapsed != 0."""
    n = len(scenes)
    col = lambda k, w=None: np.array([s[k] for s in scenes], dtype=np.float64).reshape((n,) if w is None else (n, w))
    out = {k: col(k) for k in ("x", "y", "psi", "u", "v", "r", "a_last")}
    out.update(last=col("last", 9), aux=col("aux", 3), target=col("target", 6), ye2=col("ye2", 2))
    out["elapsed"] = np.array([s["elapsed"] for s in scenes], dtype=np.int32).reshape(n)
    if env_id == V0:
        st = out["elapsed"] != 0
        for k in ("x", "y", "psi", "u", "v", "r", "a_last", "last", "aux"):
            out[k][st] = f32r(out[k][st])
        out["ye2"][:] = 0.0
    elif env_id == PID:
        out["ye2"][:] = 0.0
    return out


def _oracle_env(sc, env_id):
    n = len(sc["x"])
    env = O.AsmcV0Batch(n) if env_id == V0 else O.LegacyF64Batch(n, "ye_int" if env_id == YEINT else "pid")
    env.position = np.stack([sc["x"], sc["y"], sc["psi"]], axis=1)
    env.velocity = np.stack([sc["u"], sc["v"], sc["r"]], axis=1)
    env.target = sc["target"].copy()
    env.state = np.zeros((n, 6))
    env.state[:, 5] = sc["a_last"]
    if env_id == V0:
        env.aux, env.last = sc["aux"].copy(), sc["last"].copy()
        env.first = sc["elapsed"] == 0
    else:
        env.aux = np.concatenate([sc["aux"], sc["ye2"][:, :1]], axis=1)
        env.last = np.concatenate([sc["last"], sc["ye2"][:, 1:]], axis=1)
    return env


def _probe(s, env_id, q, steps=1):
    """Quantity q in step `steps` of one scene (the oracle on a batch of one)."""
    sc = _arrays([s], env_id)
    env = _oracle_env(sc, env_id)
    for t in range(steps):
        env.step(np.array([s["actions"][min(t, len(s["actions"]) - 1)]], dtype=F32))
    return float(env.q[q][0])


def _solve(env_id, s, key, q, want, lo, hi, sub=None):
    """The scene with s[key] (or entry `sub` of it) moved within [lo, hi] until quantity q is `want` in step 1;
    q must be monotone there.  A usv-asmc-v0 state value is solved on float32 values (it is stored as one)."""
    def put(v):
        t = dict(s)
        if key == "actions":
            t[key] = (float(F32(v)),) + tuple(s[key][1:])
        elif sub is None:
            t[key] = float(f32r(v)) if (env_id == V0 and s["elapsed"] != 0) else v
        else:
            w = list(s[key])
            w[sub] = float(f32r(v)) if (env_id == V0 and s["elapsed"] != 0 and key != "target") else v
            t[key] = tuple(w)
        return t
    flo, fhi = _probe(put(lo), env_id, q) - want, _probe(put(hi), env_id, q) - want
    assert flo * fhi < 0, (env_id, key, q, want, flo, fhi)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        fm = _probe(put(mid), env_id, q) - want
        lo, hi, flo = (mid, hi, fm) if fm * flo > 0 else (lo, mid, flo)
    return put(0.5 * (lo + hi))


# --------------------------------------------------------------------------- families
# Both thrusters saturated (e_psi near 3 rad): the surge controller cannot cancel the drag it computes
_SAT = dict(psi=-1.4, actions=(1.5, 1.5, 1.5), a_last=1.5)


def build_drag(env_id):
    sc = []
    for sg in (1.0, -1.0):
        for d, side in ((-OFF, -1), (OFF, 1), (0.0, 0)):
            sc.append(_S(u=sg * (1.2 + d), q="drag", side=side, margin=MARGIN if d else 0.0, flip="drag" if d else None,
                         note=f"u = {sg:+g} * (1.2 {d:+g}), thrust saturated", **_SAT))
        sc.append(_S(u=sg * (1.2 - 20 * OFF), q="drag", side=-1, margin=MARGIN, flip="drag",
                     note=f"u = {sg:+g} * 1.16, thrust free"))
    sc.append(_S(u=1.2 + 1.5 * OFF, q="drag", side=-1, step=3, margin=MARGIN,
                 note="u decays through 1.2 between steps 1 and 3", **_SAT))
    return sc, 0


def build_gains(env_id):
    if env_id == PID:
        return [], 0
    sc = []
    for j, (kmin, name) in enumerate(((O.KMIN_U, "ka_u"), (O.KMIN_PSI, "ka_psi"))):
        for d, side in ((-MARGIN, -1), (MARGIN, 1), (0.0, 0)):
            aux = list(_DEF["aux"])
            aux[1 + j] = kmin + d
            # u 0.3 below u_d: |sigma_u| > mu_u; e_psi = 0.3: |sigma_psi| > mu_psi (sign +1: K_dot differs from kmin's arm
            # for ka_u; for ka_psi the arm above kmin is told apart where sign is -1: e_psi small)
            kw = dict(psi=0.04) if name == "ka_psi" else {}
            sc.append(_S(aux=tuple(aux), q=name, side=side, margin=0.9 * abs(d), flip=name if d else None,
                         note=f"{name} = kmin {d:+g}", **kw))
    above = (0.02, 0.08, 0.3)                          # both gains above their minimum
    for sg in (1.0, -1.0):
        for d, side in ((-OFF, -1), (OFF, 1)):
            s = _S(aux=above, q="sig_u", side=side, margin=MARGIN, flip="sig_u", note=f"sigma_u = {sg:+g} * (mu_u {d:+g})")
            s = _solve(env_id, s, "u", "sigma_u", sg * (O.MU_U + d), 0.2, 2.0)
            sc.append(s)
            s = _S(aux=above, q="sig_psi", side=side, margin=MARGIN, flip="sig_psi", note=f"sigma_psi = {sg:+g} * (mu_psi {d:+g})")
            s = _solve(env_id, s, "r", "sigma_psi", sg * (O.MU_PSI + d), -1.0, 1.0)
            sc.append(s)
    a = float(F32(0.25))
    sc.append(_S(aux=above, psi=a, r=0.0, actions=(a, a, a), a_last=a, q="sigma_psi", side=0,
                 note="sigma_psi = 0: e_psi = 0 and r = 0, sign(0) * sqrt(0)"))
    return sc, 0


def build_exact64(env_id):
    """|sigma_psi| - mu_psi = 0 exactly: 0.125 - 0.1 and 0.125 - (0.125 - 0.1) are exact in float64 (not in float32: f64
    build only, and a first step on usv-asmc-v0), and r = 0: np.sign(0) = 0, so Ka_dot_psi = 0."""
    if env_id == PID:
        return [], 0
    return [_S(aux=(0.02, 0.08, 0.3), psi=0.125 - 0.1, r=0.0, actions=(0.125, 0.125, 0.125), a_last=0.125,
               elapsed=0 if env_id == V0 else 1, q="sig_psi", side=0, note="|sigma_psi| = mu_psi exactly: sign(0) = 0")], 0


def build_pid(env_id):
    if env_id != PID:
        return [], 0
    sc = []
    for e_u_last in (0.3, -0.3, 1e-3):
        for e_u_int in (0.0, 0.5, -2.0):
            last = list(_DEF["last"])
            last[6] = e_u_last
            sc.append(_S(last=tuple(last), aux=(e_u_int, 0.0, 0.0), q="drag", side=-1, margin=0.3,
                         note=f"stale e_u_last = {e_u_last:g}, integrator {e_u_int:g}"))
    return sc, 0


def build_thrust(env_id):
    sc = []
    # e_psi (through psi) moves Tz: port and starboard thrust go opposite ways; far scenes sit 20 N either side of a clip
    a = float(F32(0.2))
    base = dict(actions=(a, a, a), a_last=a)
    pid = env_id == PID                              # its surge law's derivative term rules Tx: tuned through the desired speed
    for q, sgn in (("tport_hi", 1), ("tport_lo", -1), ("tstbd_hi", 1), ("tstbd_lo", -1)):
        for d in (-20.0, -0.05, 0.05, 20.0):
            s = _S(q=q, side=int(np.sign(d) * sgn), margin=0.04, flip=q if abs(d) == 20.0 else None,
                   note=f"{q.split('_')[0]} raw = {'36.5' if sgn > 0 else '-30'} {sgn * d:+g} N", **base)
            sc.append(_solve(env_id, s, "target", q, sgn * d, -3.0, 5.0, sub=2) if pid else _solve(env_id, s, "psi", q, sgn * d, 0.2 - 3.1, 0.2 + 3.1))
    lo = _S(psi=-2.9, q="tstbd_lo", side=-1, margin=1.0, note="both saturated: port high, starboard low", **base)
    hi = _S(psi=3.1, q="tstbd_hi", side=1, margin=1.0, note="both saturated: port low, starboard high", **base)
    sc += [_solve(env_id, lo, "u", "tport_hi", 5.0, -1.1, 1.19), _solve(env_id, hi, "u", "tstbd_hi", 5.0, -1.1, 1.19)] if pid else [lo, hi]
    return sc, 0


def build_wrap(env_id):
    sc = []
    for ak in (0.0,) + AKS:
        tg = _target(ak, 0.5, -0.25)
        # ak = 0: both cuts; a quadrant's ak: the cut that psi - ak can pass with the heading within [-pi, pi]
        for sg in ((1.0, -1.0) if ak == 0.0 else (-np.sign(ak),)):
            for d in (-OFF, OFF):
                side = int(np.sign(d))
                lab = dict(side=side, margin=MARGIN, target=tg)
                # psi_d = a + ak; the boat heads along psi_d so the other sites stay clear where they can
                a = float(F32(sg * (PI + d) - ak))
                pd = O.wrap_once(np.float64(a + ak))
                sc.append(_S(psi=float(pd) * 0.9, actions=(a, a, a), a_last=a, q="wrap_d", note=f"a + ak = {sg:+g} (pi {d:+g}), ak = {ak:g}", **lab))
                # e_psi = psi_d - psi with psi_d = sg * 1
                a = float(F32(sg * 1.0 - ak))
                sc.append(_S(psi=float(np.float64(a) + ak - sg * (PI + d)), actions=(a, a, a), a_last=a, q="wrap_e",
                             note=f"psi_d - psi = {sg:+g} (pi {d:+g}), ak = {ak:g}", **lab))
                # the integrated heading: turning at 0.5 rad/s towards the cut
                last = list(_DEF["last"])
                last[2] = sg * 0.5
                a = float(F32(O.wrap_once(np.float64(sg * PI - ak))))
                s = _S(r=sg * 0.5, last=tuple(last), actions=(a, a, a), a_last=a, q="wrap_psi", note=f"psi integrates to {sg:+g} (pi {d:+g}), ak = {ak:g}", **lab)
                sc.append(_solve(env_id, s, "psi", "wrap_psi", d, sg * (PI - 0.05), sg * (PI + 0.05)))
                # psi - ak: beyond only where the heading can stay within [-pi, pi]
                if d < 0 or (ak != 0.0 and np.sign(ak) == -sg):
                    want = ak + sg * (PI + d)
                    if abs(want) < PI:
                        a = float(F32(O.wrap_once(np.float64(want - ak))))
                        s = _S(r=0.0, actions=(a, a, a), a_last=a, q="wrap_ak", note=f"psi - ak = {sg:+g} (pi {d:+g}), ak = {ak:g}", **lab)
                        out = 0.05 if abs(want) < PI - 0.05 else 0.5 * OFF      # ak = 0: the heading itself stays short of the cut
                        sc.append(_solve(env_id, s, "psi", "wrap_ak", d, want - sg * 0.05, want + sg * out))
    f = float(F32(PI))
    for a in (f, -f):
        sc.append(_S(psi=2.5 * np.sign(a), actions=(a, a, a), a_last=a, q="wrap_d", side=1, margin=8e-8,
                     note=f"a = {a!r}: float32(pi) > pi wraps"))
    return sc, 0


def build_path(env_id):
    sc = []
    h = float(F32(PI / 2))
    for ak in (0.0, -0.0) + AKS + (h, -h):
        for lat in (0.0, 1.5, -1.5):
            x0, y0 = 0.7, -0.4
            c, s = np.cos(ak), np.sin(ak)
            x, y = x0 + 3.0 * c - lat * s, y0 + 3.0 * s + lat * c
            a = float(F32(0.1))
            sc.append(_S(x=x, y=y, psi=float(O.wrap_once(np.float64(ak + 0.1))), target=_target(ak, x0, y0), actions=(a, a, a), a_last=a,
                         q="ye" if lat else "ye1", side=int(np.sign(lat)) if lat else -1, margin=1.4 if lat else 0.9,
                         note=f"ak = {ak!r}, {'on' if not lat else ('left of' if lat > 0 else 'right of')} the path"))
    return sc, 0


def build_reward(env_id):
    sc = []
    for ak in (0.0, AKS[1]):
        for sg in (1.0, -1.0):
            for d in (-OFF, OFF):
                a = float(F32(sg * PI / 2))
                s = _S(target=_target(ak, 0.5, -0.25), r=0.0, actions=(a, a, a), a_last=a, q="rew_ak", side=int(np.sign(d)), margin=MARGIN,
                       flip="rew_ak", note=f"psi_ak = {sg:+g} (pi/2 {d:+g}), ak = {ak:g}")
                c = float(O.wrap_once(np.float64(ak + sg * PI / 2)))
                if abs(c) > PI - 0.1:
                    continue
                sc.append(_solve(env_id, s, "psi", "rew_ak", d, c - 0.05, c + 0.05))
    for sg in (1.0, -1.0):
        for d in (-OFF, OFF):
            s = _S(y=sg * (1.0 + d), psi=0.0, v=0.0, q="ye1", side=int(np.sign(d)), margin=MARGIN, note=f"ye = {sg:+g} (1 {d:+g})")
            sc.append(_solve(env_id, s, "y", "ye1", d, sg * 0.9, sg * 1.1))
    for da, side, m in ((0.0, 0, 0.0), (1e-3, 1, 0.09), (3.0, 1, 250.0), (-3.0, 1, 250.0)):
        a = float(F32(A0 + da))
        sc.append(_S(a_last=A0, actions=(a, float(F32(a + da / 2)), a), q="adot", side=side, margin=m, note=f"action - action_last = {da:g}"))
    return sc, 0


# Held still sideways: ak = 0, psi = 0, v = r = 0, a = 0 (e_psi = 0, so Tz = 0) and u = u_d (no surge error: neither
# thruster saturates, so port and starboard balance to a rounding residue).  The boat runs along the path, ye = y - y0,
# and where |y| >= 1 the residue's sideways motion is absorbed: ye keeps its bits over the T steps.
DS_STILL = 0.9
U_STILL = (DS_STILL - O.V0_MIN_SPEED) * (1 / (1 + np.exp(10 * (0.0 - 0.5)))) + O.V0_MIN_SPEED
_STILL = dict(psi=0.0, u=U_STILL, v=0.0, r=0.0, last=(U_STILL, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.05, 0.2),
              actions=(0.0, 0.0, 0.0), a_last=0.0)


def build_ye_int(env_id):
    if env_id != YEINT:
        return [], 0
    sc = []
    still = _STILL                                   # with y = y0 = 1, ye is +0.0 exactly
    for ye in (-0.4, 0.0, 0.4):
        for ye_last in (-0.4, 0.0, 0.4):
            for ye_int in (60.0, -60.0):
                pair = (int(np.sign(ye)), int(np.sign(ye_last)))
                sc.append(_S(y=1.0 + ye, target=_target(0.0, 0.0, 1.0, DS_STILL), ye2=(ye_int, ye_last), q="ye", side=pair[0],
                             margin=0.3 if ye else 0.0, pair=pair, flip="ye_restart",
                             note=f"sign(ye) {pair[0]:+d} against sign(ye_last) {pair[1]:+d}, ye_int = {ye_int:g}", **still))
    sc.append(_S(y=1.0, target=_target(0.0, 0.0, 1.0, DS_STILL), ye2=(60.0, -0.0), q="ye", side=0, pair=(0, 0), flip="ye_restart",
                 note="ye = +0.0 against ye_last = -0.0: equal signs, no restart", **still))
    # ye = -0.0 out of the step: with ak in the second quadrant, -(x - x0) sin ak is -0.0 and (y - y0) cos ak is -0.0
    # when the step leaves x == x0 and y == y0.  At x = y = 2^50 (exact in float32 too) a step's motion is below half an
    # ulp in either precision, so the position keeps its bits under every build
    big = 2.0 ** 50
    for ye_int in (60.0, -60.0):
        sc.append(_S(x=big, y=big, psi=float(O.wrap_once(np.float64(AKS[1] + 0.1))), target=_target(AKS[1], big, big), ye2=(ye_int, 0.0),
                     q="ye", side=0, pair=(0, 0), flip="ye_restart", negzero=True,
                     note=f"ye = -0.0 against ye_last = +0.0: equal signs, no restart, ye_int = {ye_int:g}"))
    return sc, 0


def _bounds(env_id, m, elapsed):
    sc = []
    still = dict(_STILL, target=_target(0.0, 0.0, 0.0, DS_STILL), elapsed=elapsed)
    for sg in (1.0, -1.0):
        for d in (-m, m):
            # ye = y - y0 with ak = 0: tuned through y0, which is float64 under every id
            s = _S(y=sg * 10.0, q="ye10", side=int(np.sign(d)), margin=m / 2, note=f"ye = {sg:+g} (10 {d:+g})", **still)
            sc.append(_solve(env_id, s, "target", "ye10", d, -0.5, 0.5, sub=1))
        sc.append(_S(y=sg * 10.0, q="ye10", side=0, note=f"ye = {sg:+g} exactly: not beyond", **still))
    mv = dict(elapsed=elapsed)
    if env_id == V0:
        for sg, q in ((1.0, "x_hi"), (-1.0, "x_lo")):
            for d in (-m, m):
                s = _S(x=sg * 30.0, psi=0.1 if sg > 0 else 3.0, q=q, side=int(np.sign(d) * sg), margin=m / 2,
                       note=f"x = {sg:+g} (30 {d:+g}) after the step", **mv)
                if m < 1e-6 and elapsed:
                    continue                         # a float32 x cannot be placed 1e-9 from 30
                sc.append(_solve(env_id, s, "x", q, sg * d, sg * 30.0 - 0.5, sg * 30.0 + 0.5))
        sc.append(_S(x=-15.0, q="x_lo", side=1, margin=10.0, note="x = -15: beyond the other ids' x < -10, inside |x| <= 30", **mv))
        sc.append(_S(x=35.0, q="x_hi", side=1, margin=4.0, note="x = +35: beyond |x| <= 30", **mv))
    else:
        for d in (-m, m):
            s = _S(x=-10.0, psi=3.0 if d < 0 else 0.1, q="x_min", side=int(np.sign(d)), margin=m / 2,
                   note=f"x = -10 {d:+g} after the step", **mv)
            sc.append(_solve(env_id, s, "x", "x_min", d, -10.5, -9.5))
        sc.append(_S(x=-15.0, q="x_min", side=-1, margin=4.0, note="x = -15: beyond x >= -10", **mv))
        sc.append(_S(x=35.0, q="x_min", side=1, margin=40.0, note="x = +35: beyond usv-asmc-v0's |x| <= 30, inside x >= -10", **mv))
    return sc, 0


def _timelimit(env_id, limit):
    sc = []
    for y, what in ((0.3, "no termination"), (12.0, "terminates in every step")):
        for el, step in ((2, 1), (1, 2)):
            sc.append(_S(y=y, elapsed=el, q="tl", side=0 if limit else -1, step=step,
                         note=f"elapsed {el}, limit {limit}: the count reaches 3 in step {step}; {what}"))
    # |ye| passes 10 in step 2, the step on which the count reaches the limit: terminated, not truncated
    sc.append(_S(y=10.0 - 1.2e-2, psi=PI / 2, u=1.0, last=(0.0, 1.0, 0.01, 0.05, 0.0, 0.0, 0.0, 0.05, 0.2), elapsed=1, q="tl",
                 side=0 if limit else -1, step=2, actions=(float(F32(PI / 2)),) * 3, a_last=float(F32(PI / 2)),
                 note="|ye| passes 10 in step 2, when the count reaches 3"))
    return sc, limit


def build_first(env_id):
    if env_id != V0:
        return [], 0
    sc = []
    third = 1.0 / 3.0
    states = [dict(), dict(u=1.25 + third * 1e-3, v=-0.07 * third, r=0.11 * third, psi=2.0 + third),
              dict(target=_target(AKS[0], 0.3, 0.2), psi=0.9 * third, x=3.0 * third, y=-1.0 * third),
              dict(target=_target(AKS[2], -0.3, 0.2), psi=-2.0 - third, u=0.3 * third, r=-0.2 * third, aux=(0.1 * third, 0.07 * third * 3.1, 0.31 * third * 3.1)),
              dict(a_last=0.9 * third, actions=(float(F32(-0.4)), float(F32(0.7)), float(F32(0.1)))),
              dict(u=-1.21 - third * 1e-3, psi=-0.5 * third, last=tuple(v * (1 + third * 1e-3) for v in _DEF["last"]))]
    for k, st in enumerate(states):
        base = {key: (tuple(np.asarray(v) * (1 + 1e-9)) if isinstance(v, tuple) else v * (1 + 1e-9))
                for key, v in {**{f: _DEF[f] for f in ("x", "y", "psi", "u", "v", "r", "last", "aux", "a_last")}, **st}.items()
                if key not in ("target", "actions")}
        rest = {key: v for key, v in st.items() if key in ("target", "actions")}
        sc.append(_S(elapsed=0, q="first", side=1, margin=1.0, note=f"state {k} as float64 after a reset", **base, **rest))
        sc.append(_S(elapsed=1, q="first", side=-1, margin=1.0, note=f"state {k} rounded to float32, elapsed 1", **base, **rest))
    return sc, 0


_BUILDERS = {"drag": build_drag, "gains": build_gains, "pid": build_pid, "thrust": build_thrust, "wrap": build_wrap,
             "path": build_path, "reward": build_reward, "ye_int": build_ye_int,
             "bounds": lambda e: _bounds(e, OFF, 1), "bounds64": lambda e: _bounds(e, 1e-9, 0 if e == V0 else 1),
             "timelimit": lambda e: _timelimit(e, 3), "timelimit0": lambda e: _timelimit(e, 0), "first": build_first,
             "exact64": build_exact64}
BATCHES = tuple(_BUILDERS)
F64_ONLY = ("bounds64", "exact64")                   # 1e-9 from, or exactly on, a threshold float32 cannot hold
INPUT_KEYS = ("x", "y", "psi", "u", "v", "r", "last", "aux", "target", "a_last", "ye2", "elapsed", "actions")
STATE_KEYS = ("position", "velocity", "aux", "last")
QUANTITIES = ("drag", "ka_u", "ka_psi", "sig_u", "sig_psi", "sigma_u", "sigma_psi", "tport_hi", "tport_lo", "tstbd_hi",
              "tstbd_lo", "wrap_d", "wrap_e", "wrap_psi", "wrap_ak", "rew_ak", "ye1", "ye10", "x_hi", "x_lo", "x_min", "ye",
              "ye_last", "adot", "tl", "first")


SMAX = T + 1
OUTPUT_KEYS = ("obs", "reward", "terminated", "truncated") + STATE_KEYS


def fixture(g, name, env_id):
    """Batch `name` of one id cut out of the loaded tests/golden/legacy_scenes.npz: its inputs (`in_<key>`), `limit`, and the
    reference's outputs per step ([n, steps, ...])."""
    pre = SHORT[env_id] + "__"
    j = BATCHES.index(name)
    count = g[pre + "count"]
    rows = slice(int(count[:j].sum()), int(count[:j + 1].sum()))
    steps = int(g[pre + "steps"][j])
    out = {"in_" + k: g[pre + k][rows] for k in INPUT_KEYS}
    out["in_actions"] = out["in_actions"][:, :steps]
    out.update({k: g[pre + "out_" + k][rows, :steps] for k in OUTPUT_KEYS})
    for k, w in (("aux", 4), ("last", 10)):          # stored at the id's own width (and as float32 for usv-asmc-v0)
        a = out[k].astype(np.float64)
        out[k] = np.concatenate([a, np.zeros(a.shape[:2] + (w - a.shape[2],))], axis=2)
    out["position"], out["velocity"] = out["position"].astype(np.float64), out["velocity"].astype(np.float64)
    out.update(limit=int(g[pre + "limit"][j]), steps=steps)
    return out


def batches(precision, env_id):
    return tuple(b for b in BATCHES if (precision == "f64" or b not in F64_ONLY) and len(batch(b, env_id)["x"]))


@functools.lru_cache(maxsize=None)
def batch(name, env_id):
    """The named batch of one id as read-only arrays (one row per scene) plus `limit`, `steps` and the labels."""
    scenes, limit = _BUILDERS[name](env_id)
    n = len(scenes)
    out = _arrays(scenes, env_id)
    steps = T + 1 if (env_id == V0 and n and (out["elapsed"] == 0).any()) else T
    acts = np.zeros((n, steps), F32)
    for i, s in enumerate(scenes):
        a = tuple(s["actions"])
        acts[i] = (a + (a[0],) * steps)[:steps]
    out["actions"] = acts
    out["side"] = np.array([s["side"] for s in scenes], dtype=np.int64).reshape(n)
    out["step"] = np.array([s["step"] for s in scenes], dtype=np.int64).reshape(n)
    out["margin"] = np.array([s["margin"] for s in scenes], dtype=np.float64).reshape(n)
    out["negzero"] = np.array([s["negzero"] for s in scenes], dtype=bool).reshape(n)
    for v in out.values():
        v.setflags(write=False)
    out.update(q=tuple(s["q"] for s in scenes), note=tuple(s["note"] for s in scenes), flip=tuple(s["flip"] for s in scenes),
               pair=tuple(s["pair"] for s in scenes), limit=limit, steps=steps, name=name, env_id=env_id)
    return out


def scene_state(sc, env_id, order=None):
    """The set_state dictionary (field names of get_state) of the scenes, in `order` if given."""
    o = np.arange(len(sc["x"])) if order is None else np.asarray(order)
    st = {k: sc[k][o] for k in ("x", "y", "psi", "u", "v", "r")}
    st.update(v0_last=sc["last"][o], v0_aux=sc["aux"][o], v0_target=sc["target"][o], v0_action_last=sc["a_last"][o],
              elapsed=sc["elapsed"][o], v0_ye=sc["ye2"][o])       # ye_int, ye_last: zero but for usv-asmc-ye-int-v0
    return st


def describe(name, env_id, i):
    """What scene i of a batch targets, in words (for failure messages)."""
    sc = batch(name, env_id)
    side = {-1: "below", 0: "on", 1: "above"}[int(sc["side"][i])]
    return (f"{env_id} batch {name} env {i}: {sc['note'][i]}; deciding quantity {sc['q'][i]} {side} its threshold in step "
            f"{int(sc['step'][i])} (margin {sc['margin'][i]:.3g}); pose ({sc['x'][i]!r}, {sc['y'][i]!r}, {sc['psi'][i]!r}), "
            f"velocity ({sc['u'][i]!r}, {sc['v'][i]!r}, {sc['r'][i]!r}), aux {sc['aux'][i].tolist()}, ak {sc['target'][i, 3]!r}, "
            f"elapsed {int(sc['elapsed'][i])}, actions {sc['actions'][i].tolist()}")


# --------------------------------------------------------------------------- the oracle on the scenes
def run_oracle(name, env_id, flip=None):
    """The float64 oracle stepped through the batch: obs [n, S, 6] float32, reward, terminated, truncated, the
    post-step state (position [n, S, 3], velocity, aux [n, S, 4], last [n, S, 10]; the float64 ids' ye_int and
    ye_last are aux[3] and last[9], zero for usv-asmc-v0), elapsed and every deciding quantity as [n, S].
    `flip`: {comparison: [n] bool}, comparisons forced the other way in every step."""
    sc = batch(name, env_id)
    n, limit, S = len(sc["x"]), sc["limit"], sc["steps"]
    env = _oracle_env(sc, env_id)
    env.flip = dict(flip or {})
    out = {k: np.full((n, S), np.nan) for k in QUANTITIES + ("reward",)}
    out.update(obs=np.zeros((n, S, 6), F32), terminated=np.zeros((n, S), bool), truncated=np.zeros((n, S), bool),
               position=np.zeros((n, S, 3)), velocity=np.zeros((n, S, 3)), aux=np.zeros((n, S, 4)), last=np.zeros((n, S, 10)),
               elapsed=np.zeros((n, S), np.int64))
    el = sc["elapsed"].astype(np.int64).copy()
    for t in range(S if n else 0):
        obs, rew, done = env.step(sc["actions"][:, t])
        el += 1
        for k, v in env.q.items():
            out[k][:, t] = v
        out["tl"][:, t] = el - limit if limit else -1.0
        out["obs"][:, t], out["reward"][:, t], out["terminated"][:, t] = obs, rew, done
        out["truncated"][:, t] = ~done & (el >= limit) if limit else False
        out["position"][:, t], out["velocity"][:, t], out["elapsed"][:, t] = env.position, env.velocity, el
        out["aux"][:, t, :env.aux.shape[1]], out["last"][:, t, :env.last.shape[1]] = env.aux, env.last
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def trace(name, env_id):
    """run_oracle without forced comparisons (computed once, read-only)."""
    return run_oracle(name, env_id)
