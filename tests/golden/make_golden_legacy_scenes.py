"""Generate legacy_scenes.npz from the reference (romi2002/gym-usv) -- build container only.

Run:  python tests/golden/make_golden_legacy_scenes.py      (needs the reference; writes one .npz file here)

The reference is imported read-only through ``refharness``; only inputs and outputs are stored.  Per scene of
tests/legacy_scenes.py and per env id (usv-asmc-v0: UsvAsmcEnv, usv-asmc-ye-int-v0: UsvAsmcYeIntEnv, usv-pid-v0:
UsvPidEnv): a fresh reference env, np.random.seed(0), reset(), the scene's state written over ``position``,
``velocity``, ``aux_vars``, ``last``, ``target`` and ``state[5]`` (UsvAsmcYeIntEnv carries ye_int as aux_vars[3] and
ye_last as last[9]), then the batch's steps with the scene's float32 scalar actions.  The arrays get the dtype the
reference's own code leaves them in: UsvAsmcEnv float32 after a step (scenes with elapsed != 0) and float64 after a
reset (elapsed = 0), the other two float64; ``target`` is float64 everywhere.  Truncation is applied as the
project does: not done and elapsed >= limit.

Keys, per id (``v0`` / ``yeint`` / ``pid``) with the id's batches concatenated in legacy_scenes.BATCHES order
(legacy_scenes.fixture() cuts a batch out): ``<id>__count``, ``<id>__limit`` and ``<id>__steps`` per batch;
``<id>__<input>`` the scene inputs as tests/legacy_scenes.py builds them (tests/test_legacy_scenes.py checks they are
the same bits; ``actions`` [n, 4], zero past a batch's steps); and per step, as ``<id>__out_<key>``, ``obs`` [n, 4, 6] float32,
``reward``, ``terminated``, ``truncated`` and the reference's ``position``, ``velocity``, ``aux`` [n, 4, 4] and
``last`` [n, 4, 10] after the step (cut to the id's own steps and columns; float64, but float32 for usv-asmc-v0, whose step
stores float32; steps past a batch's are zero).  The file is
written with make_golden_dynamics.save's fixed zip timestamps, so a second run gives the same bytes.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import refharness  # noqa: E402
import legacy_scenes as LS  # noqa: E402
from make_golden_dynamics import save  # noqa: E402


def run_scene(cls, env_id, sc, i):
    np.random.seed(0)
    env = cls()
    env.reset()
    v0 = env_id == LS.V0
    dt = np.float32 if (v0 and sc["elapsed"][i] != 0) else np.float64
    aux, last = list(sc["aux"][i]), list(sc["last"][i])
    if env_id == LS.YEINT:
        aux, last = aux + [sc["ye2"][i, 0]], last + [sc["ye2"][i, 1]]
    env.position = np.array([sc["x"][i], sc["y"][i], sc["psi"][i]], dtype=dt)
    env.velocity = np.array([sc["u"][i], sc["v"][i], sc["r"][i]], dtype=dt)
    env.aux_vars, env.last = np.array(aux, dtype=dt), np.array(last, dtype=dt)
    env.target = np.array(sc["target"][i], dtype=np.float64)
    state = np.array(env.state, dtype=dt)
    state[5] = sc["a_last"][i]
    env.state = state
    S, limit, elapsed = sc["steps"], sc["limit"], int(sc["elapsed"][i])
    out = dict(obs=np.zeros((S, 6), np.float32), reward=np.zeros(S), terminated=np.zeros(S, bool), truncated=np.zeros(S, bool),
               position=np.zeros((S, 3)), velocity=np.zeros((S, 3)), aux=np.zeros((S, 4)), last=np.zeros((S, 10)))
    for t in range(S):
        o, r, d, _ = env.step(sc["actions"][i, t])
        elapsed += 1
        out["obs"][t], out["reward"][t], out["terminated"][t] = o, float(r), bool(d)
        out["truncated"][t] = (not d) and limit > 0 and elapsed >= limit
        out["position"][t], out["velocity"][t] = env.position, env.velocity
        out["aux"][t, :len(env.aux_vars)], out["last"][t, :len(env.last)] = env.aux_vars, env.last
    return out


def main():
    refharness.load_reference()
    import gym_usv.envs as E
    classes = {LS.V0: E.UsvAsmcEnv, LS.YEINT: E.UsvAsmcYeIntEnv, LS.PID: E.UsvPidEnv}
    arrays = {}

    def pad(a):                                      # [n, S, ...] -> [n, SMAX, ...]
        return np.concatenate([a, np.zeros((a.shape[0], LS.SMAX - a.shape[1]) + a.shape[2:], a.dtype)], axis=1)
    for env_id, cls in classes.items():
        parts = {}
        for name in LS.BATCHES:
            sc = LS.batch(name, env_id)
            n = len(sc["x"])
            for k, v in (("count", n), ("limit", sc["limit"]), ("steps", sc["steps"])):
                parts.setdefault(k, []).append(np.array([v], dtype=np.int64))
            if not n:
                continue
            for k in LS.INPUT_KEYS:
                parts.setdefault(k, []).append(pad(sc[k]) if k == "actions" else sc[k])
            rows = [run_scene(cls, env_id, sc, i) for i in range(n)]
            for k in rows[0]:
                parts.setdefault("out_" + k, []).append(pad(np.stack([r[k] for r in rows])))
            print(env_id, name, n, "scenes: terminated", int(sum(r["terminated"].sum() for r in rows)), "truncated",
                  int(sum(r["truncated"].sum() for r in rows)))
        for k, v in parts.items():
            a = np.concatenate(v)
            if k[4:] in LS.STATE_KEYS:
                w = {"aux": 4 if env_id == LS.YEINT else 3, "last": 10 if env_id == LS.YEINT else 9}.get(k[4:], 3)
                a = a[:, :LS.T if env_id != LS.V0 else LS.SMAX, :w]
                if env_id == LS.V0:                  # UsvAsmcEnv stores its state as float32: nothing is lost
                    assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
                    a = a.astype(np.float32)
            arrays[f"{LS.SHORT[env_id]}__{k}"] = a
    out = os.path.join(HERE, "legacy_scenes.npz")
    save(out, arrays)
    print("legacy_scenes.npz:", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
