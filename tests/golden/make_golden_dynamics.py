"""Generate dynamics_scenes.npz from the reference (romi2002/gym-usv) -- build container only.

Run:  python tests/golden/make_golden_dynamics.py      (needs the reference; writes one .npz file here)

The reference is imported read-only through ``refharness`` (as make_golden.py does); only inputs and
outputs are stored.  Per scene of tests/dynamics_scenes.py and per env id (usv-simple, usv-asmc-simple): a
fresh reference env, a seeded reset, the scene's state written over the reset's attributes (the names
of make_golden_ignore.snapshot; UsvAsmc's psi_d_last is ``asmc.so_filter[0]``), then T steps with the
scene's actions.  TimeLimit is applied as gym_usv/__init__.py registers it: truncated also when the
elapsed count reaches the batch's limit.

Keys: ``<batch>__<input>`` the scene inputs as the test module builds them (tests/test_dynamics_scenes.py
checks they are the same bits) and, per env id (``simple`` / ``asmc``), ``<batch>__<id>__hdr`` [n, T, 15]
float32 (the 15 header entries of the step observation), ``reward``, ``terminated``, ``truncated``, ``info``
[n, T, 22] (the step info values in the library's column order) and ``psi_d_last`` [n, T]; the contact
batches also ``sensors`` [n, T, 128] float32.  Elsewhere every sensor entry is 1.0, which ``sensors_all_one``
records.  The file is written with fixed zip timestamps, so a second run gives the same bytes.
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import refharness  # noqa: E402
import dynamics_scenes as DS  # noqa: E402

SHORT = {"usv-simple": "simple", "usv-asmc-simple": "asmc"}


def run_scene(cls, sc, i, limit):
    env = cls(render_mode=None)
    env.reset(seed=0)
    z = 0.0
    env.position = np.array([sc["x"][i], sc["y"][i], sc["psi"][i]])
    env.velocity = np.array([sc["u"][i], z, sc["r"][i]])
    env.last_action = np.array([sc["last_u"][i], z, sc["last_r"][i]])
    env.max_action = np.array([sc["max_u"][i], z, sc["max_r"][i]])
    env.reference_velocity = float(sc["ref_v"][i])
    env.progress = float(sc["progress"][i])
    env.path_start = np.array([sc["path_x0"][i], sc["path_y0"][i]])
    env.path_end = np.array([sc["path_x1"][i], sc["path_y1"][i]])
    env.obstacle_n = 1
    env.obstacle_positions = np.array([[sc["ox"][i], sc["oy"][i]]])
    env.obstacle_radius = np.array([sc["orad"][i]])
    asmc = hasattr(env, "asmc")
    if asmc:
        env.asmc.so_filter[0] = sc["asmc0"][i]
    elapsed = int(sc["elapsed"][i])
    out = dict(hdr=np.zeros((DS.T, 15), np.float32), sensors=np.zeros((DS.T, 128), np.float32), reward=np.zeros(DS.T),
               terminated=np.zeros(DS.T, bool), truncated=np.zeros(DS.T, bool), info=np.zeros((DS.T, 22)),
               psi_d_last=np.zeros(DS.T))
    for t in range(DS.T):
        o, r, te, tr, info = env.step(sc["actions"][i, t])
        elapsed += 1
        tr = bool(tr) or (limit > 0 and elapsed >= limit)
        row = {k: np.asarray(v, dtype=np.float64)[None] for k, v in info.items()}
        out["hdr"][t], out["sensors"][t], out["reward"][t] = o[:15], o[15:], r
        out["terminated"][t], out["truncated"][t] = bool(te), tr
        out["info"][t] = DS.info_rows(row)[0]
        out["psi_d_last"][t] = env.asmc.so_filter[0] if asmc else 0.0
    return out


def save(path, arrays):
    """np.savez_compressed with fixed member timestamps (identical bytes on every run)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k], order="C"), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                        compress_type=zipfile.ZIP_DEFLATED)


def main():
    refharness.load_reference()
    import gym_usv.envs as E
    classes = {"usv-simple": E.UsvSimpleEnv, "usv-asmc-simple": E.UsvSimpleASMCEnv}
    arrays, ones = {}, True
    for name in DS.BATCHES:
        sc = DS.batch(name)
        n = len(sc["x"])
        for k in DS.INPUT_KEYS:
            arrays[f"{name}__{k}"] = sc[k]
        arrays[f"{name}__limit"] = np.int64(sc["limit"])
        for env_id, cls in classes.items():
            rows = [run_scene(cls, sc, i, sc["limit"]) for i in range(n)]
            for k in rows[0]:
                a = np.stack([r[k] for r in rows])
                if k == "sensors":
                    if name in DS.WITH_OBSTACLES:
                        arrays[f"{name}__{SHORT[env_id]}__{k}"] = a
                    else:
                        ones = ones and bool(np.all(a == np.float32(1.0)))
                elif k != "psi_d_last" or env_id != "usv-simple":
                    arrays[f"{name}__{SHORT[env_id]}__{k}"] = a
            print(name, env_id, n, "scenes: terminated", int(sum(r["terminated"].sum() for r in rows)), "truncated",
                  int(sum(r["truncated"].sum() for r in rows)))
    arrays["sensors_all_one"] = np.bool_(ones)
    out = os.path.join(HERE, "dynamics_scenes.npz")
    save(out, arrays)
    print("dynamics_scenes.npz:", os.path.getsize(out), "bytes; sensors all 1.0 outside the contact batches:", ones)


if __name__ == "__main__":
    main()
