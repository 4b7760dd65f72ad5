"""Generate the ignore_obstacles fixtures from the reference (romi2002/gym-usv) -- build container only.

Run:  python tests/golden/make_golden_ignore.py      (needs the reference; writes two .npz files here)

The reference is imported read-only through ``refharness`` (as make_golden.py does); only inputs and
outputs are stored.  ``ignore_obstacles = True`` is set on the reference env after construction and
before the first reset, the way its users set it (gym_usv/envs/simple_env.py:49): every sensor reading
is then the maximum range (:222-224), the reward has no collision term (:155) and the env never
terminates on an obstacle (:334).

* ``simple_ignore_traj.npz``      -- usv-simple, 16 envs x 120 steps, seeds 0..15, TimeLimit 500; plus a
                                     second block (keys ``tl_*``) of 16 envs under TimeLimit 40: a
                                     TimeLimit-free env stepped with ``elapsed >= 40`` recorded as
                                     truncation (as simple_traj_tl.npz was made), so truncation occurs.
* ``asmc_simple_ignore_traj.npz`` -- usv-asmc-simple, 16 envs x 120 steps, seeds 0..15, TimeLimit 1000.

Keys are those of simple_traj.npz, but of the step observations only ``final_obs[..., :15]``, the 15
header entries, is stored; ``sensors_all_one`` confirms that every sensor entry of every recorded obs after the
first step was exactly 1.0 (``obs0`` keeps the reset's full row: a fresh env's stale scan is zeros).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refharness  # noqa: E402

CAP = 32
HDR = 15


def snapshot(env):
    n = env.obstacle_n
    ox, oy, r = np.zeros(CAP), np.zeros(CAP), np.zeros(CAP)
    ox[:n], oy[:n], r[:n] = env.obstacle_positions[:, 0], env.obstacle_positions[:, 1], env.obstacle_radius
    return dict(position=np.array(env.position, dtype=np.float64),
                velocity=np.array(env.velocity, dtype=np.float64),
                last_action=np.array(env.last_action, dtype=np.float64),
                progress=float(env.progress), path_start=np.array(env.path_start),
                path_end=np.array(env.path_end), target=np.array(env.target_position),
                max_action=np.array(env.max_action, dtype=np.float64),
                ref_v=float(env.reference_velocity), n_obs=int(n), ox=ox, oy=oy, orad=r,
                sensors=np.array(env.sensor_data[:, 1], dtype=np.float64))


def rollout(cls, limit, n_env=16, T=120, seed0=0, act_seed=7):
    """Per env: ignore_obstacles set, seeded reset, T random-action steps under TimeLimit(limit) with
    same-step autoreset (reset() with no seed continues the stream).  Returns the fixture's arrays."""
    rng = np.random.default_rng(act_seed)
    acts = np.stack([rng.uniform([0.2, -1], [1, 1], size=(T, 2)) for _ in range(n_env)]).astype(np.float32)
    seeds = np.arange(n_env) + seed0
    obs0 = np.zeros((n_env, 143), np.float32)
    fobs = np.zeros((n_env, T, HDR), np.float32)
    rew = np.zeros((n_env, T))
    term = np.zeros((n_env, T), bool)
    trunc = np.zeros((n_env, T), bool)
    ones = True
    st0 = []
    for e in range(n_env):
        env = cls(render_mode=None)
        env.ignore_obstacles = True
        o, _ = env.reset(seed=int(seeds[e]))
        obs0[e] = o
        st0.append(snapshot(env))
        elapsed = 0
        for t in range(T):
            o, r, te, tr, _ = env.step(acts[e, t])
            elapsed += 1
            tr = bool(tr) or (limit is not None and elapsed >= limit)
            ones = ones and bool(np.all(np.asarray(o)[HDR:] == np.float32(1.0)))
            fobs[e, t], rew[e, t], term[e, t], trunc[e, t] = o[:HDR], r, bool(te), tr
            if te or tr:
                o, _ = env.reset()
                elapsed = 0
                ones = ones and bool(np.all(np.asarray(o)[HDR:] == np.float32(1.0)))   # stale scan (:302)
    out = dict(seeds=seeds, actions=acts, obs0=obs0, final_obs=fobs, reward=rew, terminated=term,
               truncated=trunc, limit=np.int64(-1 if limit is None else limit), sensors_all_one=np.bool_(ones))
    out.update({f"init_{k}": np.stack([np.asarray(s[k]) for s in st0]) for k in st0[0]})
    return out


def main():
    refharness.load_reference()
    import gym_usv.envs as E
    a = rollout(E.UsvSimpleEnv, 500)
    b = rollout(E.UsvSimpleEnv, 40, seed0=100, act_seed=8)
    a.update({"tl_" + k: v for k, v in b.items()})
    np.savez_compressed(os.path.join(HERE, "simple_ignore_traj.npz"), **a)
    print("simple_ignore_traj.npz: terminated", int(a["terminated"].sum()), "truncated", int(a["truncated"].sum()),
          "| TimeLimit 40: truncated", int(b["truncated"].sum()), "| sensors all 1.0:",
          bool(a["sensors_all_one"]), bool(b["sensors_all_one"]))
    c = rollout(E.UsvSimpleASMCEnv, 1000)
    np.savez_compressed(os.path.join(HERE, "asmc_simple_ignore_traj.npz"), **c)
    print("asmc_simple_ignore_traj.npz: terminated", int(c["terminated"].sum()), "truncated",
          int(c["truncated"].sum()), "| sensors all 1.0:", bool(c["sensors_all_one"]))


if __name__ == "__main__":
    main()
