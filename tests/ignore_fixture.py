"""Shared by tests/test_ignore_obstacles.py (CPU) and tests/test_gpu_ignore_obstacles.py: the CPU oracle
with UsvSimpleEnv.ignore_obstacles set (gym_usv/envs/simple_env.py:49), and the fixtures' state images."""
import numpy as np

from oracle import usv_oracle as O


class _Ignore:
    """``_finish_step`` of SimpleEnvBatch with ignore_obstacles = True, restating the reference:
    every sensor reading is the maximum range (:222-224), the reward has no collision term (:155: its
    condition is ``min_sensor < 0.2 and not self.ignore_obstacles``) and ``terminated`` is
    ``min(obstacle_distance) < 0.05 and not self.ignore_obstacles`` (:334), i.e. never."""

    def _finish_step(self, a3):
        self.target, self.progress = self.closest_point()                 # :328
        self.sensors = np.full((self.n, O.SENSOR_COUNT), float(O.SENSOR_MAX_RANGE))   # :222-224
        terminated = np.zeros(self.n, dtype=bool)                         # :334
        pxy = self.position[:, :2]
        truncated = np.any((pxy > O.BOUND_HI) | (pxy < 0), axis=1)        # :336
        obs = self.obs(self.last_action)                                  # :338 (previous action)
        rew = self.reward(a3)                                             # :339
        # :155 -- reward() applies -20 where min_sensor < 0.2; with every reading at 100 it cannot
        assert self.sensors.min() >= 0.2
        self.info = self.step_info(a3, rew)
        self.last_action = a3                                             # :343
        return obs, rew, terminated, truncated


class IgnoreSimpleEnvBatch(_Ignore, O.SimpleEnvBatch):
    pass


class IgnoreSimpleAsmcEnvBatch(_Ignore, O.SimpleAsmcEnvBatch):
    pass


FIXTURES = [("simple_ignore_traj.npz", "", "usv-simple"), ("simple_ignore_traj.npz", "tl_", "usv-simple"),
            ("asmc_simple_ignore_traj.npz", "", "usv-asmc-simple")]
FIXTURE_IDS = ["simple", "simple-tl40", "asmc-simple"]


def block(g, prefix):
    """One block of a fixture file (``prefix`` '' or 'tl_') as a dict with the plain keys."""
    keys = ("seeds", "actions", "obs0", "final_obs", "reward", "terminated", "truncated", "limit",
            "sensors_all_one")
    out = {k: g[prefix + k] for k in keys}
    out.update({k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix + "init_")})
    return out


def golden_state(g):
    """The reference's post-reset state as UsvVectorEnv.set_state takes it (never-stepped: scan_valid 0)."""
    p, v, la, ma = g["init_position"], g["init_velocity"], g["init_last_action"], g["init_max_action"]
    return {"x": p[:, 0], "y": p[:, 1], "psi": p[:, 2], "u": v[:, 0], "v": v[:, 1], "r": v[:, 2],
            "last_u": la[:, 0], "last_r": la[:, 2], "progress": g["init_progress"],
            "path_x0": g["init_path_start"][:, 0], "path_y0": g["init_path_start"][:, 1],
            "path_x1": g["init_path_end"][:, 0], "path_y1": g["init_path_end"][:, 1],
            "max_u": ma[:, 0], "max_r": ma[:, 2], "ref_v": g["init_ref_v"],
            "n_obs": g["init_n_obs"], "obs_x": g["init_ox"], "obs_y": g["init_oy"],
            "obs_r": g["init_orad"], "sensor_last": g["init_sensors"], "elapsed": 0,
            "scan_valid": 0, "asmc": 0.0}
