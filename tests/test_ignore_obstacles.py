"""ignore_obstacles (gym_usv/envs/simple_env.py:49) without a GPU: the binding's constants and symbols, the
argument checks that run before any device call, and the CPU oracle with the switch set, pinned to the
reference's own trajectories (tests/golden/make_golden_ignore.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from ignore_fixture import FIXTURE_IDS, FIXTURES, IgnoreSimpleAsmcEnvBatch, IgnoreSimpleEnvBatch, block


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "usv_hip.h")).read()


def test_constants_match_header():
    from gym_usv_amd import _lib
    src = _header()
    assert int(re.search(r"USV_FLAG_IGNORE_OBSTACLES\s*=\s*(\d+)", src).group(1)) == _lib.FLAG_IGNORE_OBSTACLES == 2
    assert int(re.search(r"USV_FLAG_PERTURB\s*=\s*(\d+)", src).group(1)) == _lib.FLAG_PERTURB == 1
    assert int(re.search(r"#define USV_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 5
    bound = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert bound["usv_set_ignore_obstacles"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32])
    assert bound["usv_get_ignore_obstacles"] == (ctypes.c_int, [ctypes.c_void_p])
    assert re.search(r"int\s+usv_set_ignore_obstacles\(void\*\s*handle,\s*int32_t\s+on\);", src)
    assert re.search(r"int\s+usv_get_ignore_obstacles\(void\*\s*handle\);", src)


def test_symbols_resolve_and_config_unchanged(lib):
    assert lib.usv_set_ignore_obstacles and lib.usv_get_ignore_obstacles
    assert lib.usv_config_size() == 56 and lib.usv_abi_version() == 5
    # null handles are reported, not dereferenced
    assert lib.usv_set_ignore_obstacles(None, 1) == -1
    assert lib.usv_get_ignore_obstacles(None) == -1


def test_flag_validation_without_gpu(lib):
    from gym_usv_amd import _lib
    h = ctypes.c_void_p()
    cfg = _lib.UsvConfig()
    for mode in (_lib.MODE_ASMC_V0, _lib.MODE_ASMC_YE_INT_V0, _lib.MODE_PID_V0):   # no obstacles there
        lib.usv_config_default(ctypes.byref(cfg), mode, 16)
        cfg.flags = _lib.FLAG_IGNORE_OBSTACLES
        assert lib.usv_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == -1
        assert b"USV_FLAG_IGNORE_OBSTACLES" in lib.usv_last_error() and not h.value
    for mode, flags in ((_lib.MODE_SIMPLE, 2), (_lib.MODE_ASMC_SIMPLE, 2), (_lib.MODE_ASMC_SIMPLE, 3)):
        lib.usv_config_default(ctypes.byref(cfg), mode, 16)
        cfg.flags = flags
        rc = lib.usv_create(ctypes.byref(cfg), 0, ctypes.byref(h))
        msg = lib.usv_last_error()
        if rc == 0:                                  # a GPU is present: the handle starts with the switch on
            assert lib.usv_get_ignore_obstacles(h) == 1
            lib.usv_destroy(h)
        else:                                        # past the config check: the failure is the device's
            assert rc != -1 or b"device" in msg, msg
            assert b"flags" not in msg and b"FLAG" not in msg, msg
    lib.usv_config_default(ctypes.byref(cfg), _lib.MODE_SIMPLE, 16)
    for flags in (4, 6, 8):                          # bit 4 and above stay unknown
        cfg.flags = flags
        assert lib.usv_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == -1
        assert b"unknown flags" in lib.usv_last_error()
    cfg.flags = 3                                    # do_perturb stays usv-asmc-simple's
    assert lib.usv_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == -1
    assert b"USV_FLAG_PERTURB" in lib.usv_last_error()


@pytest.mark.parametrize("fname,prefix,env_id", FIXTURES, ids=FIXTURE_IDS)
def test_ignoring_oracle_matches_reference(golden, fname, prefix, env_id):
    """The oracle subclass whose _finish_step restates :222-224, :155 and :334 replays the reference's
    ignore_obstacles trajectories at float64: header and reward within 1e-12, flags exact, resets
    (NumPy-exact, obstacles still drawn) included."""
    g = block(golden(fname), prefix)
    assert bool(g["sensors_all_one"])                # the reference's sensors were exactly 1.0 throughout
    assert not g["terminated"].any()
    n, T = g["actions"].shape[:2]
    limit = int(g["limit"])
    e = (IgnoreSimpleEnvBatch if env_id == "usv-simple" else IgnoreSimpleAsmcEnvBatch)(n)
    obs = e.reset(seeds=[int(s) for s in g["seeds"]])
    np.testing.assert_allclose(obs, g["obs0"], rtol=0, atol=1e-12)
    assert np.all(obs[:, 15:] == 0)                  # a never-stepped env's stale scan
    np.testing.assert_allclose(e.position, g["init_position"], rtol=0, atol=1e-13)
    np.testing.assert_array_equal(e.n_obs, g["init_n_obs"])      # obstacles are still drawn
    np.testing.assert_allclose(e.ox, g["init_ox"], rtol=0, atol=1e-13)
    elapsed = np.zeros(n, dtype=np.int64)
    worst = {"hdr": 0.0, "rew": 0.0}
    for t in range(T):
        o, r, te, tr = e.step(g["actions"][:, t])
        elapsed += 1
        tr = tr | (elapsed >= limit)
        np.testing.assert_array_equal(te, g["terminated"][:, t], err_msg=f"t={t}")
        np.testing.assert_array_equal(tr, g["truncated"][:, t], err_msg=f"t={t}")
        assert np.all(o[:, 15:] == np.float32(1.0))
        worst["hdr"] = max(worst["hdr"], float(np.abs(o[:, :15].astype(np.float64) - g["final_obs"][:, t]).max()))
        worst["rew"] = max(worst["rew"], float(np.abs(r - g["reward"][:, t]).max()))
        done = te | tr
        if done.any():                               # same-step autoreset: the stream continues
            idx = np.flatnonzero(done)
            ro = e.reset(idx=idx)
            assert np.all(ro[idx, 15:] == np.float32(1.0))       # stale sensor_data (:302)
            elapsed[idx] = 0
    print(f"\n[{fname} {prefix or '-'}] max |hdr| err {worst['hdr']:.3e}, max |rew| err {worst['rew']:.3e}")
    assert worst["hdr"] <= 1e-12 and worst["rew"] <= 1e-12, worst
    if prefix:
        assert g["truncated"].sum() >= n             # TimeLimit 40 over 120 steps: truncation occurs
