"""The step-variant rules (gym-usv_amd/csrc/usv_variant.hpp): which variant a configuration runs by
default and which ones usv_set_kernel_variant lets it select.  The expected answers are a Python
restatement of the documented rules ("The step kernels"), never the library's own.

CPU: usv_variant.hpp is plain host C++, compiled here on its own and printed over a grid.
GPU: usv_set_kernel_variant over the same kind x epb x lid grid on live handles.
"""
import itertools
import subprocess

import numpy as np
import pytest

SIMPLE, ASMC_SIMPLE, ASMC_V0 = 0, 1, 2          # usv_mode
F32, F64 = 0, 1                                 # usv_precision
BRUTE, WINDOW = 0, 1                            # usv_lidar_algo

CAPS = (29, 32, 33, 64)
NS = (1, 32767, 32768, 49151, 49152, 196607, 196608)
KINDS = tuple(range(8))
EPBS = (8, 16, 32, 48, 64, 128, 256)
LIDS = (0, 3, 5, 7, 0x103, 0x107, 0x207, 0x307)


def default_variant(mode, prec, lidar, cap, n):
    """(kind, epb, lid, prio, rowspan) a new handle runs."""
    lid = 3 if lidar == BRUTE else 7
    q = prec == F32 and lidar == WINDOW and cap <= 32
    d = prec == F64 and lidar == WINDOW and cap <= 32
    if q:
        kind, epb = (6 if mode == ASMC_SIMPLE else 5), (16 if n < 32768 else 128)
    elif d:
        kind, epb = (2 if mode == ASMC_SIMPLE else 3), (64 if n >= 49152 else 32)
    else:
        kind, epb = (2, 16) if mode == ASMC_SIMPLE else (1, 64)
    return kind, epb, lid, (0 if kind >= 4 else 1), int(n >= 196608)


def variant_allowed(mode, prec, cap, n, kind, epb, lid):
    """None if usv_set_kernel_variant refuses, else (lid without the row bits, prio, rowspan).
    lidar_algo is not consulted."""
    if mode not in (SIMPLE, ASMC_SIMPLE):
        return None
    rs, lid = lid & 0x300, lid & 0xff
    if rs == 0x300 or (rs and kind not in (4, 5, 6)):
        return None
    if kind == 1:
        ok = epb in (16, 32, 64) and lid in (0, 3, 7)
    elif kind == 2:
        ok = (epb in (8, 16, 32) or (epb == 64 and lid == 7 and prec == F64)) and lid in (0, 3, 7)
    elif kind == 3:
        ok = epb in (32, 64) and lid == 7 and prec == F64 and mode == SIMPLE
    elif kind in (4, 5, 6):
        ok = ((kind != 6 or mode == ASMC_SIMPLE) and (epb == 128 or (epb == 16 and kind != 4)) and lid == 7 and
              prec == F32 and cap <= 32)
    else:
        ok = False
    if not ok:
        return None
    return lid, (0 if kind >= 4 else 1), int(rs == 0x100 if rs else n >= 196608)


MAIN = r"""
#include <cstdio>
#include <initializer_list>
#include "usv_variant.hpp"
using namespace usv;
static const int caps[] = {%(caps)s}, ns[] = {%(ns)s}, epbs[] = {%(epbs)s}, lids[] = {%(lids)s};
static void allowed(const usv_config& c) {
  for (int kind = 0; kind < 8; ++kind)
    for (int epb : epbs)
      for (int lid : lids) {
        const VariantCheck r = variant_allowed(c, kind, epb, lid);
        std::printf("A %%d %%d %%d %%d %%d %%d %%d %%d : %%d %%d %%d %%d %%d %%d\n", c.mode, c.precision, c.lidar_algo,
                    c.obstacle_cap, c.num_envs, kind, epb, lid, r.refused == nullptr, r.v.kind, r.v.epb, r.v.lid,
                    r.v.prio, r.v.rowspan);
      }
}
int main() {
  static_assert(kWaveFused == 1 && kWaveSplit == 2 && kBlockDyn == 3 && kQueueSplit == 4 && kQueueFused == 5 &&
                kQueueChain == 6, "the kinds are part of the C ABI");
  static_assert(!is_queue(3) && is_queue(4) && is_queue(5) && is_queue(6) && !is_queue(7), "is_queue");
  usv_config c{};
  for (int mode : {USV_MODE_SIMPLE, USV_MODE_ASMC_SIMPLE})
    for (int prec : {USV_F32, USV_F64})
      for (int lidar : {USV_LIDAR_BRUTE, USV_LIDAR_WINDOW})
        for (int cap : caps)
          for (int n : ns) {
            c.mode = mode; c.precision = prec; c.lidar_algo = lidar; c.obstacle_cap = cap; c.num_envs = n;
            const Variant v = default_variant(c);
            std::printf("D %%d %%d %%d %%d %%d : %%d %%d %%d %%d %%d\n", mode, prec, lidar, cap, n, v.kind, v.epb, v.lid,
                        v.prio, v.rowspan);
            allowed(c);
          }
  c.mode = USV_MODE_ASMC_V0; c.precision = USV_F32; c.lidar_algo = USV_LIDAR_WINDOW; c.obstacle_cap = 32;
  c.num_envs = 64;
  allowed(c);
  return 0;
}
"""


def test_variant_rules_on_host(tmp_path):
    """default_variant and variant_allowed of usv_variant.hpp, built as host C++ without HIP, against
    the restatement above: mode x precision x lidar x cap x n for the defaults, and x kind x epb x lid
    for what may be selected (a refusal, or the installed lid / prio / rowspan); one legacy id, refused
    throughout."""
    from gym_usv_amd.build import CSRC, INCLUDE, hipcc
    src, exe = tmp_path / "variants.cpp", tmp_path / "variants"
    csv = lambda v: ", ".join(str(x) for x in v)
    src.write_text(MAIN % dict(caps=csv(CAPS), ns=csv(NS), epbs=csv(EPBS), lids=csv(LIDS)))
    subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", f"-I{INCLUDE}", f"-I{CSRC}", "-o", str(exe),
                    str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=120).stdout
    n_default = n_allowed = n_accepted = 0
    for line in out.splitlines():
        key, got = line[2:].split(" : ")
        key, got = [int(x) for x in key.split()], [int(x) for x in got.split()]
        if line[0] == "D":
            assert tuple(got) == default_variant(*key), line
            n_default += 1
            continue
        mode, prec, lidar, cap, n, kind, epb, lid = key
        want = variant_allowed(mode, prec, cap, n, kind, epb, lid)
        assert bool(got[0]) == (want is not None), line
        if want is not None:
            assert tuple(got[1:]) == (kind, epb) + want, line
            n_accepted += 1
        n_allowed += 1
    grid = 2 * 2 * 2 * len(CAPS) * len(NS)
    assert n_default == grid and n_allowed == (grid + 1) * len(KINDS) * len(EPBS) * len(LIDS)
    assert n_accepted > 0


GPU_CONFIGS = [("usv-simple", "f32", 32), ("usv-simple", "f32", 64), ("usv-simple", "f64", 32),
               ("usv-asmc-simple", "f32", 32), ("usv-asmc-simple", "f64", 32), ("usv-asmc-v0", "f32", 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("env_id,precision,cap", GPU_CONFIGS)
def test_set_kernel_variant_sweep(env_id, precision, cap):
    """usv_set_kernel_variant over kind x epb x lid on a 64-env handle accepts exactly what the
    restatement allows, and the handle still steps afterwards (the sweep ends in refusals: kind 7):
    one reset before and one step after the sweep are the only launches, outputs finite."""
    import torch
    import gym_usv_amd
    n = 64
    env = gym_usv_amd.make_vec(env_id, n, device=0, precision=precision, obstacle_cap=cap)
    env.reset(seed=0)
    mode = {"usv-simple": SIMPLE, "usv-asmc-simple": ASMC_SIMPLE, "usv-asmc-v0": ASMC_V0}[env_id]
    prec = F32 if precision == "f32" else F64
    wrong = []
    for kind, epb, lid in itertools.product(KINDS, EPBS, LIDS):
        rc = env.lib.usv_set_kernel_variant(env._h, kind, epb, lid)
        want = variant_allowed(mode, prec, cap, n, kind, epb, lid) is not None
        if (rc == 0) != want:
            wrong.append((kind, epb, lid, rc))
    assert not wrong, f"accept / refuse differs from the rules (kind, epb, lid, rc): {wrong[:10]}"
    assert rc != 0                                  # the last call was refused
    act = torch.zeros((n, env.act_dim), dtype=torch.float32, device=env.device)
    obs, rew, term, trunc, _ = env.step(act)
    torch.cuda.synchronize()
    assert obs.shape == (n, env.obs_dim)
    assert np.isfinite(obs.cpu().numpy()).all() and np.isfinite(rew.cpu().numpy()).all()
    env.close()
