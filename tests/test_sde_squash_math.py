"""The arithmetic of the squashed gSDE head (gym-usv_amd/csrc/usv_sde_math.hpp: forward tail, backward, the order
of g_std's sum over rows) and the argument checks of usv_sde_squash_forward / _backward, without a GPU.

A stand-alone host program that includes only usv_sde_math.hpp replays sde_squash_forward_kernel,
sde_squash_backward_kernel and sde_std_finalise_kernel lane by lane, pass by pass and partial by partial with the
header's own functions, and is compared with the float64 reference of tests/sde_squash_ref.py, whose backward is
torch-CPU float64 autograd on the definition.  The host's transcendentals are libm's (the device's Box-Muller is
the hardware's), so this pins the formulas and the operation order, and the GPU test pins the device.

Eight errors, each divided by the sum of the absolute magnitudes of its terms (sde_squash_ref.errors), over
sde_squash_ref.SHAPES.  Each must stay under the ceiling of 1e-5 (the existing head's: a condition, not a
measurement) and under 4x the maximum this program measured, MEASURED below: 4x is this head's margin.

Measured maxima of the host replay over SHAPES (x86-64, glibc):
    z 4.13e-07  u 4.26e-07  a 8.75e-08  var 1.68e-07  logp 9.07e-08  g_mean 1.47e-07  g_lat 1.86e-07  g_std 9.66e-08
The gradient errors are taken at the program's own normals, which "z" bounds against sde_ref.normals as the
existing head's test does; why, and the figures at the reference's normals, are in sde_squash_ref.py's docstring."""
import ctypes

import numpy as np
import pytest

import sde_squash_ref as Q
from sde_host import bits, compile_replay, load_lib, make_sde, run_replay

MEASURED = {"z": 4.14e-7, "u": 4.26e-7, "a": 8.75e-8, "var": 1.68e-7, "logp": 9.07e-8, "g_mean": 1.47e-7,
            "g_lat": 1.86e-7, "g_std": 9.66e-8}         # the host replay's maxima over SHAPES (rounded up)
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "usv_sde_math.hpp"
using namespace usv;

// squash n L A seed gid0 epoch low0 low1 high0 high1
//   stdin: mean [n][A], lat [n][L], std [L][A], g_act [n][A], g_logp [n] f32
//   stdout: act, env, gauss, var [n][A], logp [n], g_mean [n][A], g_lat [n][L], g_std [L][A], z [n][L][A] f32
//   stderr: "C R P"
int main(int argc, char** argv) {
  if (argc != 12 || std::strcmp(argv[1], "squash")) return 2;
  const int n = std::atoi(argv[2]), L = std::atoi(argv[3]), A = std::atoi(argv[4]);
  const uint64_t seed = std::strtoull(argv[5], nullptr, 10), gid0 = std::strtoull(argv[6], nullptr, 10);
  const uint32_t epoch = (uint32_t)std::strtoul(argv[7], nullptr, 10);
  const float low[2] = {(float)std::atof(argv[8]), (float)std::atof(argv[9])};
  const float high[2] = {(float)std::atof(argv[10]), (float)std::atof(argv[11])};
  if (!sde_latent_ok(L) || (A != 1 && A != 2) || n <= 0) return 4;
  std::vector<float> mean((size_t)n * A), lat((size_t)n * L), sd((size_t)L * A), ga((size_t)n * A), gl(n);
  for (std::vector<float>* v : {&mean, &lat, &sd, &ga, &gl})
    if (std::fread(v->data(), 4, v->size(), stdin) != v->size()) return 3;
  std::vector<float> act((size_t)n * A), env((size_t)n * A), gauss((size_t)n * A), var((size_t)n * A), logp(n);
  for (int e = 0; e < n; ++e) {                           // sde_squash_forward_kernel, wave e
    const uint64_t gid = gid0 + (uint64_t)e;
    float nz[2][kSdeLanes], vr[2][kSdeLanes];
    for (int k = 0; k < 2; ++k)
      for (int l = 0; l < kSdeLanes; ++l) nz[k][l] = vr[k][l] = 0.0f;
    for (int j = 0; j < L; ++j)                           // lane sde_lane(j), ascending j
      for (int k = 0; k < A; ++k) {
        uint32_t o[4];
        float z[4];
        sde_block(seed, gid, epoch, sde_block_of(j, k, A), o);
        sde_normals(o, z);
        const float s = sd[(size_t)j * A + k];
        sde_accum(lat[(size_t)e * L + j], s, sde_weight(s, z[sde_slot_of(j, k, A)]), nz[k][sde_lane(j)], vr[k][sde_lane(j)]);
      }
    float lp = 0.0f;
    for (int k = 0; k < A; ++k) {                         // lane 0's tail
      const size_t at = (size_t)e * A + k;
      const float noise = sde_tree_sum(nz[k]), v = sde_tree_sum(vr[k]);
      const float u = sde_action(mean[at], noise);
      float a, om;
      sde_squash(u, a, om);
      act[at] = a;
      env[at] = sde_unscale(a, low[k], high[k]);
      gauss[at] = u;
      var[at] = v;
      lp = lp + sde_squash_logp_term(u, mean[at], v, om);
    }
    logp[e] = lp;
  }
  const int R = (int)sde_rows_per_partial(n), P = (int)sde_partials(n), LA = L * A;
  std::vector<float> g_mean((size_t)n * A), g_lat((size_t)n * L), g_std(LA), part((size_t)P * LA), zs((size_t)n * LA);
  for (int p = 0; p < P; ++p) {                           // sde_squash_backward_kernel, wave p
    const int e0 = p * R, e1 = e0 + R < n ? e0 + R : n;
    for (int l = 0; l < kSdeLanes; ++l)
      for (int j0 = kSdePerLane * l; j0 < L; j0 += kSdePass) {
        float s[8], gs[8];
        for (int i = 0; i < 4 * A; ++i) {
          s[i] = sd[(size_t)j0 * A + i];
          gs[i] = 0.0f;
        }
        for (int e = e0; e < e1; ++e) {
          float gn[2], gv[2];
          for (int k = 0; k < A; ++k) {
            const size_t at = (size_t)e * A + k;
            float G;
            sde_squash_grad_tail(gauss[at], mean[at], var[at], ga[at], gl[e], G, gn[k], gv[k]);
            if (j0 == 0) g_mean[at] = G;
          }
          const float* const x = &lat[(size_t)e * L + j0];
          float gx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          for (int m = 0; m < A; ++m) {
            uint32_t o[4];
            float z[4];
            sde_block(seed, gid0 + (uint64_t)e, epoch, (uint32_t)(j0 / 4) * A + m, o);
            sde_normals(o, z);
            std::memcpy(&zs[(size_t)e * LA + (size_t)j0 * A + 4 * m], z, 16);
            for (int q = 0; q < 4; ++q) {
              const int i = 4 * m + q;
              sde_grad_accum(x[i / A], s[i], z[q], gn[i % A], gv[i % A], gx[i / A], gs[i]);
            }
          }
          std::memcpy(&g_lat[(size_t)e * L + j0], gx, 16);
        }
        std::memcpy(&part[((size_t)p * L + j0) * A], gs, 16 * A);
      }
  }
  for (int i = 0; i < LA; ++i) g_std[i] = sde_partials_sum(&part[i], (size_t)LA, P);    // sde_std_finalise_kernel
  for (const std::vector<float>* v : {&act, &env, &gauss, &var, &logp, &g_mean, &g_lat, &g_std, &zs})
    std::fwrite(v->data(), 4, v->size(), stdout);
  std::fprintf(stderr, "C %d %d\n", R, P);
  return 0;
}
"""


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return compile_replay(tmp_path_factory.mktemp("sde_squash_math"), MAIN)


def replay(exe, n, L, A, case_inputs, seed=Q.SEED, gid0=Q.GID0, epoch=Q.EPOCH, low=Q.LOW, high=Q.HIGH):
    fields = (("act", (n, A)), ("env", (n, A)), ("gauss", (n, A)), ("var", (n, A)), ("logp", (n,)), ("g_mean", (n, A)),
              ("g_lat", (n, L)), ("g_std", (L, A)), ("z", (n, L, A)))
    out, (out["R"], out["P"]) = run_replay(
        exe, ("squash", n, L, A, seed, gid0, epoch, *(repr(float(x)) for x in (*low, *high))), case_inputs,
        [(name, np.float32, shape) for name, shape in fields])
    return out


@pytest.mark.parametrize("n,L,A", Q.SHAPES, ids=lambda v: str(v))
def test_replay_against_the_float64_reference(programs, n, L, A):
    inp = Q.inputs(n, L, A)
    got = replay(programs["plain"], n, L, A, inp)
    assert got["R"] == -(-n // 1024) and got["P"] == -(-n // got["R"]) and got["P"] <= 1024
    assert all(np.isfinite(got[k]).all() for k in ("act", "env", "gauss", "var", "logp", "g_mean", "g_lat", "g_std"))
    # the unscale, bit for bit on the program's own actions; actions in [-1, 1]
    lo, hi = np.float32(Q.LOW[:A]), np.float32(Q.HIGH[:A])
    assert (bits(got["env"]) == bits(Q.unscale(got["act"], lo, hi))).all()
    assert (np.abs(got["act"]) <= 1.0).all()
    if n >= 2:
        assert (got["gauss"][0] == inp[0][0]).all() and (got["var"][0] == 0).all()   # the zero latent row
        assert (got["act"][-1] == 1.0).all()                                        # the saturated row
    err = Q.errors(got, inp)
    print(f"host replay n {n} L {L} A {A}: " + " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert v < Q.CEILING, (k, v)
        assert v <= BOUND[k], (k, v, BOUND[k])


def test_zero_upstream_gradients_shards_and_the_order_of_the_row_sum(programs):
    """g_act = g_logp = 0 gives zero gradients.  A row run on its own (a shard of one row with its global env id)
    gives the whole's g_mean and g_lat rows bit for bit, and its g_std is that row's partial (n <= 1024: one row
    per partial); the whole's g_std is the strands-and-tree sum of those, restated here in NumPy float32."""
    n, L, A = 40, 8, 2
    mean, lat, std, ga, gl = Q.inputs(n, L, A)
    zero = replay(programs["plain"], n, L, A, (mean, lat, std, 0 * ga, 0 * gl))
    assert not zero["g_mean"].any() and not zero["g_lat"].any() and not zero["g_std"].any()
    got = replay(programs["plain"], n, L, A, (mean, lat, std, ga, gl))
    assert (got["R"], got["P"]) == (1, n)
    strands = [np.zeros((L, A), np.float32) for _ in range(16)]
    for e in range(n):
        one = replay(programs["plain"], 1, L, A, (mean[e:e + 1], lat[e:e + 1], std, ga[e:e + 1], gl[e:e + 1]),
                     gid0=Q.GID0 + e)
        assert (bits(one["g_lat"]) == bits(got["g_lat"][e:e + 1])).all()
        assert (bits(one["g_mean"]) == bits(got["g_mean"][e:e + 1])).all()
        strands[e % 16] = strands[e % 16] + one["g_std"]
    h = 1
    while h < 16:
        for i in range(0, 16, 2 * h):
            strands[i] = strands[i] + strands[i + h]
        h *= 2
    assert strands[0].dtype == np.float32 and (bits(strands[0]) == bits(got["g_std"])).all()


def test_replay_under_sanitizers(programs):
    for n, L, A in ((5, 260, 2), (1027, 8, 2), (1, 4, 1)):
        got = replay(programs["san"], n, L, A, Q.inputs(n, L, A), gid0=2 ** 32 - 1, epoch=0xFFFFFFFF)
        assert np.isfinite(got["g_std"]).all()


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_squash_calls_refuse_bad_arguments_without_gpu(lib):
    """Everything usv_sde_squash_forward / _backward can refuse before a HIP call is refused with USV_ERR_ARG and
    a message: every case usv_sde_sample refuses, one of gauss / var NULL, a misaligned or short-stride g_lat,
    a NULL scratch."""
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    nan = float("nan")
    FWD = ("mean", "lat", "std", "act", "env", "logp", "gauss", "var")
    BWD = ("mean", "lat", "std", "gauss", "var", "g_act", "g_logp", "g_mean", "g_lat", "g_std", "scratch")

    def calls(s, word, which=(0, 1), stride=8, g_stride=8, **kw):
        sp = ctypes.byref(s) if s is not None else None
        a = {k: p for k in FWD + BWD}
        a.update(kw)
        fns = (lambda: lib.usv_sde_squash_forward(sp, 1, a["mean"], a["lat"], stride, a["std"], a["act"], a["env"],
                                                  a["logp"], a["gauss"], a["var"], None),
               lambda: lib.usv_sde_squash_backward(sp, 1, a["mean"], a["lat"], stride, a["std"], a["gauss"], a["var"],
                                                   a["g_act"], a["g_logp"], a["g_mean"], a["g_lat"], g_stride,
                                                   a["g_std"], a["scratch"], None))
        for i in which:
            assert fns[i]() == -1, (word, i)
            assert word in lib.usv_last_error(), (word, i, lib.usv_last_error())

    calls(None, b"null usv_sde")
    for kw, word in ((dict(n=0), b"n must be > 0"), (dict(n=-3), b"n must be > 0"), (dict(act_dim=0), b"act_dim"),
                     (dict(act_dim=3), b"act_dim"), (dict(latent_dim=0), b"latent_dim"), (dict(latent_dim=6), b"latent_dim"),
                     (dict(latent_dim=4100), b"latent_dim"), (dict(latent_dim=-4), b"latent_dim"),
                     (dict(reserved=1), b"reserved"), (dict(low=(2.0, -1.0, 0, 0)), b"low must be <= high"),
                     (dict(low=(0.0, nan, 0, 0)), b"low must be <= high"), (dict(high=(nan, 1.0, 0, 0)), b"low must be <= high")):
        calls(make_sde(**kw), word)
    calls(make_sde(act_dim=1, low=(0.0, 5.0, 0, 0)), b"null buffer", std=None)
    for stride in (7, 10, 4):
        calls(make_sde(), b"row stride", stride=stride)
        calls(make_sde(), b"g_lat row stride", which=(1,), g_stride=stride)
    # forward: gauss and var together or not at all
    calls(make_sde(), b"both NULL or both set", which=(0,), gauss=None)
    calls(make_sde(), b"both NULL or both set", which=(0,), var=None)
    for name in ("mean", "lat", "std", "act", "env", "logp"):
        calls(make_sde(), b"null buffer", which=(0,), **{name: None})
        calls(make_sde(), b"aligned", which=(0,), **{name: p + 2})
    for name in ("gauss", "var"):
        calls(make_sde(), b"aligned", which=(0,), **{name: p + 2})
    # backward: gauss, var and scratch are needed; g_act and g_logp may be NULL (the next refusal is the device's)
    calls(make_sde(), b"null scratch", which=(1,), scratch=None)
    for name in ("mean", "lat", "std", "gauss", "var", "g_mean", "g_lat", "g_std"):
        calls(make_sde(), b"null buffer", which=(1,), **{name: None})
    for name in BWD:
        calls(make_sde(), b"aligned", which=(1,), **{name: p + 2})
    for name in ("lat", "g_lat", "scratch"):                # 4-B aligned is not enough for the 16-B accesses
        calls(make_sde(), b"aligned", which=(1,), **{name: p + 4})
        calls(make_sde(), b"aligned", which=(1,), **{name: p + 8})
    calls(make_sde(), b"aligned", which=(0,), lat=p + 4)
    calls(make_sde(), b"device pointer", g_act=None, g_logp=None)       # host memory: refused by the device check


def test_scratch_floats(lib):
    for n, P in ((1, 1), (1024, 1024), (1025, 513), (1027, 514), (65536, 1024)):
        for L, A in ((8, 2), (300, 2), (512, 1)):
            s = make_sde(n=n, latent_dim=L, act_dim=A)
            assert lib.usv_sde_squash_scratch_floats(ctypes.byref(s)) == P * L * A, (n, L, A)
    assert lib.usv_sde_squash_scratch_floats(None) == 0
    assert lib.usv_sde_squash_scratch_floats(ctypes.byref(make_sde(latent_dim=6))) == 0


def test_squashed_checks_its_arguments_first():
    import gym_usv_amd
    from gym_usv_amd.sde import DeviceSDE, SquashedSample
    assert gym_usv_amd.SquashedSample is SquashedSample
    assert SquashedSample._fields == ("actions", "env_actions", "log_prob", "gaussian_actions")
    assert callable(DeviceSDE.squashed)
