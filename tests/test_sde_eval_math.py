"""The arithmetic of the gSDE evaluation head (gym-usv_amd/csrc/usv_sde_math.hpp: the variance sums, the
log-probability of stored actions, PPO's clipped surrogate, their backward and the order of g_std's sum over rows)
and the argument checks of usv_sde_eval_forward / _backward, without a GPU.

A stand-alone host program that includes only usv_sde_math.hpp replays sde_eval_forward_kernel,
sde_eval_backward_kernel and sde_std_finalise_kernel lane by lane, pass by pass and partial by partial with the
header's own functions, and is compared with the float64 reference of tests/sde_eval_ref.py, whose backward is
torch-CPU float64 autograd on the definition.  The host's exp and log are libm's, so this pins the formulas and the
operation order, and the GPU test pins the device.

Seven errors, each divided by the sum of the absolute magnitudes of its terms (sde_eval_ref.errors), over
sde_eval_ref.SHAPES.  Each must stay under the ceiling of 1e-5 (the project's: a condition, not a measurement) and
under 4x the maximum this program measured, MEASURED below: 4x is this head's margin.

Measured maxima of the host replay over SHAPES (x86-64, glibc):
    var 1.67e-07  logp 9.77e-08  ratio 6.17e-08  sur 6.54e-08  g_mean 1.74e-07  g_lat 2.54e-07  g_std 1.77e-07"""
import ctypes

import numpy as np
import pytest

import sde_eval_ref as E
import sde_squash_ref as Q
from sde_host import bits, compile_replay, load_lib, make_sde, run_replay

MEASURED = {"var": 1.67e-7, "logp": 9.77e-8, "ratio": 6.17e-8, "sur": 6.54e-8, "g_mean": 1.74e-7, "g_lat": 2.54e-7,
            "g_std": 1.77e-7}                             # the host replay's maxima over SHAPES (rounded up)
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "usv_sde_math.hpp"
using namespace usv;

// eval n L A clip ppo with_g_lat
//   stdin: mean [n][A], lat [n][L], std [L][A], act [n][A], old [n], adv [n], g_logp [n], g_sur [n] f32
//   stdout: var [n][A], logp [n], ratio [n], sur [n], t [n], g_mean [n][A], g_lat [n][L], g_std [L][A],
//           var_sample [n][A] f32 (ppo = 0: ratio, sur stay 0 and t = g_logp; with_g_lat = 0: g_lat stays the
//           sentinel -7e33; var_sample: the variance by the sample head's own sde_accum)
//   stderr: "C R P"
int main(int argc, char** argv) {
  if (argc != 8 || std::strcmp(argv[1], "eval")) return 2;
  const int n = std::atoi(argv[2]), L = std::atoi(argv[3]), A = std::atoi(argv[4]);
  const float clip = (float)std::atof(argv[5]);
  const bool ppo = std::atoi(argv[6]) != 0, with_g_lat = std::atoi(argv[7]) != 0;
  if (!sde_latent_ok(L) || (A != 1 && A != 2) || n <= 0) return 4;
  std::vector<float> mean((size_t)n * A), lat((size_t)n * L), sd((size_t)L * A), act((size_t)n * A), old(n), adv(n),
      gl(n), gs(n);
  for (std::vector<float>* v : {&mean, &lat, &sd, &act, &old, &adv, &gl, &gs})
    if (std::fread(v->data(), 4, v->size(), stdin) != v->size()) return 3;
  std::vector<float> var((size_t)n * A), var_sample((size_t)n * A), logp(n), ratio(n, 0.0f), sur(n, 0.0f), tt(n);
  for (int e = 0; e < n; ++e) {                           // sde_eval_forward_kernel, wave e
    float vr[2][kSdeLanes], vs[2][kSdeLanes], nz[2][kSdeLanes];
    for (int k = 0; k < 2; ++k)
      for (int l = 0; l < kSdeLanes; ++l) vr[k][l] = vs[k][l] = nz[k][l] = 0.0f;
    for (int j = 0; j < L; ++j)                           // lane sde_lane(j), ascending j
      for (int k = 0; k < A; ++k) {
        const float s = sd[(size_t)j * A + k], x = lat[(size_t)e * L + j];
        sde_var_accum(x, s, vr[k][sde_lane(j)]);
        sde_accum(x, s, sde_weight(s, 1.0f), nz[k][sde_lane(j)], vs[k][sde_lane(j)]);
      }
    float lp = 0.0f;
    for (int k = 0; k < A; ++k) {                         // lane 0's tail
      const size_t at = (size_t)e * A + k;
      var[at] = sde_tree_sum(vr[k]);
      var_sample[at] = sde_tree_sum(vs[k]);
      lp = lp + sde_logp_term(act[at], mean[at], var[at]);
    }
    logp[e] = lp;
    if (ppo) sur[e] = sde_ppo_surrogate(lp, old[e], adv[e], clip, ratio[e]);
  }
  const int R = (int)sde_rows_per_partial(n), P = (int)sde_partials(n), LA = L * A;
  std::vector<float> g_mean((size_t)n * A), g_lat((size_t)n * L, -7.0e33f), g_std(LA), part((size_t)P * LA);
  for (int p = 0; p < P; ++p) {                           // sde_eval_backward_kernel, wave p
    const int e0 = p * R, e1 = e0 + R < n ? e0 + R : n;
    for (int l = 0; l < kSdeLanes; ++l)
      for (int j0 = kSdePerLane * l; j0 < L; j0 += kSdePass) {
        float s[8], acc[8];
        for (int i = 0; i < 4 * A; ++i) {
          s[i] = sd[(size_t)j0 * A + i];
          acc[i] = 0.0f;
        }
        for (int e = e0; e < e1; ++e) {
          const float t = ppo ? sde_eval_row_grad(gl[e], gs[e], ratio[e], adv[e], clip) : gl[e];
          tt[e] = t;
          float gv[2];
          for (int k = 0; k < A; ++k) {
            const size_t at = (size_t)e * A + k;
            float G;
            sde_eval_grad_tail(act[at], mean[at], var[at], t, G, gv[k]);
            if (j0 == 0) g_mean[at] = G;
          }
          const float* const x = &lat[(size_t)e * L + j0];
          float gx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          for (int i = 0; i < 4 * A; ++i) sde_eval_grad_accum(x[i / A], s[i], gv[i % A], gx[i / A], acc[i]);
          if (with_g_lat) std::memcpy(&g_lat[(size_t)e * L + j0], gx, 16);
        }
        std::memcpy(&part[((size_t)p * L + j0) * A], acc, 16 * A);
      }
  }
  for (int i = 0; i < LA; ++i) g_std[i] = sde_partials_sum(&part[i], (size_t)LA, P);    // sde_std_finalise_kernel
  for (const std::vector<float>* v : {&var, &logp, &ratio, &sur, &tt, &g_mean, &g_lat, &g_std, &var_sample})
    std::fwrite(v->data(), 4, v->size(), stdout);
  std::fprintf(stderr, "C %d %d\n", R, P);
  return 0;
}
"""


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return compile_replay(tmp_path_factory.mktemp("sde_eval_math"), MAIN)


@pytest.fixture(scope="module")
def squash_programs(tmp_path_factory):
    """The replay of the sample and squashed heads (tests/test_sde_squash_math.py)."""
    from test_sde_squash_math import MAIN as SQUASH_MAIN
    return compile_replay(tmp_path_factory.mktemp("sde_squash_for_eval"), SQUASH_MAIN, variants=("plain",))


def replay(exe, n, L, A, case_inputs, clip=E.CLIP, ppo=True, with_g_lat=True):
    fields = (("var", (n, A)), ("logp", (n,)), ("ratio", (n,)), ("sur", (n,)), ("t", (n,)), ("g_mean", (n, A)),
              ("g_lat", (n, L)), ("g_std", (L, A)), ("var_sample", (n, A)))
    out, (out["R"], out["P"]) = run_replay(exe, ("eval", n, L, A, repr(float(clip)), int(ppo), int(with_g_lat)),
                                           case_inputs, [(name, np.float32, shape) for name, shape in fields])
    return out


@pytest.mark.parametrize("n,L,A", E.SHAPES, ids=lambda v: str(v))
def test_replay_against_the_float64_reference(programs, n, L, A):
    inp = E.inputs(n, L, A)
    got = replay(programs["plain"], n, L, A, inp)
    assert got["R"] == -(-n // 1024) and got["P"] == -(-n // got["R"]) and got["P"] <= 1024
    assert all(np.isfinite(got[k]).all() for k in ("var", "logp", "ratio", "sur", "g_mean", "g_lat", "g_std"))
    mean, act, adv = inp[0], inp[3], inp[5]
    if n >= 2:
        assert (got["var"][0] == 0).all()                                       # the zero latent row: s2 = 1e-6
        assert (act[-1] == mean[-1]).all() and (got["g_mean"][-1] == 0).all()    # the row with act == mean
    assert (got["sur"][adv == 0] == 0).all()
    err = E.errors(got, inp)
    print(f"host replay n {n} L {L} A {A}: " + " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert v < E.CEILING, (k, v)
        assert v <= BOUND[k], (k, v, BOUND[k])


@pytest.mark.parametrize("n,L,A", Q.SHAPES, ids=lambda v: str(v))
def test_var_is_the_sample_heads_bit_for_bit(programs, squash_programs, n, L, A):
    """Against the variance of the sample head's own accumulation (sde_accum) in this program, and against the
    existing replay of the sample and squashed heads (tests/test_sde_squash_math.py) on that test's inputs."""
    from test_sde_squash_math import replay as squash_replay
    inp = E.inputs(n, L, A)
    got = replay(programs["plain"], n, L, A, inp)
    assert (bits(got["var"]) == bits(got["var_sample"])).all()
    mean, lat, std, ga, gl = Q.inputs(n, L, A)
    want = squash_replay(squash_programs["plain"], n, L, A, (mean, lat, std, ga, gl))
    z = np.zeros(n, np.float32)
    mine = replay(programs["plain"], n, L, A, (mean, lat, std, want["gauss"], z, z, z, z), ppo=False)
    assert (bits(mine["var"]) == bits(want["var"])).all()


def test_branch_rule_is_torchs_gradient_on_the_directed_rows(programs):
    """g_logp = 0, g_sur = 1: the row's t is d sur / d logp.  torch-CPU float64 autograd of min(ratio adv,
    clamp(ratio) adv) at the program's ratio gives d sur / d ratio: adv where the rule passes the gradient (an
    unclipped row ties and its two halves add up to adv; the bounds of clamp are inclusive) and 0 where it does not.
    Where it passes, t is ratio * adv rounded once."""
    import torch
    n, L, A = 40, 8, 2
    mean, lat, std, act, old, adv, gl, gs = E.inputs(n, L, A)
    got = replay(programs["plain"], n, L, A, (mean, lat, std, act, old, adv, 0 * gl, 0 * gs + 1))
    r = torch.tensor(got["ratio"].astype(np.float64), requires_grad=True)
    a = torch.tensor(adv.astype(np.float64))
    torch.min(r * a, torch.clamp(r, 1.0 - E.CLIP, 1.0 + E.CLIP) * a).sum().backward()
    g = r.grad.numpy()
    assert set(np.unique(g / np.where(a.numpy() != 0, a.numpy(), 1.0))) <= {0.0, 1.0}
    passes = g != 0
    s1 = got["ratio"] * adv                                # float32
    assert s1.dtype == np.float32
    assert (got["t"][passes] == s1[passes]).all() and (got["t"][~passes] == 0).all()
    # the directed rows: clipped and passing, clipped and blocked, unclipped, zero advantage
    want = []
    for ratio, sign in E.DIRECTED:
        clipped = ratio < 1.0 - E.CLIP or ratio > 1.0 + E.CLIP
        blocked = clipped and ((ratio > 1.0 and sign > 0) or (ratio < 1.0 and sign < 0))
        want.append(sign != 0 and not blocked)
    assert passes[:15].tolist() == want
    assert (np.abs(got["ratio"][:15] / np.array([r for r, _ in E.DIRECTED]) - 1.0) < 1e-5).all()


def test_null_gradients_rows_alone_and_the_order_of_the_row_sum(programs):
    """g_logp = g_sur = 0 gives zero gradients; without the PPO arguments t = g_logp; without g_lat nothing is
    written to it and the other outputs keep their bits.  A row run on its own gives the whole's rows bit for bit,
    and the whole's g_std is the strands-and-tree sum of the rows' (n <= 1024: one row per partial), restated here
    in NumPy float32."""
    n, L, A = 40, 8, 2
    inp = E.inputs(n, L, A)
    mean, lat, std, act, old, adv, gl, gs = inp
    zero = replay(programs["plain"], n, L, A, (mean, lat, std, act, old, adv, 0 * gl, 0 * gs))
    assert not zero["g_mean"].any() and not zero["g_lat"].any() and not zero["g_std"].any()
    got = replay(programs["plain"], n, L, A, inp)
    assert (got["R"], got["P"]) == (1, n)
    plain = replay(programs["plain"], n, L, A, inp, ppo=False)
    assert (bits(plain["t"]) == bits(gl)).all() and (bits(plain["logp"]) == bits(got["logp"])).all()
    no_lat = replay(programs["plain"], n, L, A, inp, with_g_lat=False)
    assert (no_lat["g_lat"] == np.float32(-7.0e33)).all()
    assert all((bits(no_lat[k]) == bits(got[k])).all() for k in ("g_mean", "g_std", "sur", "ratio"))
    strands = [np.zeros((L, A), np.float32) for _ in range(16)]
    for e in range(n):
        one = replay(programs["plain"], 1, L, A, tuple(x if x is std else x[e:e + 1] for x in inp))
        for k in ("var", "logp", "ratio", "sur", "g_mean", "g_lat"):
            assert (bits(one[k]) == bits(got[k][e:e + 1])).all(), k
        strands[e % 16] = strands[e % 16] + one["g_std"]
    h = 1
    while h < 16:
        for i in range(0, 16, 2 * h):
            strands[i] = strands[i] + strands[i + h]
        h *= 2
    assert strands[0].dtype == np.float32 and (bits(strands[0]) == bits(got["g_std"])).all()


def test_replay_under_sanitizers(programs):
    for n, L, A in ((5, 260, 2), (1027, 8, 2), (1, 4, 1)):
        got = replay(programs["san"], n, L, A, E.inputs(n, L, A))
        assert np.isfinite(got["g_std"]).all()
        got = replay(programs["san"], n, L, A, E.inputs(n, L, A), ppo=False, with_g_lat=False)
        assert np.isfinite(got["g_std"]).all()


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_eval_calls_refuse_bad_arguments_without_gpu(lib):
    """Everything usv_sde_eval_forward / _backward can refuse before a HIP call is refused with USV_ERR_ARG and a
    message: a bad latent_dim, act_dim or reserved, rows <= 0, partial PPO arguments, a bad clip, a short or
    misaligned stride, NULL and misaligned buffers.  The struct's n is not the evaluation's."""
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    FWD = ("mean", "lat", "std", "act", "old", "adv", "logp", "sur", "ratio", "var")
    BWD = ("mean", "lat", "std", "act", "var", "ratio", "adv", "g_logp", "g_sur", "g_mean", "g_lat", "g_std", "scratch")

    def calls(s, word, which=(0, 1), rows=4, stride=8, g_stride=8, clip=0.2, **kw):
        sp = ctypes.byref(s) if s is not None else None
        a = {k: p for k in FWD + BWD}
        a.update(kw)
        fns = (lambda: lib.usv_sde_eval_forward(sp, rows, a["mean"], a["lat"], stride, a["std"], a["act"], a["old"],
                                                a["adv"], clip, a["logp"], a["sur"], a["ratio"], a["var"], None),
               lambda: lib.usv_sde_eval_backward(sp, rows, a["mean"], a["lat"], stride, a["std"], a["act"], a["var"],
                                                 a["ratio"], a["adv"], clip, a["g_logp"], a["g_sur"], a["g_mean"],
                                                 a["g_lat"], g_stride, a["g_std"], a["scratch"], None))
        for i in which:
            assert fns[i]() == -1, (word, i)
            assert word in lib.usv_last_error(), (word, i, lib.usv_last_error())

    calls(None, b"null usv_sde")
    for kw, word in ((dict(act_dim=0), b"act_dim"), (dict(act_dim=3), b"act_dim"), (dict(latent_dim=0), b"latent_dim"),
                     (dict(latent_dim=6), b"latent_dim"), (dict(latent_dim=4100), b"latent_dim"),
                     (dict(latent_dim=-4), b"latent_dim"), (dict(reserved=1), b"reserved")):
        calls(make_sde(**kw), word)
    for rows in (0, -1, -2 ** 31):
        calls(make_sde(), b"rows must be > 0", rows=rows)
    for stride in (7, 10, 4):
        calls(make_sde(), b"row stride", stride=stride)
        calls(make_sde(), b"g_lat row stride", which=(1,), g_stride=stride)
    # the PPO arguments come together
    for name in ("old", "adv", "sur", "ratio"):
        calls(make_sde(), b"all NULL or all set", which=(0,), **{name: None})
    calls(make_sde(), b"both NULL or both set", which=(1,), ratio=None)
    calls(make_sde(), b"both NULL or both set", which=(1,), adv=None)
    calls(make_sde(), b"g_sur needs ratio", which=(1,), ratio=None, adv=None)
    for clip in (-0.1, float("nan")):
        calls(make_sde(), b"clip must be >= 0", clip=clip)
    calls(make_sde(), b"null scratch", which=(1,), scratch=None)
    for name in ("mean", "lat", "std", "act", "logp"):
        calls(make_sde(), b"null buffer", which=(0,), **{name: None})
    for name in ("mean", "lat", "std", "act", "var", "g_mean", "g_std"):
        calls(make_sde(), b"null buffer", which=(1,), **{name: None})
    for name in FWD:
        calls(make_sde(), b"aligned", which=(0,), **{name: p + 2})
    for name in BWD:
        calls(make_sde(), b"aligned", which=(1,), **{name: p + 2})
    for name in ("lat", "g_lat", "scratch"):                # 4-B aligned is not enough for the 16-B accesses
        calls(make_sde(), b"aligned", which=(1,), **{name: p + 4})
        calls(make_sde(), b"aligned", which=(1,), **{name: p + 8})
    calls(make_sde(), b"aligned", which=(0,), lat=p + 4)
    # what may be absent is: the next refusal is the device check's (host memory).  n is not read.
    calls(make_sde(n=0), b"device pointer", which=(0,), old=None, adv=None, sur=None, ratio=None, var=None)
    calls(make_sde(n=-5), b"device pointer", which=(1,), ratio=None, adv=None, g_logp=None, g_sur=None, g_lat=None,
          g_stride=0)


def test_scratch_floats(lib):
    s = make_sde(n=1)
    for rows, P in ((1, 1), (1024, 1024), (1025, 513), (1027, 514), (65536, 1024)):
        for L, A in ((8, 2), (300, 2), (512, 1)):
            s = make_sde(n=1, latent_dim=L, act_dim=A)
            assert lib.usv_sde_eval_scratch_floats(ctypes.byref(s), rows) == P * L * A, (rows, L, A)
    assert lib.usv_sde_eval_scratch_floats(None, 4) == 0
    assert lib.usv_sde_eval_scratch_floats(ctypes.byref(make_sde()), 0) == 0
    assert lib.usv_sde_eval_scratch_floats(ctypes.byref(make_sde(latent_dim=6)), 4) == 0


def test_evaluate_is_exported_and_checks_its_arguments_first():
    import torch
    import gym_usv_amd
    from gym_usv_amd.sde import DeviceSDE, Evaluation
    assert gym_usv_amd.Evaluation is Evaluation
    assert Evaluation._fields == ("log_prob", "surrogate", "ratio")
    x = torch.zeros((4, 2))
    for kw in (dict(old_log_prob=x[:, 0]), dict(advantages=x[:, 0]), dict(clip_range=0.2),
               dict(old_log_prob=x[:, 0], advantages=x[:, 0]), dict(old_log_prob=x[:, 0], clip_range=0.2)):
        with pytest.raises(ValueError, match="come together"):
            DeviceSDE.evaluate(None, x, x, x, x, **kw)
