"""The fused PPO loss without a GPU: the arithmetic of gym-usv_amd/csrc/usv_ppo_math.hpp through a stand-alone host
program built with AddressSanitizer and UBSan that replays the three kernels partial by partial.  The moments are
compared bit for bit with the float32 restatement (tests/ppo_loss_ref.py); every loss, statistic and gradient with the
float64 definition under the 1e-5 ceiling; the restatement, the NumPy definition and the scales with torch-CPU float64;
then the argument refusals of the new C entries and the Python ValueErrors that need no device."""
import ctypes
import subprocess

import numpy as np
import pytest

import ppo_loss_ref as R
import sac_loss_ref as S

MAIN = r"""
#include <cstdio>
#include <vector>
#include "usv_ppo_math.hpp"
using namespace usv;

// stdin, repeated until the end of the input: a header of 3 int64 (kind, n, flags), then
//   kind 0, the loss (flags: 1 normalize, 2 value clip, 4 entropy tensor): logp old adv values old_values returns
//           entropy [n] f32 each, clip clip_vf ent_coef vf_coef f32.
//           stdout: g_logp g_values g_entropy [n], the six outputs, mean std (0, 1 without normalisation)
//   kind 1, explained variance: values returns [n].   stdout: ev, the two means
static bool rd(std::vector<float>& v) { return std::fread(v.data(), 4, v.size(), stdin) == v.size(); }
static void wr(const std::vector<float>& v) { std::fwrite(v.data(), 4, v.size(), stdout); }

// One launch of a reduction kernel of NS sums: term(i, t) per row, each block's partial to its slot of the scratch,
// then what sac_finish leaves in the finishing thread.
template <int NS, class F>
static void launch(int64_t n, std::vector<float>& scratch, float (&s)[NS], F term) {
  const int64_t partials = sac_partials(n);
  float* const part = scratch.data() + kSacScratchHead;
  std::vector<float> col[NS];
  for (int64_t p = 0; p < partials; ++p) {
    const int64_t at = p * kSacPartialRows, count = n - at < kSacPartialRows ? n - at : kSacPartialRows;
    for (int k = 0; k < NS; ++k) col[k].assign(count, 0.0f);
    for (int64_t i = 0; i < count; ++i) {
      float t[NS];
      term(at + i, t);
      for (int k = 0; k < NS; ++k) col[k][i] = t[k];
    }
    for (int k = 0; k < NS; ++k) part[p * kPpoSums + k] = sac_partial_sum(col[k].data(), count);
  }
  for (int k = 0; k < NS; ++k) s[k] = partials == 1 ? part[k] : sac_partials_sum(part + k, kPpoSums, partials);
}

int main() {
  int64_t h[3];
  while (std::fread(h, 8, 3, stdin) == 3) {
    const int64_t n = h[1], fl = h[2];
    if (n < 1) return 4;
    std::vector<float> scratch(ppo_scratch_floats(n), 0.0f);
    if (h[0] == 0) {
      std::vector<float> logp(n), old(n), adv(n), v(n), old_v(n), ret(n), ent(n), gl(n), gv(n), ge(n);
      float sc[4];
      if (!rd(logp) || !rd(old) || !rd(adv) || !rd(v) || !rd(old_v) || !rd(ret) || !rd(ent) ||
          std::fread(sc, 4, 4, stdin) != 4) return 3;
      if (!ppo_range_ok(sc[0]) || !ppo_range_ok(sc[1])) return 5;
      const PpoForm f{(fl & 1) != 0 && n > 1, (fl & 2) != 0, (fl & 4) != 0, sc[0], sc[1], sc[2], sc[3]};
      float mom[2] = {0.0f, 1.0f};
      if (f.normalize) {
        float s[2];
        launch(n, scratch, s, [&](int64_t i, float (&t)[2]) { t[0] = adv[i]; t[1] = 0.0f; });
        mom[0] = ppo_mean(s[0], n);
        launch(n, scratch, s, [&](int64_t i, float (&t)[2]) { t[0] = ppo_sqdev(adv[i], mom[0]); t[1] = 0.0f; });
        mom[1] = ppo_std(s[0], n);
      }
      float s[kPpoSums], out[kPpoOuts];
      launch(n, scratch, s, [&](int64_t i, float (&t)[kPpoSums]) {
        ppo_row(f, logp[i], old[i], ppo_advantage(adv[i], f.normalize, mom[0], mom[1]), v[i], f.vclip ? old_v[i] : 0.0f,
                ret[i], f.with_entropy ? ent[i] : 0.0f, n, t, gl[i], gv[i]);
        ge[i] = ppo_entropy_grad(f.ent_coef, n);
      });
      ppo_finish(s, f.ent_coef, f.vf_coef, n, out);
      wr(gl), wr(gv), wr(ge);
      std::fwrite(out, 4, kPpoOuts, stdout);
      std::fwrite(mom, 4, 2, stdout);
    } else if (h[0] == 1) {
      std::vector<float> v(n), ret(n);
      if (!rd(v) || !rd(ret)) return 3;
      float s[2], out[3];
      launch(n, scratch, s, [&](int64_t i, float (&t)[2]) { t[0] = ret[i]; t[1] = ret[i] - v[i]; });
      out[1] = ppo_mean(s[0], n);
      out[2] = ppo_mean(s[1], n);
      launch(n, scratch, s, [&](int64_t i, float (&t)[2]) {
        t[0] = ppo_sqdev(ret[i], out[1]);
        t[1] = ppo_sqdev(ret[i] - v[i], out[2]);
      });
      out[0] = ppo_explained(s[0], s[1], n);
      std::fwrite(out, 4, 3, stdout);
    } else {
      return 6;
    }
  }
  std::fprintf(stderr, "sums %d outs %d scratch %zu %zu\n", kPpoSums, kPpoOuts, ppo_scratch_floats(1),
               ppo_scratch_floats(2 * kSacPartialRows + 1));
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program with AddressSanitizer + UBSan: a stand-alone host binary, run directly."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("ppo_loss_math")
    src, exe = d / "ppo.cpp", d / "ppo_san"
    src.write_text(MAIN)
    subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g", f"-I{CSRC}",
                    "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


def run(exe, records):
    """`records`: [(kind, n, flags, [arrays and scalars in the program's order], output floats)]; one run."""
    parts = []
    for kind, n, flags, items, _ in records:
        parts.append(np.array([kind, n, flags], np.int64))
        parts += [np.ascontiguousarray(x) for x in items]
    p = subprocess.run([exe], input=b"".join(x.tobytes() for x in parts), capture_output=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    assert p.stderr.decode().strip() == "sums 5 outs 6 scratch 9 19"
    out, at = [], 0
    for *_, count in records:
        out.append(np.frombuffer(p.stdout, np.float32, count, at))
        at += 4 * count
    assert at == len(p.stdout)
    return out


def loss_record(x, form, clip=R.CLIP, vf_coef=R.VF_COEF, ent_coef=R.ENT_COEF):
    B = len(x["logp"])
    flags = int(form["normalize"]) + 2 * (form["clip_vf"] is not None) + 4 * int(form["entropy"])
    items = [x[k] for k in ("logp", "old_logp", "adv", "values", "old_values", "returns", "entropy")]
    return (0, B, flags, items + [np.array([clip, form["clip_vf"] or 0.0, ent_coef, vf_coef], np.float32)], 3 * B + 8)


def unpack(got, B, form):
    """The program's (or the device's) outputs as reference()'s dict."""
    out = dict(zip(R.NAMES, got[3 * B:3 * B + 6]))
    out.update(g_logp=got[:B], g_values=got[B:2 * B])
    if form["entropy"]:
        out["g_entropy"] = got[2 * B:3 * B]
    if R.normalised(B, form):
        out["mean"], out["std"] = got[3 * B + 6], got[3 * B + 7]
    return out


def test_moments_equal_the_restatement_bitwise_and_the_rest_is_within_the_ceiling(program):
    cs = R.cases()
    worst = {}
    for (B, form, x), got in zip(cs, run(program, [loss_record(x, form) for _, form, x in cs])):
        assert R.margins_hold(x), B
        got = unpack(got, B, form)
        if R.normalised(B, form):
            assert S.same([got["mean"], got["std"]], R.moments32(x["adv"])), (B, form)
        else:
            assert "mean" not in got
        for k, v in R.errors(got, R.reference(x, form), R.scales(x, form)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("ppo loss errors of the host program:", {k: f"{v:.3e}" for k, v in sorted(worst.items())})
    assert set(worst) == set(R.NAMES) | {"mean", "std", "g_logp", "g_values", "g_entropy"}
    assert all(v < S.CEILING for v in worst.values()), worst


def test_explained_variance_equals_the_restatement_bitwise(program):
    xs = [R.inputs(B, seed=3) for B in R.ROWS]
    xs.append(dict(R.inputs(257), returns=np.full(257, 1.5, np.float32)))        # constant returns: NaN
    for x, got in zip(xs, run(program, [(1, len(x["values"]), 0, [x["values"], x["returns"]], 3) for x in xs])):
        want = R.explained32(x["values"], x["returns"])
        assert S.same(got[:1], [want]), (len(x["values"]), got, want)
        ref = R.explained64(x["values"], x["returns"])
        if math_isnan(ref):
            assert np.isnan(got[0])
        else:
            assert abs(float(got[0]) - ref) / R.explained_scale(x["values"], x["returns"]) < S.CEILING
    assert np.isnan(run(program, [(1, 1, 0, [np.float32([2.0]), np.float32([3.0])], 3)])[0][0])


def math_isnan(v):
    return v != v


def test_directed_rows_in_the_host_program(program):
    """The exact properties of the directed rows (normalisation off): the count of clipped rows, torch.min's and
    torch.clamp's ties, the value clamp's inclusive bounds."""
    B = 45
    x, ratio, sign = R.directed(B)
    form = dict(normalize=False, clip_vf=R.CLIP_VF, entropy=True)
    got, = run(program, [loss_record(x, form)])
    got = unpack(got, B, form)
    R.check_directed(got, x, ratio, sign, B)


def test_the_restatement_and_the_definition_against_torch_float64():
    """moments32 / explained32 against float64 under the ceiling with the documented scales, for advantage means of 0, 5
    and 100 standard deviations; the NumPy definition's forward against torch's."""
    worst = 0.0
    for B in R.ROWS[1:]:
        for m in (0.0, 5.0, 100.0):
            x = R.inputs(B, seed=int(m), adv_mean=m)
            ref, sc = R.define(x, R.FULL_FORM), R.scales(x, R.FULL_FORM)
            mean, std = R.moments32(x["adv"])
            worst = max(worst, abs(mean - ref["mean"]) / sc["mean"], abs(std - ref["std"]) / sc["std"])
        ev = R.explained32(x["values"], x["returns"])
        worst = max(worst, abs(float(ev) - R.explained64(x["values"], x["returns"])) / R.explained_scale(x["values"], x["returns"]))
    print("moments32 / explained32 against float64:", worst)
    assert worst < 2e-7
    for form in R.FORMS:
        for B in (1, 257):
            x = R.inputs(B, seed=5)
            ref, t = R.define(x, form), R.torch_define(x, form)
            for k in R.NAMES:
                assert abs(ref[k] - t[k]) <= 1e-12 * max(1.0, abs(t[k])), (form, B, k)
            if not form["entropy"]:
                assert (t["g_entropy"] == 0).all()


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_entries_refuse_bad_arguments_without_gpu(lib):
    """Everything the new entries can refuse before a HIP call is refused with USV_ERR_ARG and a message."""
    from gym_usv_amd import _lib
    assert _lib.ABI_VERSION == 5 == lib.usv_abi_version()
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16

    def refused(rc, word):
        assert rc == -1 and word in lib.usv_last_error(), (word, rc, lib.usv_last_error())

    assert [lib.usv_ppo_scratch_floats(r) for r in (-1, 0, 1, S.P, S.P + 1, 65 * S.P + 1)] == [0, 0, 9, 9, 14, 334]

    def loss(word, rows=5, req=(p,) * 5, old_values=p, entropy=p, clip=0.2, clip_vf=0.25, moments=p, out=p,
             g=(p, p, p), scratch=p):
        logp, old_logp, adv, values, returns = req
        refused(lib.usv_ppo_loss(rows, logp, old_logp, adv, values, old_values, returns, entropy, 1, clip, clip_vf, 0.0,
                                 0.5, moments, out, *g, scratch, None), word)

    for rows in (0, -4):
        loss(b"rows must be >= 1", rows=rows)
    for bad in (-0.1, float("nan"), float("inf")):
        loss(b"clip must be finite and >= 0", clip=bad)
        loss(b"clip_vf must be finite and >= 0", clip_vf=bad)
    loss(b"come together", old_values=None)                 # a clip_vf without old_values
    loss(b"come together", old_values=None, clip_vf=float("nan"))
    loss(b"g_entropy needs entropy", entropy=None)
    loss(b"null buffer", scratch=None)
    loss(b"not 16-B aligned", scratch=p + 4)
    loss(b"null buffer", moments=None)
    loss(b"null buffer", out=None)
    for i in range(5):
        loss(b"null buffer", req=tuple(None if j == i else p for j in range(5)))
        loss(b"not 4-B aligned", req=tuple(p + 2 if j == i else p for j in range(5)))
    for i in range(3):
        loss(b"not 4-B aligned", g=tuple(p + 1 if j == i else p for j in range(3)))
    loss(b"not 4-B aligned", old_values=p + 2)
    loss(b"not 4-B aligned", entropy=p + 2)

    def ev(word, rows=5, values=p, returns=p, out=p, scratch=p):
        refused(lib.usv_ppo_explained_variance(rows, values, returns, out, scratch, None), word)

    ev(b"rows must be >= 1", rows=0)
    ev(b"null buffer", values=None)
    ev(b"null buffer", returns=None)
    ev(b"null buffer", out=None)
    ev(b"null buffer", scratch=None)
    ev(b"not 16-B aligned", scratch=p + 8)
    ev(b"not 4-B aligned", out=p + 2)


def test_python_checks_need_no_device():
    import torch
    import gym_usv_amd
    from gym_usv_amd import ppo
    assert gym_usv_amd.DevicePPOLoss is ppo.DevicePPOLoss and gym_usv_amd.PPOLoss is ppo.PPOLoss
    assert gym_usv_amd.PPOLoss._fields == R.NAMES
    with pytest.raises(gym_usv_amd.UsvLibError):
        ppo.DevicePPOLoss(torch.device("cpu"))
    rows, grad = torch.zeros(4), torch.zeros(4, requires_grad=True)
    for a in ((0.2, 0.5, 0.0, rows, None), (0.2, 0.5, 0.0, None, 0.25), (-0.2, 0.5, 0.0, None, None),
              (float("nan"), 0.5, 0.0, None, None), (float("inf"), 0.5, 0.0, None, None), (0.2, 0.5, 0.0, rows, -1.0),
              (0.2, 0.5, 0.0, rows, float("nan")), (0.2, 0.5, 0.0, None, None, (rows, grad))):
        with pytest.raises(ValueError):
            ppo.check_loss_args(*a)
    assert ppo.check_loss_args(0.2, 1, 0, None, None, (rows,)) == (0.2, 0.0, 1.0, 0.0)
    assert ppo.check_loss_args(0, 0.5, 0.01, rows, 0.25) == (0.0, 0.25, 0.5, 0.01)
