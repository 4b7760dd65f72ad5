"""The CAPS regulariser without a GPU: the arithmetic of gym-usv_amd/csrc/usv_caps_math.hpp through a stand-alone host
program built with AddressSanitizer and UBSan and run directly, compared with the NumPy restatement
(tests/caps_ref.py) bit for bit where squash = 0; with squash = 1 (the host's tanhf is libm's) against torch-CPU
float64 autograd of the definition under the ceiling of 1e-4, on inputs whose rows keep both distances at least 0.05
in action space (caps_ref.floored_inputs says why); the host-side noise against sde_ref's normals; the argument
refusals of the two C entries; and the Python ValueErrors that need no device."""
import ctypes
import subprocess

import numpy as np
import pytest

import caps_ref as C
import sac_loss_ref as S

MAIN = r"""
#include <cstdio>
#include <vector>
#include "usv_caps_math.hpp"
using namespace usv;

// stdin, repeated until the end of the input: a header of 4 int64 (kind, B, width, flags), then
//   kind 0, loss (width = A; flags: 1 squash): mean mean_next mean_near [B][A] f32, lambda_t lambda_s f32.
//           stdout: g_mean g_next g_near [B][A], loss temporal spatial
//   kind 1, perturbation (width = W): seed epoch int64, eps f32, obs [B][W] f32.   stdout: out [B][W]
static bool rd(std::vector<float>& v) { return std::fread(v.data(), 4, v.size(), stdin) == v.size(); }
static void wr(const std::vector<float>& v) { std::fwrite(v.data(), 4, v.size(), stdout); }

template <int A>
static void rows(int64_t B, bool squash, const float* m, const float* mn, const float* mr, float lt, float ls, float* nT,
                 float* nS, float* gm, float* gn, float* gr) {
  for (int64_t i = 0; i < B; ++i) {
    float a[A], b[A], c[A], x[A], y[A], z[A];
    for (int k = 0; k < A; ++k) a[k] = m[i * A + k], b[k] = mn[i * A + k], c[k] = mr[i * A + k];
    caps_row<A>(a, b, c, squash, lt, ls, B, nT[i], nS[i], true, x, y, z);
    for (int k = 0; k < A; ++k) gm[i * A + k] = x[k], gn[i * A + k] = y[k], gr[i * A + k] = z[k];
  }
}

int main() {
  int64_t h[4];
  while (std::fread(h, 8, 4, stdin) == 4) {
    const int64_t B = h[1], W = h[2], fl = h[3];
    if (B < 1 || W < 1) return 4;
    const size_t n = (size_t)B * (size_t)W;
    if (h[0] == 0) {
      if (!caps_act_ok(W)) return 4;
      std::vector<float> m(n), mn(n), mr(n), gm(n), gn(n), gr(n), nT(B), nS(B);
      float sc[2];
      if (!rd(m) || !rd(mn) || !rd(mr) || std::fread(sc, 4, 2, stdin) != 2) return 3;
      if (!caps_weight_ok(sc[0]) || !caps_weight_ok(sc[1])) return 5;
#define ROWS(A) case A: rows<A>(B, (fl & 1) != 0, m.data(), mn.data(), mr.data(), sc[0], sc[1], nT.data(), nS.data(), \
                                gm.data(), gn.data(), gr.data()); break;
      switch (W) { ROWS(1) ROWS(2) ROWS(3) ROWS(4) ROWS(5) ROWS(6) ROWS(7) ROWS(8) }
      float out[3];
      caps_loss(sac_sum(nT.data(), B), sac_sum(nS.data(), B), sc[0], sc[1], B, out);
      wr(gm), wr(gn), wr(gr);
      std::fwrite(out, 4, 3, stdout);
    } else if (h[0] == 1) {
      int64_t key[2];
      float eps;
      std::vector<float> obs(n), out(n);
      if (std::fread(key, 8, 2, stdin) != 2 || std::fread(&eps, 4, 1, stdin) != 1 || !rd(obs)) return 3;
      if (!caps_weight_ok(eps)) return 5;
      for (int64_t r = 0; r < B; ++r)
        for (int64_t b = 0; b < caps_row_blocks(W); ++b) {          // caps_perturb_kernel, thread (r, b)
          float z[4];
          caps_block_normals((uint64_t)key[0], (uint64_t)r, (uint32_t)key[1], (uint32_t)b, z);
          for (int q = 0; q < 4 && 4 * b + q < W; ++q) out[r * W + 4 * b + q] = caps_near(obs[r * W + 4 * b + q], eps, z[q]);
        }
      wr(out);
    } else {
      return 6;
    }
  }
  std::fprintf(stderr, "A %d ok %d %d %d %d\n", kCapsMaxAct, (int)caps_weight_ok(-0.5f), (int)caps_weight_ok(0.0f),
               (int)caps_weight_ok(INFINITY), (int)caps_weight_ok(NAN));
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program with AddressSanitizer + UBSan: a stand-alone host binary, run directly."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("caps_math")
    src, exe = d / "caps.cpp", d / "caps_san"
    src.write_text(MAIN)
    subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g", f"-I{CSRC}",
                    "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


def run(exe, records):
    """`records`: [(kind, B, width, flags, [arrays and scalars in the program's order], output floats)]; one run."""
    parts = []
    for kind, B, W, flags, items, _ in records:
        parts.append(np.array([kind, B, W, flags], np.int64))
        parts += [np.ascontiguousarray(x) for x in items]
    p = subprocess.run([exe], input=b"".join(x.tobytes() for x in parts), capture_output=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    assert p.stderr.decode().strip() == "A 8 ok 0 1 0 0"
    out, at = [], 0
    for *_, count in records:
        out.append(np.frombuffer(p.stdout, np.float32, count, at))
        at += 4 * count
    assert at == len(p.stdout)
    return out


def loss_record(x, lambda_t, lambda_s, squash):
    B, A = x[0].shape
    return (0, B, A, int(squash), [*x, np.array([lambda_t, lambda_s], np.float32)], 3 * B * A + 3)


def split(got, B, A):
    n = B * A
    out = {k: got[i * n:(i + 1) * n].reshape(B, A) for i, k in enumerate(("g_mean", "g_next", "g_near"))}
    out.update(loss=got[3 * n], temporal=got[3 * n + 1], spatial=got[3 * n + 2])
    return out


def noise_record(B, W, seed, epoch, eps, obs):
    return (1, B, W, 0, [np.array([seed, epoch], np.int64), np.array([eps], np.float32), obs], B * W)


def test_the_loss_equals_the_restatement_bitwise(program):
    cases = [(B, A, 10.0, 5.0 if B != 63 else 0.0) for B in C.ROWS for A in C.ACTS] + [(1025, 2, 0.0, 5.0)]
    xs = [C.inputs(B, A, seed=1) for B, A, _, _ in cases]
    got = run(program, [loss_record(x, lt, ls, False) for x, (_, _, lt, ls) in zip(xs, cases)])
    for (B, A, lt, ls), x, g in zip(cases, xs, got):
        want, g = C.loss(*x, lt, ls, False), split(g, B, A)
        for k, w in want.items():
            assert S.same(g[k], w), (B, A, lt, ls, k)
        # rows whose mean_next is mean bit for bit: exact zeros in g_next and no temporal part in g_mean
        assert (x[1][::5] == x[0][::5]).all() and (g["g_next"][::5] == 0).all()
        assert (g["g_mean"][::5] == -g["g_near"][::5]).all()
        if B > 2:                                          # and one whose mean_near is: no spatial part
            assert (g["g_near"][2] == 0).all() and (g["g_mean"][2] == -g["g_next"][2]).all()
        if lt == 0.0:
            assert (g["g_next"] == 0).all() and g["loss"] == np.float32(ls) * g["spatial"] and g["temporal"] > 0
        assert np.isfinite(g["loss"]) and g["loss"] > 0


def test_a_nan_row_gives_nan_out(program):
    for B, A in ((5, 2), (S.P + 1, 3)):
        x = C.inputs(B, A, nan_row=True)
        g = split(run(program, [loss_record(x, 10.0, 5.0, False)])[0], B, A)
        want = C.loss(*x, 10.0, 5.0, False)
        for k, w in want.items():
            assert S.same(g[k], w), (B, A, k)
        assert np.isnan(g["loss"]) and np.isnan(g["spatial"]) and not np.isnan(g["temporal"])
        assert np.isnan(g["g_near"][B // 2]).all() and np.isnan(g["g_mean"][B // 2]).all()
        assert not np.isnan(g["g_next"]).any() and np.isnan(g["g_near"]).sum() == A


def test_squashed_loss_against_float64_autograd(program):
    """libm's tanhf on the host and NumPy's in the restatement: both within the ceiling of the float64 definition,
    on rows whose two distances are at least caps_ref.FLOOR in action space."""
    cases = [(B, A) for B in C.ROWS for A in C.ACTS]
    xs = [C.floored_inputs(B, A, seed=2) for B, A in cases]
    got = run(program, [loss_record(x, 10.0, 5.0, True) for x in xs])
    worst = {"host": {}, "restatement": {}}
    for (B, A), x, g in zip(cases, xs, got):
        ref = C.torch_loss(*x, 10.0, 5.0, True)
        for who, val in (("host", split(g, B, A)), ("restatement", C.loss(*x, 10.0, 5.0, True))):
            for k, v in C.errors(val, ref, 10.0, 5.0).items():
                worst[who][k] = max(worst[who].get(k, 0.0), v)
    print("caps squash errors:", {w: {k: f"{v:.3e}" for k, v in e.items()} for w, e in worst.items()})
    for e in worst.values():
        assert len(e) == 6 and all(v < C.CEILING for v in e.values()), worst
    # squash = 0 on the same inputs: the restatement against the definition
    for (B, A), x in zip(cases[::5], xs[::5]):
        e = C.errors(C.loss(*x, 10.0, 5.0, False), C.torch_loss(*x, 10.0, 5.0, False), 10.0, 5.0)
        assert all(v < C.CEILING for v in e.values()), (B, A, e)


def test_the_noise_is_the_counter_layout(program):
    seed, epoch = 0x0123456789ABCDE, 3
    shapes = ((3, 715), (9, 5), (6, 1), (2, 8))
    zero = [np.zeros(s, np.float32) for s in shapes]
    got = run(program, [noise_record(B, W, seed, epoch, 1.0, o) for (B, W), o in zip(shapes, zero)])
    for (B, W), g in zip(shapes, got):
        z, r = C.normals(seed, epoch, B, W)
        err = np.abs(g.reshape(B, W) - z) / np.maximum(1.0, r)       # test_sde_math.py's bound of the host's Box-Muller
        print(f"host noise [{B}, {W}]: {err.max():.3e}")
        assert err.max() < 1e-5
    # out = obs + (eps z), each operation rounded on its own
    rng = np.random.default_rng(5)
    obs = rng.standard_normal((3, 715)).astype(np.float32)
    near, more, other = run(program, [noise_record(3, 715, seed, epoch, 0.1, obs),
                                      noise_record(5, 715, seed, epoch, 0.1, np.concatenate((obs, obs[:2]))),
                                      noise_record(3, 715, seed, epoch + 1, 0.1, obs)])
    assert S.same(near, (obs + np.float32(0.1) * got[0].reshape(3, 715)).reshape(-1))
    assert S.same(more[:3 * 715], near)                              # rows [0, 3) of a 5-row call
    assert (other != near).mean() > 0.99                             # another epoch
    a, b = near.reshape(3, 715), more.reshape(5, 715)
    assert (b[3] - obs[0] != a[0] - obs[0]).mean() > 0.99            # another row, the same obs
    same, = run(program, [noise_record(3, 715, seed, epoch, 0.0, obs)])
    assert (same.reshape(3, 715) == obs).all()


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_entries_refuse_bad_arguments_without_gpu(lib):
    """Everything the two entries can refuse before a HIP call is refused with USV_ERR_ARG and its own message."""
    from gym_usv_amd import _lib
    assert _lib.ABI_VERSION == 5 == lib.usv_abi_version()
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    bad = (-1e-9, float("nan"), float("inf"), -float("inf"))

    def refused(rc, word):
        assert rc == -1 and word in lib.usv_last_error(), (word, rc, lib.usv_last_error())

    def perturb(word, rows=4, width=5, obs=p, out=p, eps=0.1):
        refused(lib.usv_caps_perturb(rows, width, obs, out, eps, 7, 1, None), word)

    for rows in (0, -3):
        perturb(b"rows must be >= 1", rows=rows)
    for width in (0, -1):
        perturb(b"width must be >= 1", width=width)
    perturb(b"rows * width is above 2^31 - 1", rows=1 << 16, width=1 << 15)
    perturb(b"rows * width is above 2^31 - 1", rows=2 ** 31 - 1, width=2 ** 31 - 1)
    for eps in bad:
        perturb(b"eps must be finite and >= 0", eps=eps)
    perturb(b"usv_caps: null buffer", obs=None)
    perturb(b"usv_caps: null buffer", out=None)
    perturb(b"not 4-B aligned", obs=p + 2)
    perturb(b"not 4-B aligned", out=p + 1)

    def loss(word, rows=4, A=2, req=(p,) * 4, lt=10.0, ls=5.0, g=(p, p, p), scratch=p):
        mean, mean_next, mean_near, out3 = req
        refused(lib.usv_caps_loss(rows, A, 1, mean, mean_next, mean_near, lt, ls, out3, *g, scratch, None), word)

    for rows in (0, -3):
        loss(b"rows must be >= 1", rows=rows)
    for A in (0, -1, 9):
        loss(b"act_dim must be in [1, 8]", A=A)
    loss(b"rows * act_dim is above 2^31 - 1", rows=2 ** 31 - 1, A=2)
    for w in bad:
        loss(b"lambda_t must be finite and >= 0", lt=w)
        loss(b"lambda_s must be finite and >= 0", ls=w)
    loss(b"usv_caps: null buffer", scratch=None)
    loss(b"not 16-B aligned", scratch=p + 4)
    for i in range(4):
        loss(b"usv_caps: null buffer", req=tuple(None if j == i else p for j in range(4)))
        loss(b"not 4-B aligned", req=tuple(p + 2 if j == i else p for j in range(4)))
    for i in range(3):
        loss(b"not 4-B aligned", g=tuple(p + 2 if j == i else None for j in range(3)))


def test_python_checks_need_no_device():
    import torch
    import gym_usv_amd
    from gym_usv_amd import caps
    assert gym_usv_amd.DeviceCAPS is caps.DeviceCAPS and gym_usv_amd.SmoothLoss is caps.SmoothLoss
    assert gym_usv_amd.SmoothLoss._fields == ("loss", "temporal", "spatial")
    with pytest.raises(gym_usv_amd.UsvLibError):          # well-formed, but not on a GPU: no CPU fallback
        caps.DeviceCAPS(torch.device("cpu"), 1)
    for kw in (dict(lambda_t=-1.0), dict(lambda_s=float("nan")), dict(eps_s=float("inf")), dict(eps_s=-0.1),
               dict(lambda_t="much"), dict(lambda_s=None)):
        with pytest.raises(ValueError):
            caps.DeviceCAPS(torch.device("cpu"), 1, **kw)
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            caps.DeviceCAPS(torch.device("cpu"), seed)
    cpu = torch.device("cpu")
    m = torch.zeros(4, 2)
    assert caps.check_means(m, m.clone(), m.clone(), cpu) == (4, 2)
    assert caps.check_means(torch.zeros(1, 8), torch.zeros(1, 8), torch.zeros(1, 8), cpu) == (1, 8)
    for a in ((m.double(), m, m), (m, m.double(), m), (m, m, torch.zeros(4, 2, dtype=torch.float16)),
              (torch.zeros(8), torch.zeros(8), torch.zeros(8)), (m, torch.zeros(4, 3), m), (m, m, torch.zeros(5, 2)),
              (m, m, torch.zeros(4, 2, 1)), (torch.zeros(0, 2),) * 3, (torch.zeros(4, 9),) * 3, (torch.zeros(4, 0),) * 3,
              (m, m, m.numpy())):
        with pytest.raises(ValueError):
            caps.check_means(*a, cpu)
    with pytest.raises(ValueError):                       # another device than the object's
        caps.check_means(m, m, m, torch.device("cuda", 0))
