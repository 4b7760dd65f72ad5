"""The arithmetic of the fused gSDE head (gym-usv_amd/csrc/usv_sde_math.hpp) and the argument checks of
usv_sde_sample / usv_sde_weights, without a GPU.

usv_sde_math.hpp is plain C++: a stand-alone program that includes nothing else runs its Philox, its
element numbering, its uniforms and, lane by lane and through the reduction tree, the whole head on host
arrays.  The counter and element numbering, the (u1, u2) floats and the clip are compared with the NumPy
restatement of the definition (tests/sde_ref.py) bit for bit: no tolerance.  The host's Box-Muller is
libm's (the device's is the hardware's), so normals and sums are compared within the bounds the GPU test
uses as its ceiling."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import sde_ref as R
from sde_host import bits, compile_replay, load_lib, make_sde, run_replay

KAT = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        "d16cfe09 94fdcceb 5001e420 24126ea1"))
CEILING = 1e-5                                          # the GPU test's condition on each error

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "usv_sde_math.hpp"
using namespace usv;

// kat c0 c1 c2 c3 k0 k1 (hex)            -> stdout "o0 o1 o2 o3" (hex)
// head n L A seed gid0 epoch low0 low1 high0 high1; stdin: mean [n][A], lat [n][L], std [L][A] f32
//   -> stdout: per env and element (j, k): block u32, slot u32                     [n][L][A][2] u32
//              per env and block: the four words u32, then (u1, u2, u1', u2') f32  [n][L A / 4][8]
//              w [n][L][A] f32, act [n][A] f32, act_env [n][A] f32, logp [n] f32
int main(int argc, char** argv) {
  if (argc == 8 && !std::strcmp(argv[1], "kat")) {
    uint32_t v[6], o[4];
    for (int i = 0; i < 6; ++i) v[i] = (uint32_t)std::strtoul(argv[2 + i], nullptr, 16);
    sde_philox(v[0], v[1], v[2], v[3], v[4], v[5], o);
    std::printf("%08x %08x %08x %08x\n", o[0], o[1], o[2], o[3]);
    return 0;
  }
  if (argc != 12 || std::strcmp(argv[1], "head")) return 2;
  const int n = std::atoi(argv[2]), L = std::atoi(argv[3]), A = std::atoi(argv[4]);
  const uint64_t seed = std::strtoull(argv[5], nullptr, 10), gid0 = std::strtoull(argv[6], nullptr, 10);
  const uint32_t epoch = (uint32_t)std::strtoul(argv[7], nullptr, 10);
  const float low[2] = {(float)std::atof(argv[8]), (float)std::atof(argv[9])};
  const float high[2] = {(float)std::atof(argv[10]), (float)std::atof(argv[11])};
  if (!sde_latent_ok(L) || (A != 1 && A != 2) || n <= 0) return 4;
  std::vector<float> mean((size_t)n * A), lat((size_t)n * L), sd((size_t)L * A);
  if (std::fread(mean.data(), 4, mean.size(), stdin) != mean.size()) return 3;
  if (std::fread(lat.data(), 4, lat.size(), stdin) != lat.size()) return 3;
  if (std::fread(sd.data(), 4, sd.size(), stdin) != sd.size()) return 3;
  const int B = L * A / 4;
  std::vector<uint32_t> num((size_t)n * L * A * 2), words((size_t)n * B * 8);
  std::vector<float> w((size_t)n * L * A), act((size_t)n * A), env((size_t)n * A), logp(n);
  for (int e = 0; e < n; ++e) {
    const uint64_t gid = gid0 + (uint64_t)e;
    for (int b = 0; b < B; ++b) {                         // sde_weights_kernel, thread (e, b)
      uint32_t o[4];
      float z[4];
      sde_block(seed, gid, epoch, (uint32_t)b, o);
      sde_normals(o, z);
      uint32_t* const wd = &words[((size_t)e * B + b) * 8];
      const float u[4] = {sde_u1(o[0]), sde_u2(o[1]), sde_u1(o[2]), sde_u2(o[3])};
      std::memcpy(wd, o, 16);
      std::memcpy(wd + 4, u, 16);
      for (int q = 0; q < 4; ++q) w[(size_t)e * L * A + 4 * (size_t)b + q] = sde_weight(sd[4 * (size_t)b + q], z[q]);
    }
    float noise[2][kSdeLanes], var[2][kSdeLanes];
    for (int k = 0; k < 2; ++k)
      for (int l = 0; l < kSdeLanes; ++l) noise[k][l] = var[k][l] = 0.0f;
    for (int j = 0; j < L; ++j)                           // sde_sample_kernel: lane sde_lane(j), ascending j
      for (int k = 0; k < A; ++k) {
        const size_t at = ((size_t)e * L + j) * A + k;
        num[2 * at] = sde_block_of(j, k, A);
        num[2 * at + 1] = (uint32_t)sde_slot_of(j, k, A);
        uint32_t o[4];
        float z[4];
        sde_block(seed, gid, epoch, sde_block_of(j, k, A), o);
        sde_normals(o, z);
        const float s = sd[(size_t)j * A + k];
        sde_accum(lat[(size_t)e * L + j], s, sde_weight(s, z[sde_slot_of(j, k, A)]), noise[k][sde_lane(j)],
                  var[k][sde_lane(j)]);
      }
    float lp = 0.0f;
    for (int k = 0; k < A; ++k) {                         // lane 0's tail
      const float nz = sde_tree_sum(noise[k]), vr = sde_tree_sum(var[k]);
      const float m = mean[(size_t)e * A + k];
      const float a = sde_action(m, nz);
      act[(size_t)e * A + k] = a;
      env[(size_t)e * A + k] = sde_clip(a, low[k], high[k]);
      lp = lp + sde_logp_term(a, m, vr);
    }
    logp[e] = lp;
  }
  std::fwrite(num.data(), 4, num.size(), stdout);
  std::fwrite(words.data(), 4, words.size(), stdout);
  std::fwrite(w.data(), 4, w.size(), stdout);
  std::fwrite(act.data(), 4, act.size(), stdout);
  std::fwrite(env.data(), 4, env.size(), stdout);
  std::fwrite(logp.data(), 4, logp.size(), stdout);
  std::fprintf(stderr, "C %d %d %d %d\n", kSdeLanes, kSdePerLane, kSdePass, kSdeMaxLatent);
  return 0;
}
"""


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return compile_replay(tmp_path_factory.mktemp("sde_math"), MAIN)


def inputs(n, L, A, seed=0):
    """lat = relu(randn) as the ReLU body gives it, log_std around -2 +- 1, mean within +-2."""
    rng = np.random.default_rng(1000 * n + 10 * L + A + seed)
    lat = np.maximum(rng.standard_normal((n, L)), 0.0).astype(np.float32)
    std = np.exp(rng.uniform(-3.0, -1.0, (L, A))).astype(np.float32)
    mean = rng.uniform(-2.0, 2.0, (n, A)).astype(np.float32)
    if n >= 2:
        mean[0], mean[-1] = 50.0, -50.0                   # one row past each bound whatever the noise
    return mean, lat, std


LOW, HIGH = (0.0, -1.0), (1.0, 1.0)


def head(exe, n, L, A, seed, gid0, epoch, mean, lat, std, low=LOW, high=HIGH):
    out, out["consts"] = run_replay(
        exe, ("head", n, L, A, seed, gid0, epoch, *(repr(float(x)) for x in (*low, *high))), (mean, lat, std),
        (("num", np.uint32, (n, L, A, 2)), ("words", np.uint32, (n, L * A // 4, 8)), ("w", np.float32, (n, L, A)),
         ("act", np.float32, (n, A)), ("env", np.float32, (n, A)), ("logp", np.float32, (n,))))
    return out


def test_philox_known_answers(programs):
    for ctr, key, want in KAT:
        assert " ".join(f"{w:08x}" for w in R.philox(ctr, key)) == want
        p = subprocess.run([programs["plain"], "kat", *(f"{v:x}" for v in (*ctr, *key))], capture_output=True,
                           text=True, timeout=60)
        assert p.returncode == 0 and p.stdout.strip() == want, (ctr, key, p.stdout)


def check_numbering(exe, n, L, A, seed, gid0, epoch):
    mean, lat, std = inputs(n, L, A)
    got = head(exe, n, L, A, seed, gid0, epoch, mean, lat, std)
    key = f"n {n} L {L} A {A} seed {seed} gid0 {gid0} epoch {epoch}"
    assert got["consts"] == [64, 4, 256, 4096]
    B = L * A // 4
    i = np.arange(L * A).reshape(L, A)
    assert (got["num"][..., 0] == (i // 4)[None]).all() and (got["num"][..., 1] == (i % 4)[None]).all(), key
    for e in range(n):
        for b in range(B):
            words = R.block_words(seed, gid0 + e, epoch, b)
            assert tuple(int(x) for x in got["words"][e, b, :4]) == words, (key, e, b)
            assert (got["words"][e, b, 4:] == R.uniforms(words).view(np.uint32)).all(), (key, e, b)
    # u1 in (0, 1], u2 in [0, 1)
    u = got["words"][..., 4:].view(np.float32)
    assert (u[..., 0::2] > 0).all() and (u[..., 0::2] <= 1).all() and (u[..., 1::2] >= 0).all() and (u[..., 1::2] < 1).all()
    # the clip, bit for bit on the program's own actions, both bounds in use
    low, high = np.float32(LOW[:A]), np.float32(HIGH[:A])
    assert (bits(got["env"]) == bits(R.clip(got["act"], low, high))).all(), key
    if n >= 2:
        assert (got["act"] > high).any() and (got["act"] < low).any(), key
    return got, (mean, lat, std)


@pytest.mark.parametrize("A", (1, 2))
@pytest.mark.parametrize("L", (4, 256, 260))
def test_numbering_uniforms_and_clip_bit_for_bit(programs, L, A):
    check_numbering(programs["plain"], 5, L, A, seed=0x0123456789ABCDEF, gid0=7, epoch=3)


def test_gid_straddles_2_to_the_32(programs):
    got, _ = check_numbering(programs["plain"], 4, 8, 2, seed=5, gid0=2 ** 32 - 2, epoch=1)
    other, _ = check_numbering(programs["plain"], 4, 8, 2, seed=5, gid0=2 ** 64 - 2, epoch=1)    # and wraps at 2^64
    assert (got["words"][2] != other["words"][2]).any()
    # env 2 of this head is global env 2^32: counter word 1 = 1, word 0 = 0
    assert tuple(int(x) for x in got["words"][2, 0, :4]) == R.philox((0, 1, 1, 0), (5, 0))


def test_clip_edge_values(programs):
    """NaN stays NaN (torch.max(torch.min()) keeps it), infinities and exact bounds clip."""
    mean = np.array([[np.nan, 5.0], [np.inf, -np.inf], [1.0, -1.0], [0.0, 1.0]], np.float32)
    lat = np.zeros((4, 4), np.float32)
    std = np.ones((4, 2), np.float32)
    got = head(programs["plain"], 4, 4, 2, 1, 0, 0, mean, lat, std)
    assert (bits(got["act"]) == bits(mean)).all()                              # lat = 0: a == mean
    want = np.array([[np.nan, 1.0], [1.0, -1.0], [1.0, -1.0], [0.0, 1.0]], np.float32)
    assert (bits(got["env"]) == bits(want)).all()


@pytest.mark.parametrize("n,L,A", ((3, 4, 1), (5, 256, 2), (3, 260, 2), (2, 512, 1)))
def test_head_against_the_float64_reference(programs, n, L, A):
    """The host replay (libm transcendentals) against sde_ref in float64: each of the GPU test's three
    errors below the GPU test's ceiling; one-hot rows of the replay equal its own W bit for bit."""
    seed, gid0, epoch = 11, 3, 2
    got, (mean, lat, std) = check_numbering(programs["plain"], n, L, A, seed, gid0, epoch)
    ones = head(programs["plain"], n, L, A, seed, gid0, epoch, mean, lat, np.ones_like(std))
    z, r = R.normals(seed, gid0, epoch, n, L, A)
    ez = np.abs(ones["w"] - z) / np.maximum(1.0, r)
    a, scale, _ = R.sample(seed, gid0, epoch, mean, lat, std)
    ea = np.abs(got["act"] - a) / scale
    lp, lscale = R.logp_of(got["act"], mean, lat, std)
    el = np.abs(got["logp"] - lp) / lscale
    print(f"host replay n {n} L {L} A {A}: z {ez.max():.3e} a {ea.max():.3e} logp {el.max():.3e}")
    assert ez.max() < CEILING and ea.max() < CEILING and el.max() < CEILING
    j = L - 1
    hot = np.zeros_like(lat)
    hot[:, j] = 1.0
    oh = head(programs["plain"], n, L, A, seed, gid0, epoch, np.zeros_like(mean), hot, std)
    assert (bits(oh["act"]) == bits(got["w"][:, j, :])).all()


def test_replay_under_sanitizers(programs):
    check_numbering(programs["san"], 3, 260, 2, seed=9, gid0=2 ** 32 - 1, epoch=0xFFFFFFFF)
    check_numbering(programs["san"], 1, 4, 1, seed=0, gid0=0, epoch=0)


def setting_normals(seed, epoch):
    z, _ = R.normals(seed, 0, epoch, 64, 256, 2)
    return z


def test_reference_distribution():
    """The reference's own normals in the setting the GPU test reuses (seed 0, epoch 1, 64 envs, L = 256,
    A = 2: 32 768 normals): mean and variance z-scores within 3, KS p > 0.01 where scipy imports, and the
    correlations between the two action columns and between epochs 1 and 2 within 3 / sqrt(n)."""
    z1, z2 = setting_normals(0, 1), setting_normals(0, 2)
    n = z1.size
    assert n == 32768
    zm, zv = R.stats(z1)
    c_cols, c_ep = R.corr(z1[..., 0], z1[..., 1]), R.corr(z1, z2)
    print(f"reference: mean z {zm:.3f} var z {zv:.3f} corr cols {c_cols:.5f} epochs {c_ep:.5f} (n {n})")
    assert abs(zm) < 3 and abs(zv) < 3
    assert abs(c_cols) < 3 / math.sqrt(n) and abs(c_ep) < 3 / math.sqrt(n)     # n = all 32 768 normals, in both
    try:
        from scipy import stats as S
    except ImportError:
        return
    p = S.kstest(z1.ravel(), "norm").pvalue
    print(f"reference: KS p {p:.3f}")
    assert p > 0.01


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_sde_calls_refuse_bad_arguments_without_gpu(lib):
    """Everything usv_sde_sample / usv_sde_weights can refuse before a HIP call is refused with USV_ERR_ARG
    and a message (so also on a machine without a GPU)."""
    from gym_usv_amd import _lib
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    nan = float("nan")

    def calls(s, word, stride=8, which=(0, 1), mean=p, lat=p, std=p, act=p, env=p, logp=p, w=p):
        sp = ctypes.byref(s) if s is not None else None
        fns = (lambda: lib.usv_sde_sample(sp, 1, mean, lat, stride, std, act, env, logp, None),
               lambda: lib.usv_sde_weights(sp, 1, std, w, None))
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
    # bounds past act_dim are not looked at: the next refusal is the buffers'
    calls(make_sde(act_dim=1, low=(0.0, 5.0, 0, 0)), b"null buffer", std=None)
    calls(make_sde(), b"row stride", stride=7, which=(0,))
    calls(make_sde(), b"row stride", stride=10, which=(0,))
    calls(make_sde(), b"row stride", stride=4, which=(0,))
    for name in ("mean", "lat", "std", "act", "env", "logp"):
        calls(make_sde(), b"null buffer", which=(0,), **{name: None})
        calls(make_sde(), b"aligned", which=(0,), **{name: p + 2})
    calls(make_sde(), b"aligned", which=(0,), lat=p + 4)         # 4-B aligned is not enough for the latent rows
    calls(make_sde(), b"aligned", which=(0,), lat=p + 8)
    for name in ("std", "w"):
        calls(make_sde(), b"null buffer", which=(1,), **{name: None})
        calls(make_sde(), b"aligned", which=(1,), **{name: p + 1})
    calls(make_sde(n=2 ** 31 - 1, latent_dim=4096), b"blocks of 256", which=(1,))
    assert ctypes.sizeof(_lib.UsvSde) == 4 * 4 + 2 * 8 + 8 * 4


def test_device_sde_checks_its_arguments_first():
    """Bad shapes raise ValueError before the device is looked at; good ones then meet the no-CPU-fallback
    rule."""
    import torch
    import gym_usv_amd
    from gym_usv_amd.sde import DeviceSDE
    assert gym_usv_amd.DeviceSDE is DeviceSDE
    cpu = torch.device("cpu")
    for bad in ((0, 256, 2), (4, 6, 2), (4, 0, 2), (4, 4100, 2), (4, 256, 3), (4, 256, 0)):
        with pytest.raises(ValueError):
            DeviceSDE(*bad, cpu, 1, [0.0] * bad[2], [1.0] * bad[2])
    with pytest.raises(ValueError):
        DeviceSDE(4, 256, 2, cpu, 1, [0.0, 2.0], [1.0, 1.0])
    with pytest.raises(ValueError):
        DeviceSDE(4, 256, 2, cpu, 1, [0.0], [1.0])
    with pytest.raises(ValueError):
        DeviceSDE(4, 256, 2, cpu, -1, [0.0, -1.0], [1.0, 1.0])
    with pytest.raises(gym_usv_amd.UsvLibError):
        DeviceSDE(4, 256, 2, cpu, 1, [0.0, -1.0], [1.0, 1.0])
