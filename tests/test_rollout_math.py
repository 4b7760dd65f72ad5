"""The arithmetic and the slot numbering of the device rollout buffer
(gym-usv_amd/csrc/usv_rollout_math.hpp) and the argument checks of usv_rollout_*, without a GPU.

usv_rollout_math.hpp is plain C++: a stand-alone program that includes nothing else replays scripted
[T][n] inputs through the kernels' work split (chunk counts -> prefix over chunks -> rank within the
chunk) and their GAE loop, on host arrays.  adv, ret and term_slot are compared with SB3's RolloutBuffer
restated in NumPy float32 (tests/rollout_ref.py) bit for bit: no tolerance.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import rollout_ref as R

GAMMA, LAM = 0.99, 0.95
TS = (1, 2, 5, 33)
NS = (1, 63, 64, 65, 257)

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "usv_rollout_math.hpp"
using namespace usv;

// argv: T n cap gamma gae_lambda; stdin: rew [T][n] f32, val [T][n] f32, term [T][n] u8, trunc [T][n] u8,
// start0 [n] u8, last_val [n] f32, term_val [cap] f32.  stdout: adv [T][n] f32, ret [T][n] f32,
// term_slot [T][n] i32, (stored, overflow) i32, start [T + 1][n] u8 (after the gae's carry).
// stderr: "C block max_chunks chunks chunk_envs".
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int T = std::atoi(argv[1]);
  const int64_t n = std::atoll(argv[2]);
  const int cap = std::atoi(argv[3]);
  const double gamma = std::atof(argv[4]), lam = std::atof(argv[5]);
  const size_t M = (size_t)T * n;
  std::vector<float> rew(M), val(M), last(n), tval(cap > 0 ? cap : 1), adv(M), ret(M);
  std::vector<unsigned char> term(M), trunc(M), start((size_t)(T + 1) * n);
  std::vector<int32_t> slot(M);
  if (std::fread(rew.data(), 4, M, stdin) != M || std::fread(val.data(), 4, M, stdin) != M) return 3;
  if (std::fread(term.data(), 1, M, stdin) != M || std::fread(trunc.data(), 1, M, stdin) != M) return 3;
  if (std::fread(start.data(), 1, n, stdin) != (size_t)n || std::fread(last.data(), 4, n, stdin) != (size_t)n) return 3;
  if (cap > 0 && std::fread(tval.data(), 4, cap, stdin) != (size_t)cap) return 3;
  const int P = ro_num_chunks(n), R = ro_chunk_envs(n);
  int64_t totals[2] = {0, 0};
  int32_t count[2] = {0, 0};
  for (int t = 0; t < T; ++t) {                           // usv_rollout_put_step
    const unsigned char* tm = &term[(size_t)t * n];
    const unsigned char* tr = &trunc[(size_t)t * n];
    std::vector<int> counts(P, 0);                        // rollout_count_kernel
    for (int b = 0; b < P; ++b)
      for (int64_t e = (int64_t)b * R; e < (int64_t)(b + 1) * R && e < n; ++e) counts[b] += ro_bootstraps(tm[e], tr[e]);
    const int64_t base = t == 0 ? 0 : totals[t & 1];      // rollout_step_kernel
    int64_t total = 0;
    for (int b = 0; b < P; ++b) total += counts[b];
    for (int b = 0; b < P; ++b) {
      int64_t before = 0;
      for (int p = 0; p < b; ++p) before += counts[p];
      int rank = 0;
      for (int64_t e = (int64_t)b * R; e < (int64_t)(b + 1) * R && e < n; ++e) {
        const bool bs = ro_bootstraps(tm[e], tr[e]);
        slot[(size_t)t * n + e] = bs ? ro_slot(base, before, rank, cap) : -1;
        rank += bs;
        start[(size_t)(t + 1) * n + e] = (tm[e] | tr[e]) != 0;
      }
    }
    totals[(t + 1) & 1] = base + total;
    count[0] = ro_stored(base + total, cap);
    count[1] = ro_overflow(base + total, cap);
  }
  const float g32 = ro_g32(gamma), gl32 = ro_gl32(gamma, lam);
  for (int64_t e = 0; e < n; ++e) {                       // rollout_gae_kernel, lane e
    float nv = last[e], gae = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
      const size_t at = (size_t)t * n + e;
      float r = rew[at];
      if ((uint32_t)slot[at] < (uint32_t)cap) r = ro_bootstrap(r, g32, tval[slot[at]]);
      ret[at] = ro_gae_step(r, val[at], nv, start[at + n], g32, gl32, gae);
      adv[at] = gae;
      nv = val[at];
    }
    start[e] = start[(size_t)T * n + e];
  }
  std::fwrite(adv.data(), 4, M, stdout);
  std::fwrite(ret.data(), 4, M, stdout);
  std::fwrite(slot.data(), 4, M, stdout);
  std::fwrite(count, 4, 2, stdout);
  std::fwrite(start.data(), 1, start.size(), stdout);
  std::fprintf(stderr, "C %d %d %d %d\n", kRoBlock, kRoMaxChunks, P, R);
  return 0;
}
"""


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """The replay program, plain (-O3 for a target with FMA, where the compiler would contract) and with
    AddressSanitizer + UBSan (both stand-alone host binaries)."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("rollout_math")
    src = d / "replay.cpp"
    src.write_text(MAIN)
    out = {}
    import platform
    # -mfma: an x86-64 build contracts a * b + c only when the target has FMA instructions, so without it
    # the host could not show a contraction that usv_rollout_math.hpp failed to switch off
    fma = ["-mfma"] if platform.machine() in ("x86_64", "AMD64") else []
    for name, flags in (("plain", ["-O3", *fma]),
                        ("san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / f"replay_{name}"
        subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", *flags, f"-I{CSRC}", "-o", str(exe), str(src)],
                       check=True)
        out[name] = str(exe)
    return out


def replay(exe, sc, n, T, cap, term_val, start0):
    data = b"".join(np.ascontiguousarray(x).tobytes() for x in (
        sc["rew"].astype(np.float32), sc["val"], sc["term"].astype(np.uint8), sc["trunc"].astype(np.uint8),
        start0.astype(np.uint8), sc["last_val"], term_val.astype(np.float32)))
    p = subprocess.run([exe, str(T), str(n), str(cap), repr(GAMMA), repr(LAM)], input=data, capture_output=True,
                       timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    consts = [int(x) for x in p.stderr.decode().split("C ", 1)[1].split()]
    M, o = T * n, p.stdout
    return dict(adv=np.frombuffer(o, np.float32, M, 0).reshape(T, n),
                ret=np.frombuffer(o, np.float32, M, 4 * M).reshape(T, n),
                term_slot=np.frombuffer(o, np.int32, M, 8 * M).reshape(T, n),
                count=np.frombuffer(o, np.int32, 2, 12 * M),
                start=np.frombuffer(o, np.uint8, (T + 1) * n, 12 * M + 8).reshape(T + 1, n)), consts


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def check(exe, n, T, pattern="random", cap=None, stats=None):
    W, A = 3, 1
    sc = R.script(n, T, W, A, pattern)
    ref = R.run(sc, n, T, W, A, term_cap=cap, gamma=GAMMA, gae_lambda=LAM, stats=stats)
    term_val = R.value_of(ref.term_obs)
    term_val[ref.stored:] = np.nan                        # unreferenced slots must not reach an output
    got, consts = replay(exe, sc, n, T, ref.cap, term_val, np.ones(n, np.uint8))
    key = f"n {n} T {T} {pattern} cap {ref.cap}"
    assert (got["term_slot"] == ref.term_slot).all(), key
    assert tuple(got["count"]) == (ref.stored, ref.overflow), key
    assert (got["start"] == ref.start).all(), key
    assert (bits(got["adv"]) == bits(ref.adv)).all(), key
    assert (bits(got["ret"]) == bits(ref.ret)).all(), key
    assert np.isfinite(got["adv"]).all(), key
    return consts, ref


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", NS)
def test_replay_matches_rollout_buffer_bit_for_bit(programs, n, T):
    consts, _ = check(programs["plain"], n, T)
    assert consts[:2] == [256, 1024] and consts[2] == -(-n // consts[3])
    if n == 257:
        assert consts[2] == 2                              # the slot prefix crosses a chunk


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_done_patterns_and_overflow(programs, pattern):
    check(programs["plain"], 65, 5, pattern)
    _, ref = check(programs["plain"], 65, 5, pattern, cap=3)
    pairs = int((ref.term_slot >= 0).sum())
    assert pairs == ref.stored <= 3
    if pattern in ("all_trunc", "consecutive", "random"):
        assert ref.stored == 3 and ref.overflow > 0
        sc = R.script(65, 5, 3, 1, pattern)
        t, e = np.nonzero(sc["trunc"] & ~sc["term"])     # exactly the first three pairs in (t, env) order
        assert [int(ref.term_slot[t[i], e[i]]) for i in range(3)] == [0, 1, 2]
        assert (ref.term_slot[t[3:], e[3:]] == -1).all()
    if pattern in ("none", "both"):
        assert ref.stored == 0 and ref.overflow == 0


def test_script_would_show_a_contraction():
    """The scripted values contain bootstraps and GAE steps whose FMA-contracted result differs from the
    two-rounding one; with none of them the bitwise comparison could not see a contraction."""
    stats = {}
    for n, T in ((65, 5), (257, 33)):
        sc = R.script(n, T, 3, 1, "random")
        R.run(sc, n, T, 3, 1, gamma=GAMMA, gae_lambda=LAM, stats=stats)
        assert (sc["rew"] < -15).any() and (sc["rew"] > -5).any()
    assert stats["gae"] > 100 and stats["bootstrap"] > 10, stats


def test_replay_under_sanitizers(programs):
    """The same program built with -fsanitize=address,undefined, run directly (a stand-alone binary)."""
    check(programs["san"], 257, 33)
    check(programs["san"], 65, 5, "all_trunc", cap=3)
    check(programs["san"], 1, 1)


def test_chunks_grow_so_that_the_prefix_stays_bounded():
    """ro_chunk_envs / ro_num_chunks at 2^23 envs would need as many rows of input; the rule is restated
    and checked against the header's constants."""
    import os
    src = open(os.path.join(os.path.dirname(R.__file__), "..", "gym-usv_amd", "csrc", "usv_rollout_math.hpp")).read()
    assert "kRoBlock = 256" in src and "kRoMaxChunks = 1024" in src
    for n, envs in ((1, 256), (262144, 256), (262145, 512), (1 << 23, 8192)):
        assert 256 * max(1, -(-n // (256 * 1024))) == envs and -(-n // envs) <= 1024


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_scratch_bytes(lib):
    assert lib.usv_rollout_scratch_bytes(0) == 0 and lib.usv_rollout_scratch_bytes(-5) == 0
    assert lib.usv_rollout_scratch_bytes(1) == 16 + 8
    assert lib.usv_rollout_scratch_bytes(257) == 16 + 8
    assert lib.usv_rollout_scratch_bytes(3 * 256) == 16 + 16
    assert lib.usv_rollout_scratch_bytes(1 << 23) == 16 + 4096


def test_rollout_calls_refuse_bad_arguments_without_gpu(lib):
    """Everything usv_rollout_put_obs / _put_step / _gae can refuse before a HIP call is refused with
    USV_ERR_ARG and a message (so also on a machine without a GPU)."""
    from gym_usv_amd import _lib
    buf = (ctypes.c_uint8 * 128)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 8

    def ro(**kw):
        f = dict(n=4, n_steps=3, obs_width=6, act_dim=2, term_cap=8, reserved=0, obs=p, act=p, rew=p, val=p, logp=p,
                 adv=p, ret=p, start=p, term_slot=p, term_obs=p, term_count=p, scratch=p)
        f.update(kw)
        return _lib.UsvRollout(**f)

    def calls(r, word, t=1, stride=6, rb=4, gamma=0.99, lam=0.95, src=p, tv=p, which=(0, 1, 2)):
        rp = ctypes.byref(r) if r is not None else None
        fns = (lambda: lib.usv_rollout_put_obs(rp, t, src, stride, p, p, p, None),
               lambda: lib.usv_rollout_put_step(rp, t, p, rb, p, p, p, None),
               lambda: lib.usv_rollout_gae(rp, p, tv, gamma, lam, None))
        for i in which:
            assert fns[i]() == -1, (word, i)
            assert word in lib.usv_last_error(), (word, i, lib.usv_last_error())

    calls(None, b"null usv_rollout")
    for kw, word in ((dict(n=0), b"must be > 0"), (dict(n_steps=-1), b"must be > 0"), (dict(obs_width=0), b"must be > 0"),
                     (dict(act_dim=0), b"must be > 0"), (dict(term_cap=-1), b"term_cap"), (dict(reserved=1), b"reserved"),
                     (dict(obs=None), b"null buffer"), (dict(start=None), b"null buffer"),
                     (dict(term_obs=None), b"null buffer"), (dict(scratch=None), b"null buffer"),
                     (dict(val=p + 2), b"aligned"), (dict(scratch=p + 4), b"aligned"), (dict(term_slot=p + 1), b"aligned")):
        calls(ro(**kw), word)
    calls(ro(), b"[0, n_steps)", t=-1, which=(0, 1))
    calls(ro(), b"[0, n_steps)", t=3, which=(0, 1))
    calls(ro(), b"row stride", stride=5, which=(0,))
    calls(ro(), b"4-B aligned", src=p + 2, which=(0,))
    calls(ro(), b"reward_bytes", rb=2, which=(1,))
    calls(ro(), b"reward_bytes", rb=0, which=(1,))
    for g, lam in ((1.5, 0.95), (-0.1, 0.95), (0.99, 1.01), (0.99, -1e-9), (float("nan"), 0.95), (0.99, float("nan"))):
        calls(ro(), b"gamma and gae_lambda", gamma=g, lam=lam, which=(2,))
    calls(ro(), b"term_val is missing", tv=None, which=(2,))
    assert ctypes.sizeof(_lib.UsvRollout) == 6 * 4 + 12 * 8


def test_device_rollout_checks_its_arguments_first():
    """Bad shapes and dtypes raise ValueError before the device is looked at; good ones then meet the
    no-CPU-fallback rule."""
    import torch
    import gym_usv_amd
    from gym_usv_amd.rollout import DeviceRollout
    assert gym_usv_amd.DeviceRollout is DeviceRollout
    cpu = torch.device("cpu")
    for bad in ((0, 8, 6, 2), (4, 0, 6, 2), (4, 8, 0, 2), (4, 8, 6, -1)):
        with pytest.raises(ValueError):
            DeviceRollout(*bad, cpu)
    with pytest.raises(ValueError):
        DeviceRollout(4, 8, 6, 2, cpu, term_cap=-1)
    with pytest.raises(ValueError):
        DeviceRollout(4, 8, 6, 2, cpu, reward_dtype=torch.float16)
    with pytest.raises(gym_usv_amd.UsvLibError):
        DeviceRollout(4, 8, 6, 2, cpu)
