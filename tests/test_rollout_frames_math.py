"""The index and liveness arithmetic of the frame-deduplicated rollout storage
(gym-usv_amd/csrc/usv_rollout_frames_math.hpp) and the argument checks of usv_rollout_put_obs_frames /
usv_rollout_gather, without a GPU.

The header is plain C++: a stand-alone program built with AddressSanitizer and UBSan replays the frame
store (put_obs at t = 0, 1, ..) and the gather on host arrays whose sizes are exactly the layout's, through
the functions the kernels use.  The gathered rows are compared with full storage
(tests/rollout_frames_ref.py) bit for bit: no tolerance.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import rollout_frames_ref as F

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "usv_rollout_frames_math.hpp"
using namespace usv;

// argv: T n k D keep_sign B; stdin: windows [T][n][k D] f32, start [T + 1][n] u8, idx [B] i64.
// stdout: obs_out [B][k D] f32, bad count i64.  stderr: "C max_stack rows_in_flight".
int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int T = std::atoi(argv[1]), k = std::atoi(argv[3]), D = std::atoi(argv[4]);
  const int64_t n = std::atoll(argv[2]), B = std::atoll(argv[6]);
  const bool keep = std::atoi(argv[5]) != 0;
  const int W = k * D;
  std::vector<float> win((size_t)T * n * W), frames((size_t)n * rf_rows(T, k) * D, -77.0f), out((size_t)B * W);
  std::vector<unsigned char> start((size_t)(T + 1) * n);
  std::vector<int64_t> idx(B);
  if (std::fread(win.data(), 4, win.size(), stdin) != win.size()) return 3;
  if (std::fread(start.data(), 1, start.size(), stdin) != start.size()) return 3;
  if (std::fread(idx.data(), 8, B, stdin) != (size_t)B) return 3;
  for (int t = 0; t < T; ++t)                             // rollout_frames_obs_kernel
    for (int64_t e = 0; e < n; ++e) {
      const float* const src = &win[((size_t)t * n + e) * W] + rf_put_col(t, k, D);
      float* const dst = frames.data() + rf_row_offset(e, rf_put_row(t, k), T, k, D);
      for (int c = 0; c < rf_put_width(t, k, D); ++c) dst[c] = src[c];
    }
  int64_t bad = 0;
  const int64_t total = (int64_t)T * n;
  for (int64_t b = 0; b < B; ++b) {                       // rollout_gather_kernel
    float* const o = &out[(size_t)b * W];
    if (!rf_index_ok(idx[b], total)) {
      ++bad;
      for (int c = 0; c < W; ++c) o[c] = __builtin_nanf("");
      continue;
    }
    const int64_t t = idx[b] / n, e = idx[b] - t * n;
    const uint32_t live = rf_live_mask(start.data(), n, e, (int32_t)t, k);
    if (live & ~rf_all_live(k)) return 4;
    const float* const src = frames.data() + rf_sample_offset(e, t, T, k, D);
    for (int c = 0; c < W; ++c) o[c] = rf_slot_value(src[c], live, c / D, keep);
  }
  std::fwrite(out.data(), 4, out.size(), stdout);
  std::fwrite(&bad, 8, 1, stdout);
  std::fprintf(stderr, "C %d %d\n", kRfMaxStack, kRfRows);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The replay program with AddressSanitizer + UBSan: a stand-alone host binary, run directly."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("rollout_frames_math")
    src, exe = d / "replay.cpp", d / "replay_san"
    src.write_text(MAIN)
    # host C++ only (-x c++: no device pass); -fno-gpu-sanitize says so for the sanitizers as well
    subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g", f"-I{CSRC}",
                    "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


def replay(exe, win, start, idx, k, D, keep):
    T, n, W = win.shape
    idx = np.ascontiguousarray(idx, np.int64)
    data = b"".join(np.ascontiguousarray(x).tobytes() for x in (win.astype(np.float32), start.astype(np.uint8), idx))
    p = subprocess.run([exe, str(T), str(n), str(k), str(D), str(int(keep)), str(len(idx))], input=data,
                       capture_output=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    B = len(idx)
    return (np.frombuffer(p.stdout, np.float32, B * W).reshape(B, W),
            int(np.frombuffer(p.stdout, np.int64, 1, 4 * B * W)[0]),
            [int(x) for x in p.stderr.decode().split("C ", 1)[1].split()])


def starts(sc, T, n):
    """start as put_step writes it; row 0 is all ones: the gather must not consult it."""
    s = np.ones((T + 1, n), np.uint8)
    s[1:] = sc["term"] | sc["trunc"]
    return s


def check(exe, n, T, k, D, pattern, keep):
    sc = F.script(n, T, k, D, pattern=pattern, keep_sign=keep)
    rng = np.random.default_rng(n + T + k + D)
    M = T * n
    idx = np.concatenate((np.arange(M), rng.permutation(M), rng.integers(0, M, 7)))
    got, bad, consts = replay(exe, sc["obs"], starts(sc, T, n), idx, k, D, keep)
    assert bad == 0 and consts == [32, 4]
    assert (F.bits(got) == F.bits(F.gather(sc["obs"], idx))).all(), (n, T, k, D, pattern, keep)


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("k", (1, 2, 5))
def test_replay_equals_full_storage_bit_for_bit(program, k, keep):
    for D in (1, 3, 4, 143):
        for T in sorted({1, max(k - 1, 1), k, k + 2}):
            for n in (1, 65):
                for pattern in ("random", "double", "last"):
                    check(program, n, T, k, D, pattern, keep)


@pytest.mark.parametrize("pattern", F.PATTERNS)
def test_every_done_pattern(program, pattern):
    for keep in (False, True):
        check(program, 65, 7, 5, 6, pattern, keep)
        check(program, 65, 3, 5, 143, pattern, keep)


def test_scripts_can_show_a_wrong_clear_rule_and_an_off_by_one():
    """The scripts hold what the bitwise comparison needs to see: negative frames behind a boundary (the
    two clear modes differ there in the sign of zero), windows with two boundaries, and a live prologue."""
    n, T, k, D = 65, 7, 5, 6
    a = F.script(n, T, k, D, pattern="double", keep_sign=False)
    b = F.script(n, T, k, D, pattern="double", keep_sign=True)
    assert (a["frames"] < 0).mean() > 0.4 and (F.bits(a["frames"]) == 0x80000000).any() and (a["frames"] == 0).any()
    assert (F.bits(a["obs"]) != F.bits(b["obs"])).any() and (a["obs"] == b["obs"]).all()   # only the sign of zero
    assert (F.bits(b["obs"]) == 0x80000000).sum() > 100
    done = a["term"] | a["trunc"]
    assert (done[:-1] & done[1:]).any()                                   # two boundaries inside one window
    assert (a["windows"][0][:, :D] != 0).any()                            # frames older than the rollout, live
    last = F.script(n, T, k, D, pattern="last")
    assert (last["term"] | last["trunc"])[T - 1].all()
    # a gather that ignored the boundaries, or looked one step too far back or not far enough, is seen
    frames = np.concatenate((a["windows"][0].reshape(n, k, D)[:, :-1].transpose(1, 0, 2), a["frames"]))
    plain = np.stack([frames[t:t + k].transpose(1, 0, 2).reshape(n, k * D) for t in range(T)])
    assert (F.bits(plain) != F.bits(a["obs"])).any()


def test_replay_counts_bad_indices_and_fills_nan(program):
    n, T, k, D = 65, 5, 5, 3
    sc = F.script(n, T, k, D)
    M = T * n
    idx = np.array([0, -1, M - 1, M, 5, 2 ** 40, -2 ** 63, 7], np.int64)
    got, bad, _ = replay(program, sc["obs"], starts(sc, T, n), idx, k, D, False)
    ok = (idx >= 0) & (idx < M)
    assert bad == int((~ok).sum()) == 4
    assert np.isnan(got[~ok]).all()
    assert (F.bits(got[ok]) == F.bits(F.gather(sc["obs"], idx[ok]))).all()


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_frame_calls_refuse_bad_arguments_without_gpu(lib):
    """Everything usv_rollout_put_obs_frames / usv_rollout_gather can refuse before a HIP call is refused
    with USV_ERR_ARG and a message (so also on a machine without a GPU)."""
    from gym_usv_amd import _lib
    assert ctypes.sizeof(_lib.UsvRolloutFrames) == 3 * 4 + 4 + 2 * 8
    assert ctypes.sizeof(_lib.UsvRollout) == 6 * 4 + 12 * 8 and _lib.ABI_VERSION == 5 == lib.usv_abi_version()
    buf = (ctypes.c_uint8 * 128)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 8

    def ro(**kw):
        f = dict(n=4, n_steps=3, obs_width=6, act_dim=2, term_cap=8, reserved=0, obs=p, act=p, rew=p, val=p, logp=p,
                 adv=p, ret=p, start=p, term_slot=p, term_obs=p, term_count=p, scratch=p)
        f.update(kw)
        return _lib.UsvRollout(**f)

    def fr(**kw):
        f = dict(k=2, d=3, flags=0, frames=p, bad_count=p)
        f.update(kw)
        return _lib.UsvRolloutFrames(**f)

    def calls(r, f, word, t=1, stride=6, B=5, idx=p, outs=(p,) * 6, which=(0, 1)):
        rp = ctypes.byref(r) if r is not None else None
        fp = ctypes.byref(f) if f is not None else None
        fns = (lambda: lib.usv_rollout_put_obs_frames(rp, fp, t, p, stride, p, p, p, None),
               lambda: lib.usv_rollout_gather(rp, fp, idx, B, *outs, None))
        for i in which:
            assert fns[i]() == -1, (word, i)
            assert word in lib.usv_last_error(), (word, i, lib.usv_last_error())

    calls(None, fr(), b"null usv_rollout")
    calls(ro(), None, b"null usv_rollout_frames")
    for kw, word in ((dict(k=0), b"k and d"), (dict(d=0), b"k and d"), (dict(k=-1, d=-6), b"k and d"),
                     (dict(k=33, d=1), b"k must be <= 32"), (dict(k=2, d=4), b"must equal obs_width"),
                     (dict(k=5, d=143), b"must equal obs_width"), (dict(flags=2), b"unknown flags"),
                     (dict(frames=p + 2), b"4-B aligned"), (dict(bad_count=p + 1), b"4-B aligned")):
        calls(ro(), fr(**kw), word)
    calls(ro(obs=None), fr(frames=None), b"has no frames", which=(0,))     # a frame-mode call without frames
    calls(ro(), fr(frames=None), b"has no frames", which=(0,))
    calls(ro(), fr(), b"B must be > 0", B=0, which=(1,))
    calls(ro(), fr(), b"B must be > 0", B=-3, which=(1,))
    calls(ro(), fr(bad_count=None), b"null bad_count", which=(1,))
    calls(ro(), fr(), b"null idx", idx=None, which=(1,))
    calls(ro(), fr(), b"idx is not 8-B aligned", idx=p + 4, which=(1,))
    for i in range(6):
        calls(ro(), fr(), b"null output", outs=tuple(None if j == i else p for j in range(6)), which=(1,))
        calls(ro(), fr(), b"output is not 4-B aligned", outs=tuple(p + 2 if j == i else p for j in range(6)),
              which=(1,))
    # what usv_rollout_put_obs refuses
    calls(ro(), fr(), b"[0, n_steps)", t=-1, which=(0,))
    calls(ro(), fr(), b"[0, n_steps)", t=3, which=(0,))
    calls(ro(), fr(), b"row stride", stride=5, which=(0,))
    calls(ro(n=0), fr(), b"must be > 0")
    calls(ro(start=None), fr(), b"null buffer")
    calls(ro(obs=None), fr(frames=None), b"null buffer", which=(1,))      # full storage needs obs


def test_device_rollout_checks_n_stack_first():
    import torch
    from gym_usv_amd.rollout import DeviceRollout, RolloutSamples
    import gym_usv_amd
    cpu = torch.device("cpu")
    for bad in (0, 33, 4, -1):
        with pytest.raises(ValueError):
            DeviceRollout(4, 8, 6, 2, cpu, n_stack=bad)
    with pytest.raises(gym_usv_amd.UsvLibError):
        DeviceRollout(4, 8, 6, 2, cpu, n_stack=2)
    assert RolloutSamples._fields == ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns")
