"""The index and liveness arithmetic of the device replay buffer (gym-usv_amd/csrc/usv_replay_math.hpp)
and the argument checks of usv_replay_put_obs / _put_step / _gather, without a GPU.

The header is plain C++: a stand-alone program built with AddressSanitizer and UBSan replays the stores
and the gather on host arrays whose sizes are exactly the layout's, through the functions the kernels
use.  Every gathered output is compared with full storage (tests/replay_ref.py) bit for bit: no tolerance.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import replay_ref as P

A = 2

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "usv_replay_math.hpp"
using namespace usv;

// stdin, repeated until the end of the input, one case each: a header of 8 int64 (T n k D A R keep_sign checks),
// windows [T + 1][n][k D] f32, final_stack [T][n][k D] f32, act [T][n][A] f32, rew [T][n] f32, term [T][n] u8,
// trunc [T][n] u8, then `checks` checks in increasing count: count i64, B i64, idx [B] i64.  stdout, per check:
// obs [B][k D], act [B][A], next_obs [B][k D], dones [B], rewards [B] f32 and the bad count i64.
// stderr: "C rows_in_flight".
template <typename T>
static bool rd(std::vector<T>& v) { return std::fread(v.data(), sizeof(T), v.size(), stdin) == v.size(); }

static int run_case(const int64_t* h) {
  const int T = (int)h[0], k = (int)h[2], D = (int)h[3], A = (int)h[4], R = (int)h[5];
  const int64_t n = h[1];
  const bool keep = h[6] != 0;
  int64_t checks_left = h[7];
  const int W = k * D;
  const int64_t Pr = rp_frame_rows(R, k);
  std::vector<float> win((size_t)(T + 1) * n * W), fin((size_t)T * n * W), act((size_t)T * n * A), rew((size_t)T * n);
  std::vector<unsigned char> term((size_t)T * n), trunc((size_t)T * n);
  if (!rd(win) || !rd(fin) || !rd(act) || !rd(rew) || !rd(term) || !rd(trunc)) return 3;
  // the buffers of usv_replay, exactly as large as the layout says
  std::vector<float> frames((size_t)n * Pr * D, -77.0f), next_frame((size_t)R * n * D, -78.0f);
  std::vector<float> b_act((size_t)R * n * A, -79.0f), b_rew((size_t)R * n, -80.0f);
  std::vector<unsigned char> b_done((size_t)R * n, 9), b_timeout((size_t)R * n, 9), age((size_t)R * n, 99);
  std::vector<unsigned char> age_now((size_t)n, (unsigned char)rp_age_start(k));
  int64_t next_count = -1, B = 0;
  std::vector<int64_t> idx;
  auto next_check = [&]() {
    int64_t h[2];
    if (checks_left-- <= 0) { next_count = -1; return true; }
    if (std::fread(h, 8, 2, stdin) != 2) return false;
    next_count = h[0];
    B = h[1];
    idx.resize(B);
    return rd(idx);
  };
  if (!next_check()) return 3;
  for (int64_t c = 0; c < T; ++c) {
    const int32_t slot = rp_slot(c, R);
    for (int64_t e = 0; e < n; ++e) {                     // replay_obs_kernel
      const float* const w = &win[((size_t)c * n + e) * W];
      if (c == 0)
        for (int j = 0; j < k - 1; ++j)
          for (int x = 0; x < D; ++x)
            frames[rp_frame_offset(e, rp_frame_row(j - (k - 1), Pr), Pr, D) + x] = w[j * D + x];
      for (int x = 0; x < D; ++x) frames[rp_frame_offset(e, rp_frame_row(c, Pr), Pr, D) + x] = w[(k - 1) * D + x];
      for (int x = 0; x < A; ++x) b_act[rp_slot_offset(slot, e, n, A) + x] = act[((size_t)c * n + e) * A + x];
      age[rp_slot_offset(slot, e, n, 1)] = age_now[e];
    }
    for (int64_t e = 0; e < n; ++e) {                     // replay_step_kernel
      const size_t at = (size_t)c * n + e, s = rp_slot_offset(slot, e, n, 1);
      const unsigned char dn = rp_done(term[at], trunc[at]);
      b_rew[s] = rew[at];
      b_done[s] = dn;
      b_timeout[s] = rp_timeout(term[at], trunc[at]);
      age_now[e] = (unsigned char)rp_age_next(age_now[e], dn != 0, k);
      const float* const src = (dn ? &fin[at * W] : &win[((size_t)(c + 1) * n + e) * W]) + (k - 1) * D;
      for (int x = 0; x < D; ++x) next_frame[rp_slot_offset(slot, e, n, D) + x] = src[x];
    }
    const int64_t count = c + 1;
    if (count != next_count) continue;
    // replay_gather_kernel
    const RpLaps g = rp_laps(count, R, k);
    const int64_t size = rp_size(count, R);
    std::vector<float> o_obs((size_t)B * W), o_act((size_t)B * A), o_next((size_t)B * W), o_done(B), o_rew(B);
    int64_t bad = 0;
    const float nan = __builtin_nanf("");
    for (int64_t b = 0; b < B; ++b) {
      const int64_t i = idx[b];
      if (!rp_index_ok(i, size, n)) {
        ++bad;
        for (int x = 0; x < W; ++x) o_obs[b * W + x] = o_next[b * W + x] = nan;
        for (int x = 0; x < A; ++x) o_act[b * A + x] = nan;
        o_done[b] = o_rew[b] = nan;
        continue;
      }
      const int64_t slot = i / n, e = i - slot * n;
      const int32_t first = rp_first_row(g, (int32_t)slot, (int32_t)Pr);
      if (first != rp_frame_row(rp_step_of_slot((int32_t)slot, count, R) - (k - 1), Pr)) return 4;
      const uint32_t live = rp_live_mask(age[i], k);
      if ((live & ~rf_all_live(k)) || !((live >> (k - 1)) & 1u)) return 5;
      for (int j = 0; j <= k; ++j) {
        const float* const src = j == k ? &next_frame[rp_slot_offset(slot, e, n, D)]
                                        : &frames[rp_frame_offset(e, rp_wrap(first + j, (int32_t)Pr), Pr, D)];
        // slot j - 1 of next_obs has the liveness of frame j
        if (j >= 1 && (((rp_next_live_mask(age[i], k) >> (j - 1)) & 1u) != 0) !=
                          (rp_frame_value(1.0f, live, j, k, false) == 1.0f))
          return 6;
        const int np = D >= 4 ? rp_pieces(D) : D, w = D >= 4 ? 4 : 1;
        for (int p = 0; p < np; ++p) {
          const int col = D >= 4 ? rp_piece_col(p, D) : p;
          for (int x = col; x < col + w; ++x) {
            const float v = rp_frame_value(src[x], live, j, k, keep);
            if (j < k) o_obs[(size_t)b * W + j * D + x] = v;
            if (j >= 1) o_next[(size_t)b * W + (j - 1) * D + x] = v;
          }
        }
      }
      for (int x = 0; x < A; ++x) o_act[b * A + x] = b_act[(size_t)i * A + x];
      o_done[b] = rp_done_out(b_done[i], b_timeout[i]);
      o_rew[b] = b_rew[i];
    }
    std::fwrite(o_obs.data(), 4, o_obs.size(), stdout);
    std::fwrite(o_act.data(), 4, o_act.size(), stdout);
    std::fwrite(o_next.data(), 4, o_next.size(), stdout);
    std::fwrite(o_done.data(), 4, o_done.size(), stdout);
    std::fwrite(o_rew.data(), 4, o_rew.size(), stdout);
    std::fwrite(&bad, 8, 1, stdout);
    if (!next_check()) return 3;
  }
  return next_count >= 0 ? 7 : 0;                         // 7: a check that no store reached
}

int main() {
  int64_t h[8];
  while (std::fread(h, 8, 8, stdin) == 8)
    if (const int rc = run_case(h)) return rc;
  std::fprintf(stderr, "C %d\n", kRpRows);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The replay program with AddressSanitizer + UBSan: a stand-alone host binary, run directly."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("replay_math")
    src, exe = d / "replay.cpp", d / "replay_san"
    src.write_text(MAIN)
    # host C++ only (-x c++: no device pass); -fno-gpu-sanitize says so for the sanitizers as well
    subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g", f"-I{CSRC}",
                    "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


def replay_many(exe, cases):
    """`cases`: [(sc, n, k, D, R, keep, checks)] with checks = [(count, idx)] in increasing count, all through
    one run of the program.  Returns, per case, [(obs, act, next_obs, dones, rewards, bad)] per check."""
    parts = []
    for sc, n, k, D, R, keep, checks in cases:
        T = max(c for c, _ in checks)
        parts += [np.array([T, n, k, D, A, R, int(keep), len(checks)], np.int64), sc["windows"][:T + 1],
                  sc["final_stack"][:T], sc["act"][:T], sc["rew"][:T].astype(np.float32),
                  sc["term"][:T].astype(np.uint8), sc["trunc"][:T].astype(np.uint8)]
        for count, idx in checks:
            parts += [np.array([count, len(idx)], np.int64), np.asarray(idx, np.int64)]
    data = b"".join(np.ascontiguousarray(x).tobytes() for x in parts)
    p = subprocess.run([exe], input=data, capture_output=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    assert p.stderr.decode().strip() == "C 4"
    res, at = [], 0
    for sc, n, k, D, R, keep, checks in cases:
        W, out = k * D, []
        for _, idx in checks:
            B, got = len(idx), []
            for w in (W, A, W, 1, 1):
                got.append(np.frombuffer(p.stdout, np.float32, B * w, at).reshape(B, w))
                at += 4 * B * w
            got.append(int(np.frombuffer(p.stdout, np.int64, 1, at)[0]))
            at += 8
            out.append(got)
        res.append(out)
    assert at == len(p.stdout)
    return res


def replay(exe, sc, n, k, D, R, keep, checks):
    return replay_many(exe, [(sc, n, k, D, R, keep, checks)])[0]


def case(n, k, D, R, pattern, keep):
    """A scripted case: its reference states and its checks, over every valid index and a permutation."""
    counts = P.counts_of(R)
    sc = P.script(n, max(counts), k, D, A, pattern, keep)
    refs = P.run(sc, n, R, k, D, A, counts)
    rng = np.random.default_rng(n + k + D + R)
    checks = []
    for c in counts:
        M = min(c, R) * n
        checks.append((c, np.concatenate((np.arange(M), rng.permutation(M)))))
    return (sc, n, k, D, R, keep, checks), refs, (n, k, D, R, pattern, keep)


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("k", (1, 2, 5))
def test_replay_equals_full_storage_bit_for_bit(program, k, keep):
    for D in (1, 3, 4, 143):
        made = [case(n, k, D, R, pattern, keep) for R in sorted({1, 2, max(k - 1, 1), k, k + 2}) for n in (1, 65)
                for pattern in P.PATTERNS]                # one run of the program for all of them
        for (args, refs, what), got_checks in zip(made, replay_many(program, [m[0] for m in made])):
            for (c, idx), got in zip(args[6], got_checks):
                assert got[5] == 0
                for name, g, w in zip(("obs", "act", "next_obs", "dones", "rewards"), got, refs[c].get(idx)):
                    assert g.shape == w.shape and (P.bits(g) == P.bits(w)).all(), (name, what, c)


def rebuild(sc, n, k, D, R, count, keep, use_age=True, back=0):
    """A NumPy frame-storage rebuild of every valid (slot, env) of obs and next_obs after `count` stores,
    optionally wrong: ignoring age, or reading `back` rows too far back."""
    W = k * D
    done = sc["term"] | sc["trunc"]
    fr = {c: sc["windows"][c][:, (k - 1) * D:] for c in range(count)}
    for j in range(k - 1):
        fr[j - (k - 1)] = sc["windows"][0][:, j * D:(j + 1) * D]
    fr[-k] = np.full((n, D), 123.0, np.float32)          # (one row further back than the layout keeps)
    ages = np.full(n, k - 1)
    age = {}
    for c in range(count):
        age[c] = ages.copy()
        ages = np.where(done[c], 0, np.minimum(ages + 1, k - 1))
    obs, nxt = np.zeros((min(count, R), n, W), np.float32), np.zeros((min(count, R), n, W), np.float32)
    for slot in range(min(count, R)):
        c = slot + R * ((count - 1 - slot) // R)
        nf = np.where(done[c][:, None], sc["final"][c], sc["windows"][c + 1][:, (k - 1) * D:])
        seq = [fr[max(c - k + 1 + j - back, -k)] for j in range(k)] + [nf]
        for j in range(k + 1):
            live = (min(j, k - 1) >= k - 1 - age[c]) | (not use_age)
            v = np.where(live[:, None], seq[j], P.F.cleared(seq[j], keep))
            if j < k:
                obs[slot][:, j * D:(j + 1) * D] = v
            if j >= 1:
                nxt[slot][:, (j - 1) * D:j * D] = v
    return obs, nxt


def test_scripts_can_show_a_wrong_rebuild():
    """The scripts hold what the bitwise comparison needs to see."""
    n, k, D, R = 65, 5, 6, 7
    count = 2 * R + (R + 1) // 2                         # 18
    a = P.script(n, count, k, D, A, "double", False)
    b = P.script(n, count, k, D, A, "double", True)
    rnd = P.script(n, count, k, D, A, "random", False)
    Pr = R + k - 1
    # windows that straddle the ring end: a valid step whose k frame rows wrap
    steps = [slot + R * ((count - 1 - slot) // R) for slot in range(R)]
    assert any((c - k + 1) % Pr > c % Pr for c in steps)
    done = a["term"] | a["trunc"]
    assert (done[:-1] & done[1:]).any()                                   # two boundaries inside one window
    assert (a["windows"][0][:, :D] != 0).any()                            # a live prologue
    # negative frames behind a boundary: the two clear modes differ in the sign of zero only
    assert (P.bits(a["windows"]) != P.bits(b["windows"])).any() and (a["windows"] == b["windows"]).all()
    assert (P.bits(b["windows"]) == 0x80000000).sum() > 100
    tr, tm = rnd["trunc"], rnd["term"]
    assert (tr & ~tm).any() and (tm & tr).any() and (tm & ~tr).any()      # timeouts, and both kinds of termination
    # the right rebuild equals full storage; one that ignores age, or reads a row too far back, does not
    for sc, keep in ((a, False), (b, True), (rnd, False)):
        ref = P.run(sc, n, R, k, D, A, [count])[count]
        obs, nxt = rebuild(sc, n, k, D, R, count, keep)
        assert (P.bits(obs) == P.bits(ref.obs)).all() and (P.bits(nxt) == P.bits(ref.next_obs)).all()
        for kw in (dict(use_age=False), dict(back=1)):
            o2, n2 = rebuild(sc, n, k, D, R, count, keep, **kw)
            assert (P.bits(o2) != P.bits(ref.obs)).any() and (P.bits(n2) != P.bits(ref.next_obs)).any(), kw
    # a live prologue is seen by the first stores
    ref = P.run(a, n, R, k, D, A, [1])[1]
    o2, _ = rebuild(a, n, k, D, R, 1, False, back=1)
    assert (P.bits(o2) != P.bits(ref.obs[:1])).any()


def test_replay_counts_bad_indices_and_fills_nan(program):
    n, k, D, R = 65, 5, 3, 4
    sc = P.script(n, R + 1, k, D, A)
    refs = P.run(sc, n, R, k, D, A, [2, R + 1])
    # slot 2 (index 2 * n + 5) is valid only once the ring holds three transitions
    idx = np.array([0, -1, 2 * n - 1, 2 * n + 5, 5, 2 ** 40, -2 ** 63, 7, R * n], np.int64)
    for (count, ref), got in zip(sorted(refs.items()), replay(program, sc, n, k, D, R, False, [(2, idx), (R + 1, idx)])):
        ok = (idx >= 0) & (idx < min(count, R) * n)
        assert got[5] == int((~ok).sum()) == (5 if count == 2 else 4)
        for g, w in zip(got[:5], ref.get(idx[ok])):
            assert np.isnan(g[~ok]).all()
            assert (P.bits(g[ok]) == P.bits(w)).all()


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_replay_calls_refuse_bad_arguments_without_gpu(lib):
    """Everything usv_replay_put_obs / _put_step / _gather can refuse before a HIP call is refused with
    USV_ERR_ARG and a message (so also on a machine without a GPU)."""
    from gym_usv_amd import _lib
    assert ctypes.sizeof(_lib.UsvReplay) == 8 * 4 + 9 * 8
    assert _lib.ABI_VERSION == 5 == lib.usv_abi_version()
    buf = (ctypes.c_uint8 * 128)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 8

    def rp(**kw):
        f = dict(n=4, rows=3, obs_width=6, act_dim=2, k=2, d=3, flags=0, reserved=0, frames=p, next_frame=p, act=p,
                 rew=p, done=p, timeout=p, age=p, age_now=p, bad_count=p)
        f.update(kw)
        return _lib.UsvReplay(**f)

    def calls(r, word, c=1, stride=6, rb=4, B=5, idx=p, outs=(p,) * 5, src=p, which=(0, 1, 2)):
        r = ctypes.byref(r) if r is not None else None
        fns = (lambda: lib.usv_replay_put_obs(r, c, src, stride, p, None),
               lambda: lib.usv_replay_put_step(r, c, src, rb, p, p, p, stride, p, None),
               lambda: lib.usv_replay_gather(r, c, idx, B, *outs, None))
        for i in which:
            assert fns[i]() == -1, (word, i)
            assert word in lib.usv_last_error(), (word, i, lib.usv_last_error())

    calls(None, b"null usv_replay")
    for kw, word in ((dict(n=0), b"must be > 0"), (dict(rows=0), b"must be > 0"), (dict(obs_width=-6), b"must be > 0"),
                     (dict(act_dim=0), b"must be > 0"), (dict(k=0), b"k must be in [1, 32]"),
                     (dict(d=0), b"d >= 1"),
                     (dict(k=2, d=4), b"must equal obs_width"), (dict(flags=2), b"unknown flags"),
                     (dict(reserved=1), b"unknown flags"), (dict(frames=None), b"null buffer"),
                     (dict(age_now=None), b"null buffer"), (dict(bad_count=None), b"null buffer"),
                     (dict(frames=p + 2), b"not aligned"), (dict(rew=p + 1), b"not aligned"),
                     (dict(bad_count=p + 2), b"not aligned")):
        calls(rp(**kw), word)
    calls(rp(k=33, d=1, obs_width=33), b"k must be in [1, 32]", stride=33)
    calls(rp(), b"must be >= 0", c=-1)
    calls(rp(), b"row stride", stride=5, which=(0, 1))
    calls(rp(), b"null argument", src=None, which=(0, 1))
    calls(rp(), b"not aligned", src=p + 2, which=(0, 1))
    calls(rp(), b"reward_bytes must be 4 or 8", rb=2, which=(1,))
    calls(rp(), b"not aligned", src=p + 4, rb=8, which=(1,))
    calls(rp(), b"B must be > 0", B=0, which=(2,))
    calls(rp(), b"B must be > 0", B=-3, which=(2,))
    calls(rp(), b"null idx", idx=None, which=(2,))
    calls(rp(), b"idx is not 8-B aligned", idx=p + 4, which=(2,))
    for i in range(5):
        calls(rp(), b"null output", outs=tuple(None if j == i else p for j in range(5)), which=(2,))
        calls(rp(), b"output is not 4-B aligned", outs=tuple(p + 2 if j == i else p for j in range(5)), which=(2,))


def test_device_replay_checks_its_arguments_first():
    import torch
    import gym_usv_amd
    from gym_usv_amd.replay import DeviceReplay, ReplaySamples
    cpu = torch.device("cpu")
    for bad in (0, 33, 4, -1):
        with pytest.raises(ValueError):
            DeviceReplay(4, 64, 6, 2, cpu, n_stack=bad)
    with pytest.raises(ValueError):
        DeviceReplay(4, 0, 6, 2, cpu, n_stack=2)
    with pytest.raises(ValueError):
        DeviceReplay(4, 64, 6, 2, cpu, torch.float16, n_stack=2)
    with pytest.raises(gym_usv_amd.UsvLibError):
        DeviceReplay(4, 64, 6, 2, cpu, n_stack=2)
    assert gym_usv_amd.DeviceReplay is DeviceReplay
    assert ReplaySamples._fields == ("observations", "actions", "next_observations", "dones", "rewards")
