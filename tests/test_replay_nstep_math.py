"""N-step sampling of the device replay buffer without a GPU: the two restatements of SB3's
NStepReplayBuffer._get_samples (tests/replay_nstep_ref.py) against each other, the header's stop rule, row
arithmetic and return accumulation (gym-usv_amd/csrc/usv_replay_math.hpp) through a stand-alone host program
built with AddressSanitizer and UBSan, and the argument checks of usv_replay_gather_nstep.  Every comparison
is bitwise: no tolerance."""
import ctypes
import subprocess

import numpy as np
import pytest

import replay_nstep_ref as N
import replay_ref as P

A = 2
N_STEPS = (1, 2, 3, 7, 8, 32)
GAMMAS = (0.99, 1.0, 0.0)

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "usv_replay_math.hpp"
using namespace usv;

// stdin, repeated until the end of the input, one case each: a header of 8 int64 (T n k D A R keep_sign checks),
// windows [T + 1][n][k D] f32, final_stack [T][n][k D] f32, act [T][n][A] f32, rew [T][n] f32, term [T][n] u8,
// trunc [T][n] u8, then `checks` checks in non-decreasing count: count, B, n_steps i64, g [33] f32, idx [B] i64.
// stdout, per check: obs [B][k D], act [B][A], next_obs [B][k D], dones [B], rewards [B], discounts [B] f32, then
// m [B], s_m [B], the next_obs mask [B] and the next_obs ring rows [B][k] (slot k - 1: -1) i64.
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
  // the buffers of usv_replay, exactly as large as the layout says; unwritten rows hold what would continue a run
  std::vector<float> frames((size_t)n * Pr * D, -77.0f), next_frame((size_t)R * n * D, -78.0f);
  std::vector<float> b_act((size_t)R * n * A, -79.0f), b_rew((size_t)R * n, -80.0f);
  std::vector<unsigned char> b_done((size_t)R * n, 0), b_timeout((size_t)R * n, 0), age((size_t)R * n, 99);
  std::vector<unsigned char> age_now((size_t)n, (unsigned char)rp_age_start(k));
  int64_t next_count = -1, B = 0, n_steps = 0;
  std::vector<int64_t> idx;
  std::vector<float> g(kRpMaxNStep + 1);
  auto next_check = [&]() {
    int64_t h[3];
    if (checks_left-- <= 0) { next_count = -1; return true; }
    if (std::fread(h, 8, 3, stdin) != 3) return false;
    next_count = h[0];
    B = h[1];
    n_steps = h[2];
    idx.resize(B);
    return n_steps >= 1 && n_steps <= kRpMaxNStep && rd(g) && rd(idx);
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
    while (count == next_count) {                         // replay_gather_nstep_kernel
      const RpLaps lp = rp_laps(count, R, k);
      const int64_t size = rp_size(count, R);
      std::vector<float> o_obs((size_t)B * W), o_act((size_t)B * A), o_next((size_t)B * W), o_done(B), o_rew(B), o_disc(B);
      std::vector<int64_t> o_m(B), o_sm(B), o_mask(B), o_rows((size_t)B * k, -1);
      for (int64_t b = 0; b < B; ++b) {
        const int64_t i = idx[b];
        if (!rp_index_ok(i, size, n)) return 8;
        const int64_t slot = i / n, e = i - slot * n;
        RpRun run = rp_run_begin();
        int32_t s = (int32_t)slot;
        // every step's values are read before any is applied, the steps behind the stop too
        std::vector<int32_t> sj(n_steps);
        std::vector<unsigned char> dn(n_steps), to(n_steps), ag(n_steps);
        std::vector<float> rv(n_steps);
        for (int j = 0; j < n_steps; ++j) {
          const size_t at = rp_slot_offset(s, e, n, 1);
          sj[j] = s, dn[j] = b_done[at], to[j] = b_timeout[at], ag[j] = age[at], rv[j] = b_rew[at];
          s = rp_next_slot(s, R);
        }
        for (int j = 0; j < n_steps; ++j) rp_run_step(run, j, sj[j], dn[j], to[j], ag[j], rv[j], g[j], lp.last);
        if (run.m > size - 1 || run.slot != (slot + run.m) % R) return 9;
        const int32_t first = rp_first_row(lp, (int32_t)slot, (int32_t)Pr);
        const uint32_t live = rp_live_mask(age[i], k), nlive = rp_next_live_mask(run.age, k);
        for (int f = 0; f < 2 * k; ++f) {
          const bool nx = f >= k;
          const int j = nx ? f - k : f;
          const float* src;
          if (nx && j == k - 1) {
            src = &next_frame[rp_slot_offset(run.slot, e, n, D)];
          } else {
            const int32_t row = nx ? rp_nstep_row(first, run.m, j, (int32_t)Pr) : rp_wrap(first + j, (int32_t)Pr);
            if (row < 0 || row >= Pr) return 10;
            if (nx) o_rows[(size_t)b * k + j] = row;
            src = &frames[rp_frame_offset(e, row, Pr, D)];
          }
          for (int x = 0; x < D; ++x)
            (nx ? o_next : o_obs)[(size_t)b * W + j * D + x] = rf_slot_value(src[x], nx ? nlive : live, j, keep);
        }
        for (int x = 0; x < A; ++x) o_act[b * A + x] = b_act[(size_t)i * A + x];
        o_done[b] = rp_done_out(run.done, run.timeout);
        o_rew[b] = run.ret;
        o_disc[b] = g[run.m + 1];
        o_m[b] = run.m, o_sm[b] = run.slot, o_mask[b] = nlive;
      }
      std::fwrite(o_obs.data(), 4, o_obs.size(), stdout);
      std::fwrite(o_act.data(), 4, o_act.size(), stdout);
      std::fwrite(o_next.data(), 4, o_next.size(), stdout);
      std::fwrite(o_done.data(), 4, o_done.size(), stdout);
      std::fwrite(o_rew.data(), 4, o_rew.size(), stdout);
      std::fwrite(o_disc.data(), 4, o_disc.size(), stdout);
      std::fwrite(o_m.data(), 8, o_m.size(), stdout);
      std::fwrite(o_sm.data(), 8, o_sm.size(), stdout);
      std::fwrite(o_mask.data(), 8, o_mask.size(), stdout);
      std::fwrite(o_rows.data(), 8, o_rows.size(), stdout);
      if (!next_check()) return 3;
    }
  }
  return next_count >= 0 ? 7 : 0;                         // 7: a check that no store reached
}

int main() {
  int64_t h[8];
  while (std::fread(h, 8, 8, stdin) == 8)
    if (const int rc = run_case(h)) return rc;
  std::fprintf(stderr, "N %d\n", kRpMaxNStep);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The n-step program with AddressSanitizer + UBSan: a stand-alone host binary, run directly."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("replay_nstep_math")
    src, exe = d / "nstep.cpp", d / "nstep_san"
    src.write_text(MAIN)
    # host C++ only (-x c++: no device pass); -fno-gpu-sanitize says so for the sanitizers as well
    subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g", f"-I{CSRC}",
                    "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


def padded_table(gamma, n_steps):
    g = np.zeros(33, np.float32)
    g[:n_steps + 1] = N.table(gamma, n_steps)
    return g


def run_many(exe, cases):
    """`cases`: [(sc, n, k, D, R, keep, checks)] with checks = [(count, n_steps, gamma, idx)] in non-decreasing
    count, all through one run of the program.  Returns, per case and check, the six outputs, m, s_m, the
    next_obs mask and the next_obs rows [B, k]."""
    parts = []
    for sc, n, k, D, R, keep, checks in cases:
        T = max(c[0] for c in checks)
        parts += [np.array([T, n, k, D, A, R, int(keep), len(checks)], np.int64), sc["windows"][:T + 1],
                  sc["final_stack"][:T], sc["act"][:T], sc["rew"][:T].astype(np.float32),
                  sc["term"][:T].astype(np.uint8), sc["trunc"][:T].astype(np.uint8)]
        for count, n_steps, gamma, idx in checks:
            parts += [np.array([count, len(idx), n_steps], np.int64), padded_table(gamma, n_steps), np.asarray(idx, np.int64)]
    data = b"".join(np.ascontiguousarray(x).tobytes() for x in parts)
    p = subprocess.run([exe], input=data, capture_output=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    assert p.stderr.decode().strip() == "N 32"
    res, at = [], 0
    for sc, n, k, D, R, keep, checks in cases:
        W, out = k * D, []
        for _, _, _, idx in checks:
            B, got = len(idx), []
            for w in (W, A, W, 1, 1, 1):
                got.append(np.frombuffer(p.stdout, np.float32, B * w, at).reshape(B, w))
                at += 4 * B * w
            for w in (1, 1, 1, k):
                got.append(np.frombuffer(p.stdout, np.int64, B * w, at).reshape(B, w))
                at += 8 * B * w
            out.append(got)
        res.append(out)
    assert at == len(p.stdout)
    return res


def ages_of(sc, n, k, count):
    """age[c] [n] of every stored step c < count, by the rule of usv_replay_math.hpp."""
    done = sc["term"] | sc["trunc"]
    ages, out = np.full(n, k - 1), []
    for c in range(count):
        out.append(ages.copy())
        ages = np.where(done[c], 0, np.minimum(ages + 1, k - 1))
    return out


def case(n, k, D, R, pattern, keep, seed=0):
    counts = P.counts_of(R)
    sc = P.script(n, max(counts), k, D, A, pattern, keep, seed=seed)
    refs = P.run(sc, n, R, k, D, A, counts)
    rng = np.random.default_rng(n + k + D + R)
    checks = []
    for c in counts:
        M = min(c, R) * n
        idx = np.concatenate((np.arange(M), rng.permutation(M)))
        for i, n_steps in enumerate(N_STEPS):
            checks.append((c, n_steps, GAMMAS[(i + c) % len(GAMMAS)], idx))
    return (sc, n, k, D, R, keep, checks), refs, (n, k, D, R, pattern, keep)


def test_the_two_restatements_agree():
    """The loop and the vectorised transcription: m, s_m and dones exactly for every n_steps; returns and
    discounts bit for bit for n_steps <= 7, where NumPy's sum(axis=1) is sequential."""
    seen = np.zeros(4, np.int64)
    for R in (1, 2, 3, 7):
        for pattern in P.PATTERNS:
            n, k, D = 65, 2, 1
            counts = P.counts_of(R)
            sc = P.script(n, max(counts), k, D, A, pattern)
            for c, ref in P.run(sc, n, R, k, D, A, counts).items():
                idx = np.arange(ref.size * n)
                for n_steps in N_STEPS + (4, 5, 6):
                    for gamma in GAMMAS + (0.9,):
                        (_, _, _, dones, ret, disc), m, sm, kinds = N.get_nstep(ref, idx, n_steps, gamma, count=c)
                        v_ret, v_disc, v_dones, v_m, v_sm = N.get_nstep_sb3(ref, idx, n_steps, gamma)
                        what = (R, pattern, c, n_steps, gamma)
                        assert (m == v_m).all() and (sm == v_sm).all(), what
                        assert (N.bits(dones) == N.bits(v_dones)).all(), what
                        assert (N.bits(disc) == N.bits(v_disc)).all(), what
                        assert (m <= ref.size - 1).all() and (m <= n_steps - 1).all()
                        if n_steps <= 7:
                            # (the transcription adds masked terms as +0.0: only a -0.0 return could differ)
                            assert (N.bits(ret) == N.bits(v_ret))[N.bits(ret) != 0x80000000].all(), what
                            assert (ret == v_ret).all(), what
                        np.add.at(seen, kinds, 1)
    assert (seen > 0).all(), dict(zip(N.STOPS, seen))


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("k", (1, 2, 5))
def test_header_functions_equal_the_definition(program, k, keep):
    seen = np.zeros(4, np.int64)
    for D in (1, 3, 4, 143):
        made = [case(n, k, D, R, pattern, keep) for R in sorted({1, 2, 3, k + 2}) for n in ((1, 65) if D < 143 else (3,))
                for pattern in P.PATTERNS]                # one run of the program for all of them
        for (args, refs, what), got_checks in zip(made, run_many(program, [m[0] for m in made])):
            sc, n, _, _, R, _, checks = args
            Pr = R + k - 1
            for (c, n_steps, gamma, idx), got in zip(checks, got_checks):
                want, m, sm, kinds = N.get_nstep(refs[c], idx, n_steps, gamma, count=c)
                np.add.at(seen, kinds, 1)
                for name, g, w in zip(("obs", "act", "next_obs", "dones", "rewards", "discounts"), got, want):
                    assert g.shape == w.shape and (P.bits(g) == P.bits(w)).all(), (name, what, c, n_steps, gamma)
                assert (got[6][:, 0] == m).all() and (got[7][:, 0] == sm).all(), (what, c, n_steps)
                # the masks and the rows, from the steps themselves
                slot, e = idx // n, idx % n
                step = slot + R * ((c - 1 - slot) // R) + m               # the step of transition (s_m, e)
                age = np.stack(ages_of(sc, n, k, c))[step, e]
                mask = np.zeros(len(idx), np.int64)
                for j in range(k):                                        # slot j of next_obs is live
                    mask |= ((j + 1 >= k - 1 - age) | (j == k - 1)).astype(np.int64) << j
                assert (got[8][:, 0] == mask).all(), (what, c, n_steps)
                for j in range(k - 1):
                    assert (got[9][:, j] == (step - k + 2 + j) % Pr).all(), (what, c, n_steps, j)
                assert (got[9][:, k - 1] == -1).all()
    assert (seen > 0).all(), dict(zip(N.STOPS, seen))


def test_returns_are_sequential_float32_sums_without_fma(program):
    """A run whose fused and unfused sums differ: the program's return is the unfused one."""
    n, k, D, R = 65, 1, 1, 40
    sc = P.script(n, R, k, D, A, "none")
    ref = P.run(sc, n, R, k, D, A, [R])[R]
    idx = np.arange(n)                                    # slot 0: 32 steps, no stop
    got = run_many(program, [(sc, n, k, D, R, False, [(R, 32, 0.99, idx)])])[0][0]
    want, m, _, _ = N.get_nstep(ref, idx, 32, 0.99, count=R)
    assert (m == 31).all()
    assert (P.bits(got[4]) == P.bits(want[4])).all()
    g = N.table(0.99, 32).astype(np.float64)
    fused = np.zeros(n, np.float32)
    for b in range(n):
        acc = ref.rew[0, b]
        for j in range(1, 32):                            # fl(acc + rew g) with one rounding
            acc = np.float32(np.float64(acc) + np.float64(ref.rew[j, b]) * g[j])
        fused[b] = acc
    assert (P.bits(fused) != P.bits(want[4][:, 0])).any()


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_gather_nstep_refuses_bad_arguments_without_gpu(lib):
    """Everything usv_replay_gather_nstep can refuse before a HIP call is refused with USV_ERR_ARG and a
    message (so also on a machine without a GPU): what usv_replay_gather refuses, and its own."""
    from gym_usv_amd import _lib
    assert _lib.ABI_VERSION == 5 == lib.usv_abi_version()
    buf = (ctypes.c_uint8 * 128)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 8
    good = (ctypes.c_float * 33)(*([1.0] * 33))

    def rp(**kw):
        f = dict(n=4, rows=3, obs_width=6, act_dim=2, k=2, d=3, flags=0, reserved=0, frames=p, next_frame=p, act=p,
                 rew=p, done=p, timeout=p, age=p, age_now=p, bad_count=p)
        f.update(kw)
        return _lib.UsvReplay(**f)

    def call(r, word, c=1, B=5, idx=p, n_steps=3, table=good, outs=(p,) * 6):
        r = ctypes.byref(r) if r is not None else None
        assert lib.usv_replay_gather_nstep(r, c, idx, B, n_steps, table, *outs, None) == -1, word
        assert word in lib.usv_last_error(), (word, lib.usv_last_error())

    call(None, b"null usv_replay")
    for kw, word in ((dict(n=0), b"must be > 0"), (dict(rows=0), b"must be > 0"), (dict(obs_width=-6), b"must be > 0"),
                     (dict(act_dim=0), b"must be > 0"), (dict(k=0), b"k must be in [1, 32]"), (dict(d=0), b"d >= 1"),
                     (dict(k=2, d=4), b"must equal obs_width"), (dict(flags=2), b"unknown flags"),
                     (dict(reserved=1), b"unknown flags"), (dict(frames=None), b"null buffer"),
                     (dict(age_now=None), b"null buffer"), (dict(bad_count=None), b"null buffer"),
                     (dict(frames=p + 2), b"not aligned"), (dict(rew=p + 1), b"not aligned"),
                     (dict(bad_count=p + 2), b"not aligned")):
        call(rp(**kw), word)
    call(rp(k=33, d=1, obs_width=33), b"k must be in [1, 32]")
    call(rp(), b"must be >= 0", c=-1)
    call(rp(), b"B must be > 0", B=0)
    call(rp(), b"B must be > 0", B=-3)
    call(rp(), b"null idx", idx=None)
    call(rp(), b"idx is not 8-B aligned", idx=p + 4)
    for i in range(6):
        call(rp(), b"null output", outs=tuple(None if j == i else p for j in range(6)))
        call(rp(), b"output is not 4-B aligned", outs=tuple(p + 2 if j == i else p for j in range(6)))
    for bad in (0, -1, 33, 2 ** 31 - 1):
        call(rp(), b"n_steps must be in [1, 32]", n_steps=bad)
    call(rp(), b"null discount table", table=None)
    for at, v in ((0, float("nan")), (3, float("inf")), (2, -float("inf"))):
        t = (ctypes.c_float * 33)(*([1.0] * 33))
        t[at] = v
        call(rp(), b"not finite", table=t)
    t = (ctypes.c_float * 33)(*([1.0] * 33))
    t[4] = float("nan")                                   # behind g[n_steps]: not read, the next check refuses
    call(rp(), b"null idx", table=t, idx=None)


def test_device_replay_checks_n_steps_and_gamma_first():
    import torch
    import gym_usv_amd
    from gym_usv_amd.replay import DeviceReplay, NStepReplaySamples, ReplaySamples, discount_table
    cpu = torch.device("cpu")
    for kw in (dict(n_steps=0), dict(n_steps=33), dict(n_steps=2.5), dict(gamma=-0.1), dict(gamma=1.5),
               dict(gamma=float("nan"))):
        with pytest.raises(ValueError):
            DeviceReplay(4, 64, 6, 2, cpu, n_stack=2, **kw)
    with pytest.raises(gym_usv_amd.UsvLibError):
        DeviceReplay(4, 64, 6, 2, cpu, n_stack=2, n_steps=3, gamma=0.9)
    assert gym_usv_amd.NStepReplaySamples is NStepReplaySamples
    assert NStepReplaySamples._fields == ReplaySamples._fields + ("discounts",)
    for gamma in GAMMAS + (0.9,):
        assert (N.bits(np.array(discount_table(gamma, 32), np.float32)) == N.bits(N.table(gamma, 32))).all()
    assert discount_table(0.0, 2) == [1.0, 0.0, 0.0]
