"""The minibatch permutation and cursor of usv_rollout_gather_perm without a GPU: perm_index / perm_inverse /
cursor_ticked (gym-usv_amd/csrc/usv_rollout_perm_math.hpp) through a stand-alone host program built with
AddressSanitizer and UBSan, compared index for index with tests/rollout_perm_ref.py's restatement; the argument
refusals of the new C entry, which are reached before any HIP call; and the ValueError paths of the sampler and of the
PPO example's flags that need no device."""
import ctypes
import itertools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import rollout_perm_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 4, 5, 6, 35, 64, 257, 512, 1000, 4096, 80_000)
SEEDS = (0, 0x5DE5DE5DE5DE5DE5, 0xFFFFFFFFFFFFFFFF)
EPOCHS = (0, 1, 2, 0xFFFFFFFF)
BIG = (2 ** 31 + 11, 2 ** 40 + 3)
WALK_CAP = 128            # a pass leaves [0, M) with probability below 3/4: 128 passes in a row do not occur
CHI2_15, CHI2_3 = 44.3, 21.1      # the 1 - 1e-4 quantiles at 15 and 3 degrees of freedom

MAIN = r"""
#include <cstdio>
#include <vector>
#include "usv_rollout_perm_math.hpp"
using namespace usv;

// stdin, repeated until the end of the input: u64 seed, u32 epoch, u32 mode, i64 M, i64 count, and for the modes 0
// and 1 count i64 values.  stdout per record: count pairs of i64.
//   mode 0  (perm_index(value), passes taken)      mode 1  (perm_inverse(value), 0)
//   mode 2  mode 0 over the values 0 .. count - 1  mode 3  the cursor (epoch, batch = seed) ticked count times with
//                                                          n_batches = M: (epoch, batch) after every tick
int main() {
  static_assert(sizeof(RolloutCursor) == 16 && alignof(RolloutCursor) == 16, "the cursor block");
  struct Head { uint64_t seed; uint32_t epoch, mode; int64_t M, count; } h;
  static_assert(sizeof(Head) == 32, "the record's head");
  while (std::fread(&h, sizeof h, 1, stdin) == 1) {
    if (h.M < 1 || h.count < 0 || h.mode > 3) return 3;
    std::vector<int64_t> in((size_t)(h.mode < 2 ? h.count : 0)), out((size_t)h.count * 2);
    if (!in.empty() && std::fread(in.data(), 8, in.size(), stdin) != in.size()) return 4;
    uint32_t epoch = h.epoch, batch = (uint32_t)h.seed;
    for (int64_t j = 0; j < h.count; ++j) {
      int walk = 0;
      if (h.mode == 0 || h.mode == 2) {
        const int64_t p = h.mode == 0 ? in[(size_t)j] : j;
        if (p < 0 || p >= h.M) return 5;
        out[2 * j] = perm_index(h.seed, h.epoch, h.M, p, &walk);
        out[2 * j + 1] = walk;
      } else if (h.mode == 1) {
        out[2 * j] = perm_inverse(h.seed, h.epoch, h.M, in[(size_t)j]);
        out[2 * j + 1] = 0;
      } else {
        cursor_ticked(epoch, batch, (uint32_t)h.M);
        out[2 * j] = epoch;
        out[2 * j + 1] = batch;
      }
    }
    if (!out.empty() && std::fwrite(out.data(), 8, out.size(), stdout) != out.size()) return 6;
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program with AddressSanitizer + UBSan: a stand-alone host binary, run directly."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("rollout_perm_math")
    src, exe = d / "perm.cpp", d / "perm_san"
    src.write_text(MAIN)
    subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g", f"-I{CSRC}",
                    "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


def record(seed, epoch, mode, M, count, values=None):
    head = np.array([seed], np.uint64).tobytes() + np.array([epoch, mode], np.uint32).tobytes() + \
        np.array([M, count], np.int64).tobytes()
    return head + (b"" if values is None else np.asarray(values, np.int64).tobytes())


def run(program, records, counts):
    """One process for all records; returns one [count, 2] int64 array per record."""
    p = subprocess.run([program], input=b"".join(records), capture_output=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    out = np.frombuffer(p.stdout, np.int64).reshape(-1, 2)
    assert len(out) == sum(counts)
    return np.split(out, np.cumsum(counts)[:-1])


@pytest.fixture(scope="module")
def sweep(program):
    """perm_index over every position of every (M, seed, epoch) of the sweep: {case: [M, 2] (index, passes)}."""
    cases = list(itertools.product(SIZES, SEEDS, EPOCHS))
    outs = run(program, [record(s, e, 2, M, M) for M, s, e in cases], [M for M, _, _ in cases])
    return dict(zip(cases, outs))


def test_every_case_is_a_bijection_and_equals_the_restatement(sweep):
    longest = 0
    for (M, seed, epoch), out in sweep.items():
        idx, walks = out[:, 0], out[:, 1]
        assert (np.sort(idx) == np.arange(M)).all(), (M, seed, epoch)
        ref, ref_walks = P.perm_index(seed, epoch, M, np.arange(M), walks=True)
        assert (idx == ref).all() and (walks == ref_walks).all(), (M, seed, epoch)
        longest = max(longest, int(walks.max()))
    print(f"longest cycle walk over {len(sweep)} cases: {longest} passes")
    assert longest <= WALK_CAP


def test_the_inverse_inverts(program):
    cases = [(M, s, e) for M in (1, 2, 3, 35, 512, 1000) for s in SEEDS[:2] for e in EPOCHS[1:3]]
    outs = run(program, [record(s, e, 1, M, M, np.arange(M)) for M, s, e in cases], [M for M, _, _ in cases])
    for (M, s, e), out in zip(cases, outs):
        perm = P.permutation(s, e, M)
        assert (perm[out[:, 0]] == np.arange(M)).all(), (M, s, e)
        assert (P.perm_inverse(s, e, M, np.arange(M)) == out[:, 0]).all(), (M, s, e)


@pytest.mark.parametrize("M", BIG)
def test_large_m_stays_in_range_and_inverts(program, M):
    """Halves above 16 bits, and for 2^40 + 3 a sample index past 2^32: too large to enumerate, so the inverse."""
    rng = np.random.default_rng(M % 1000)
    pos = np.unique(np.concatenate(([0, M - 1], rng.integers(0, M, 4094))))
    seed, epoch = SEEDS[1], 7
    fwd, = run(program, [record(seed, epoch, 0, M, len(pos), pos)], [len(pos)])
    idx = fwd[:, 0]
    assert ((idx >= 0) & (idx < M)).all() and len(np.unique(idx)) == len(pos)
    back, = run(program, [record(seed, epoch, 1, M, len(pos), idx)], [len(pos)])
    assert (back[:, 0] == pos).all()
    assert (P.perm_index(seed, epoch, M, pos) == idx).all()
    print(f"M = {M}: longest walk {int(fwd[:, 1].max())} passes")
    assert fwd[:, 1].max() <= WALK_CAP


def test_epochs_and_seeds_give_different_permutations(program):
    M = 512
    cases = [(s, e) for s in SEEDS for e in range(64)]
    outs = run(program, [record(s, e, 2, M, M) for s, e in cases], [M] * len(cases))
    assert len({o[:, 0].tobytes() for o in outs}) == len(cases)      # no two of 3 x 64 are the same


def test_where_a_position_and_a_sample_land_is_uniform(program):
    """M = 512, B = 128, one seed, 2048 epochs: the sample that position 0 draws, in 16 buckets, and the minibatch
    that sample 0 falls into.  Deterministic: the seed is fixed."""
    M, B, seed, n = 512, 128, 0x5DE5DE5DE5DE5DE5, 2048
    outs = run(program, [record(seed, e, m, M, 1, [0]) for e in range(n) for m in (0, 1)], [1] * (2 * n))
    land = np.array([o[0, 0] for o in outs[0::2]])
    where = np.array([o[0, 0] for o in outs[1::2]])
    assert (land == [P.perm_index(seed, e, M, 0)[0] for e in range(0, n)]).all()

    def chi2(counts):
        want = n / len(counts)
        return float(((counts - want) ** 2 / want).sum())
    first = chi2(np.bincount(land // (M // 16), minlength=16))
    second = chi2(np.bincount(where // B, minlength=M // B))
    print(f"chi-square: position 0's sample {first:.2f} (15 dof), sample 0's minibatch {second:.2f} (3 dof)")
    assert first < CHI2_15 and second < CHI2_3


def test_the_cursor_ticks_through_an_epoch_and_wraps(program):
    a, b, c = run(program, [record(0, 5, 3, 4, 9), record(3, 0xFFFFFFFF, 3, 4, 2), record(9, 7, 3, 4, 1)], [9, 2, 1])
    want = [(5, 1), (5, 2), (5, 3), (6, 0), (6, 1), (6, 2), (6, 3), (7, 0), (7, 1)]
    assert [tuple(r) for r in a] == want
    assert [tuple(r) for r in b] == [(0, 0), (0, 1)]                 # batch 3 of 4 was the last: 0xFFFFFFFF wraps to 0
    assert [tuple(r) for r in c] == [(7, 1)]                         # a batch word that is no batch counts as 0
    e, k = 5, 0
    for got in a:
        e, k = P.cursor_ticked(e, k, 4)
        assert (e, k) == tuple(got)
    assert P.cursor_ticked(0xFFFFFFFF, 3, 4) == (0, 0) and P.cursor_ticked(7, 9, 4) == (7, 1)
    one, = run(program, [record(0, 0xFFFFFFFE, 3, 1, 3)], [3])       # one minibatch an epoch
    assert [tuple(r) for r in one] == [(0xFFFFFFFF, 0), (0, 0), (1, 0)]


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_gather_perm_refuses_bad_arguments_without_gpu(lib):
    """Everything usv_rollout_gather_perm can refuse before a HIP call is refused with USV_ERR_ARG and a message."""
    from gym_usv_amd import _lib
    assert _lib.ABI_VERSION == 5 == lib.usv_abi_version()
    assert lib.usv_rollout_cursor_bytes() == 16 and lib.usv_rollout_cursor_bytes() % 16 == 0
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    q = p + 64                                              # the cursor block: not an output

    def ro(**kw):
        f = dict(n=4, n_steps=3, obs_width=6, act_dim=2, term_cap=8, reserved=0, obs=p, act=p, rew=p, val=p, logp=p,
                 adv=p, ret=p, start=p, term_slot=p, term_obs=p, term_count=p, scratch=p)
        f.update(kw)
        return _lib.UsvRollout(**f)

    def fr(**kw):
        f = dict(k=2, d=3, flags=0, frames=p, bad_count=p)
        f.update(kw)
        return _lib.UsvRolloutFrames(**f)

    def refused(word, r=None, f=None, cursor=q, B=6, idx_out=None, outs=(p,) * 6, null_ro=False, null_fr=False):
        r, f = r or ro(), f or fr()
        rc = lib.usv_rollout_gather_perm(None if null_ro else ctypes.byref(r), None if null_fr else ctypes.byref(f),
                                         cursor, 1, B, idx_out, *outs, None)
        assert rc == -1 and word in lib.usv_last_error(), (word, rc, lib.usv_last_error())

    for B in (5, 7, 8, 13, 24):                             # M = 12
        refused(b"B must divide n_steps * n", B=B)
    refused(b"B must be > 0", B=0)
    refused(b"B must be > 0", B=-4)
    refused(b"null cursor block", cursor=None)
    for off in (1, 4, 8):
        refused(b"cursor block is not 16-B aligned", cursor=q + off)
    for i in range(6):
        refused(b"null output", outs=tuple(None if j == i else p for j in range(6)))
        refused(b"output is not 4-B aligned", outs=tuple(p + 2 if j == i else p for j in range(6)))
        refused(b"aliases the cursor block", outs=tuple(q if j == i else p for j in range(6)))
    refused(b"idx_out is not 8-B aligned", idx_out=p + 4)
    refused(b"aliases the cursor block", idx_out=q)
    # ... and what usv_rollout_gather refuses
    refused(b"null usv_rollout", null_ro=True)
    refused(b"null usv_rollout_frames", null_fr=True)
    refused(b"must equal obs_width", f=fr(k=2, d=4))
    refused(b"unknown flags", f=fr(flags=2))
    refused(b"null bad_count", f=fr(bad_count=None))
    refused(b"must be > 0", r=ro(n=0))
    refused(b"null buffer", r=ro(start=None))
    refused(b"null buffer", r=ro(obs=None), f=fr(frames=None))      # full storage needs obs


def test_python_paths_that_need_no_device():
    import gym_usv_amd
    from gym_usv_amd import rollout
    assert gym_usv_amd.RolloutSampler is rollout.RolloutSampler and "RolloutSampler" in gym_usv_amd.__all__
    ro = types.SimpleNamespace(n_steps=8, n=64, lib=None, device=None)
    for bad in (0, -1, 100, 1024, 2 ** 31):                 # 512 samples
        with pytest.raises(ValueError):
            rollout.RolloutSampler(ro, bad, 1)
    with pytest.raises(ValueError):
        rollout.DeviceRollout.sampler(ro, 100, 1)           # what ro.sampler(...) calls

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import ppo_torch
    flags = dict(fused=True, sde_kernel=True, eval_kernel=True, adam_kernel=True, loss_kernel=True, perm_kernel=True)
    quiet = dict(envs=64, updates=1, n_steps=8, batch_size=128, log=lambda s: None)
    for off in flags:
        with pytest.raises(ValueError, match="--graph"):
            ppo_torch.train(graph=True, **quiet, **dict(flags, **{off: False}))
    for test_mode in ("check_eval", "check_loss"):
        with pytest.raises(ValueError, match="--graph"):
            ppo_torch.train(graph=True, **quiet, **dict(flags, **{test_mode: True}))
    with pytest.raises(ValueError, match="fused"):
        ppo_torch.train(perm_kernel=True, **quiet)
    with pytest.raises(ValueError, match="divides"):
        ppo_torch.train(perm_kernel=True, fused=True, **dict(quiet, batch_size=100))
    ppo_torch.check_graph_args(False, *(False,) * 8)        # without --graph nothing is asked
    ppo_torch.check_graph_args(True, *(True,) * 6, False, False)
