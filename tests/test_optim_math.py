"""The fused optimizer step without a GPU: the arithmetic and the summation order of gym-usv_amd/csrc/usv_optim_math.hpp
through a stand-alone host program built with AddressSanitizer and UBSan, compared bit for bit with the NumPy
restatement (tests/optim_ref.py); the restatement against torch-CPU float64 clip_grad_norm_ + Adam under the 1e-5
ceiling and under 4x the maximum this program measured, MEASURED below (4x is the project's standing allowance for
other inputs); the argument refusals of the new C entries; and the DeviceAdam ValueErrors that need no device."""
import ctypes
import subprocess

import numpy as np
import pytest

import optim_ref as R

# the largest normalised errors of the float64 comparison below (printed by the test), rounded up
MEASURED = {"p": 4.64e-7, "m": 5.87e-8, "v": 4.00e-7, "total": 1.34e-7}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}

MAIN = r"""
#include <cstdio>
#include <vector>
#include "usv_optim_math.hpp"
using namespace usv;

// stdin, repeated until the end of the input: a header of 3 int64 (n tensors, step, flags: 1 clip), 5 f64 (lr, beta1,
// beta2, eps, max_norm), n int64 numels, then per tensor p g m v [numel] f32 each.
// stdout: per tensor p' m' v' [numel], then total (with clipping).
// m and v pass through two flat buffers laid out by optim_state_floats, as the kernels' are.
int main() {
  int64_t h[3];
  while (std::fread(h, 8, 3, stdin) == 3) {
    const int64_t n = h[0], t = h[1];
    const bool clip = (h[2] & 1) != 0;
    double d[5];
    if (n < 1 || t < 1 || std::fread(d, 8, 5, stdin) != 5) return 3;
    if (!adam_rate_ok(d[0]) || !adam_rate_ok(d[3]) || !adam_beta_ok(d[1]) || !adam_beta_ok(d[2])) return 4;
    std::vector<int64_t> numel(n), at(n);
    if (std::fread(numel.data(), 8, n, stdin) != (size_t)n) return 3;
    int64_t state = 0, chunks = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (numel[i] < 1) return 4;
      at[i] = state;
      state += optim_state_floats(numel[i]);
      chunks += optim_chunks(numel[i]);
    }
    std::vector<std::vector<float>> p(n), g(n);
    std::vector<float> m(state), v(state);
    for (int64_t i = 0; i < n; ++i) {
      p[i].resize(numel[i]), g[i].resize(numel[i]);
      const size_t c = (size_t)numel[i];
      if (std::fread(p[i].data(), 4, c, stdin) != c || std::fread(g[i].data(), 4, c, stdin) != c ||
          std::fread(m.data() + at[i], 4, c, stdin) != c || std::fread(v.data() + at[i], 4, c, stdin) != c) return 3;
    }
    const AdamScalars s = adam_scalars(t, d[0], d[1], d[2], d[3]);
    float total = 0.0f, coef = 1.0f;
    if (clip) {
      float acc = 0.0f;
      for (int64_t i = 0; i < n; ++i) acc = optim_tensor_sqsum(acc, g[i].data(), numel[i]);
      total = optim_norm(acc);
      coef = adam_clip_coef(total, (float)d[4]);
    }
    for (int64_t i = 0; i < n; ++i) {
      for (int64_t e = 0; e < numel[i]; ++e)
        adam_value(p[i][e], m[at[i] + e], v[at[i] + e], clip ? adam_clipped(g[i][e], coef) : g[i][e], s);
      std::fwrite(p[i].data(), 4, numel[i], stdout);
      std::fwrite(m.data() + at[i], 4, numel[i], stdout);
      std::fwrite(v.data() + at[i], 4, numel[i], stdout);
    }
    if (clip) std::fwrite(&total, 4, 1, stdout);
    if (optim_scratch_floats(chunks) != (size_t)(kOptimScratchHead + chunks)) return 5;
  }
  std::fprintf(stderr, "C %d strands %d groups %d state %lld %lld %lld\n", kOptimChunk, kOptimStrands, kOptimStrandGroups,
               (long long)optim_state_floats(1), (long long)optim_state_floats(4), (long long)optim_state_floats(4097));
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program with AddressSanitizer + UBSan: a stand-alone host binary, run directly."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("optim_math")
    src, exe = d / "optim.cpp", d / "optim_san"
    src.write_text(MAIN)
    subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g", f"-I{CSRC}",
                    "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


def run(exe, cases):
    """`cases`: [(tensors (p, g, m, v lists), t, max_norm or None)]; one run.  Returns [(p', m', v', total)]."""
    parts = []
    for (ps, gs, ms, vs), t, max_norm in cases:
        parts.append(np.array([len(ps), t, int(max_norm is not None)], np.int64))
        parts.append(np.array([R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"], R.HYPER["eps"],
                               0.0 if max_norm is None else max_norm], np.float64))
        parts.append(np.array([len(p) for p in ps], np.int64))
        for quad in zip(ps, gs, ms, vs):
            parts += [np.ascontiguousarray(x, np.float32) for x in quad]
    p = subprocess.run([exe], input=b"".join(x.tobytes() for x in parts), capture_output=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    assert p.stderr.decode().strip() == f"C {R.C} strands {R.STRANDS} groups 4 state 4 4 4100"
    out, at = [], 0
    for (ps, *_), _, max_norm in cases:
        po, mo, vo = [], [], []
        for x in ps:
            for dst in (po, mo, vo):
                dst.append(np.frombuffer(p.stdout, np.float32, len(x), at))
                at += 4 * len(x)
        total = None
        if max_norm is not None:
            total = np.frombuffer(p.stdout, np.float32, 1, at)[0]
            at += 4
        out.append((po, mo, vo, total))
    assert at == len(p.stdout)
    return out


def same_step(got, want):
    return all(R.same(np.concatenate(a), np.concatenate(b)) for a, b in zip(got[:3], want[:3])) and \
        ((got[3] is None and want[3] is None) or R.same([got[3]], [want[3]]))


LISTS = [(n,) for n in R.NUMELS] + [R.NUMELS, R.MANY, (R.BIG,)]
BITES, SPARES = 1e-3, 1e6                                 # max_norms below and above every list's norm


def test_lists_are_what_they_should_be():
    assert len(R.MANY) == 130 > R.K and set(R.MANY) == set(range(1, 8))
    assert R.chunks((R.BIG,)) == 66 and R.state_offsets((1, 5, 4))[0] == [0, 4, 12]


def test_steps_equal_the_restatement_bitwise(program):
    cases = [(R.inputs(numels, seed=t), t, mn) for numels in LISTS for t in R.STEPS for mn in (BITES, SPARES, None)]
    bit = spared = 0
    for (x, t, mn), got in zip(cases, run(program, cases)):
        want = R.step(*x, t, max_norm=mn)
        assert same_step(got, want), ([len(p) for p in x[0]][:4], t, mn)
        if mn is not None:
            bit += want[3] > mn
            spared += want[3] < mn
            assert (want[3] > BITES) and (want[3] < SPARES)
    assert bit == spared == len(cases) // 3


def test_inf_and_nan_gradients_are_not_special_cased(program):
    cases = [(R.inputs(numels, bad=bad), 2, mn) for numels in (R.NUMELS, (R.BIG,), (5,))
             for bad in (np.inf, np.nan) for mn in (BITES, None)]
    for (x, t, mn), got in zip(cases, run(program, cases)):
        want = R.step(*x, t, max_norm=mn)
        assert same_step(got, want)
        bad = x[1][len(x[1]) // 2][len(x[1][len(x[1]) // 2]) // 2]
        p_all = np.concatenate(got[0])
        if mn is None:                                    # the element alone is lost
            assert np.isnan(p_all).sum() == 1
        elif np.isinf(bad):                               # coef = 0: 0 * inf is NaN there, the others step on g' = 0
            assert got[3] == np.inf and np.isnan(p_all).sum() == 1
        else:                                             # a NaN norm reaches every element
            assert np.isnan(got[3]) and np.isnan(p_all).all()


def test_the_sum_is_the_fixed_order_and_not_a_sequential_one(program):
    """Cases whose sequential float32 sum of squares gives another norm than the chunk-strand-tree one (four seeds, so
    that the two do not agree by chance in all): the program gives the latter in every one."""
    numels = (2 * R.C + 1, 7)
    cases = [(R.inputs(numels, seed=11 + j), 1, SPARES) for j in range(4)]
    differ = 0
    for (x, _, _), got in zip(cases, run(program, cases)):
        seq = np.float32(0.0)
        for g in np.concatenate(x[1]):
            seq = seq + g * g
        assert R.same([got[3]], [R.total_norm(x[1])])
        differ += not R.same([np.sqrt(seq)], [got[3]])
    assert differ > 0


def test_the_restatement_is_within_the_bounds_of_the_definition():
    """The float32 order against torch-CPU float64 clip_grad_norm_ + Adam, one step from the same state, errors over
    the sums of magnitudes; gradients scaled per tensor by 10^-4 .. 10^0."""
    worst = {}
    scale = lambda i: 10.0 ** -(i % 5)                    # noqa: E731
    for numels in (R.NUMELS, R.MANY, (R.BIG,)):
        for t in (1, 10, 1000):
            for mn in (0.5, SPARES, None):
                x = R.inputs(numels, seed=100 + t, scale=scale)
                err = R.errors(R.step(*x, t, max_norm=mn), R.torch_step(*x, t, max_norm=mn), R.scales(*x, t, max_norm=mn))
                for k, v in err.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(worst)
    assert set(worst) == set(BOUND)
    for k, v in worst.items():
        assert np.isfinite(v) and v < R.CEILING and v <= BOUND[k], (k, v, BOUND[k])


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_entries_refuse_bad_arguments_without_gpu(lib):
    """Everything usv_adam_step can refuse before a HIP call is refused with USV_ERR_ARG and a message."""
    from gym_usv_amd import _lib
    assert _lib.ABI_VERSION == 5 == lib.usv_abi_version()
    buf = (ctypes.c_uint8 * 512)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    T = _lib.UsvAdamTensor
    assert ctypes.sizeof(T) == 24

    def refused(word, tensors, n=None, m=p, v=p, state=1 << 20, step=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, mg=0.5,
                scratch=p, scratch_floats=1 << 20, norm=p):
        arr = (T * len(tensors))(*tensors) if tensors is not None else None
        rc = lib.usv_adam_step(arr, len(tensors) if n is None else n, m, v, state, step, lr, b1, b2, eps, mg, scratch,
                               scratch_floats, norm, None)
        assert rc == -1 and word in lib.usv_last_error(), (word, rc, lib.usv_last_error())

    good = [T(p, p + 64, 8)]
    refused(b"null tensors", None, n=1)
    refused(b"n must be >= 1", good, n=0)
    refused(b"n must be >= 1", good, n=-3)
    refused(b"numel must be >= 0", [T(p, p + 64, -1)])
    refused(b"null param or grad", [T(None, p, 8)])
    refused(b"null param or grad", good + [T(p, None, 8)])
    refused(b"not 4-B aligned", [T(p + 2, p + 64, 8)])
    refused(b"not 4-B aligned", [T(p, p + 65, 8)])
    refused(b"same address", good + [T(p + 32, p + 32, 8)])
    for step in (0, -1):
        refused(b"step must be >= 1", good, step=step)
    for bad in (-1e-9, float("nan"), float("inf")):
        refused(b"lr must be finite", good, lr=bad)
        refused(b"eps must be finite", good, eps=bad)
    for bad in (-1e-9, 1.0, 1.5, float("nan")):
        refused(b"betas must be in [0, 1)", good, b1=bad)
        refused(b"betas must be in [0, 1)", good, b2=bad)
    refused(b"max_grad_norm is NaN", good, mg=float("nan"))
    refused(b"clipping needs norm_out", good, norm=None)
    refused(b"null state", good, m=None)
    refused(b"null state", good, v=None)
    refused(b"clipping needs scratch", good, scratch=None)
    refused(b"state is too small", good, state=7)
    refused(b"scratch is too small", good, scratch_floats=4)
    refused(b"not 16-B aligned", good, m=p + 4)
    refused(b"not 16-B aligned", good, v=p + 8)
    refused(b"not 16-B aligned", good, scratch=p + 4)
    refused(b"not 4-B aligned", good, norm=p + 2)
    refused(b"2^31 - 1 chunks", [T(p, p + 64, (1 << 31) * R.C)])
    # (a buffer on another device is refused by a HIP call: not here)
    # the sizes: each segment padded to four floats; the ticket's four floats and one per chunk of C; zero-element
    # tensors are skipped, unread
    arr = (T * 3)(T(p, p + 64, 2 * R.C + 3), T(None, None, 0), T(p, p + 64, 1))
    assert lib.usv_adam_state_floats(arr, 3) == 2 * R.C + 4 + 4
    assert lib.usv_adam_scratch_floats(arr, 3) == 4 + 3 + 1
    assert lib.usv_adam_state_floats(arr, 0) == 0 == lib.usv_adam_scratch_floats(arr, 0)
    assert lib.usv_adam_state_floats((T * 1)(T(p, p, -2)), 1) == 0
    none = (T * 1)(T(None, None, 0))
    assert lib.usv_adam_step(none, 1, p, p, 0, 1, 1e-3, 0.9, 0.999, 1e-8, -1.0, None, 0, None, None) == 0   # no launch


def test_python_checks_need_no_device():
    import torch
    import gym_usv_amd
    from gym_usv_amd import optim
    assert gym_usv_amd.DeviceAdam is optim.DeviceAdam and "DeviceAdam" in gym_usv_amd.__all__
    a = torch.zeros(3, 4)
    for params in ([], [a.double()], [a.t()], [a, a.half()], [3.0], [a]):      # the last: float32, but on the CPU
        with pytest.raises(ValueError):
            optim.DeviceAdam(params)
    for kw in (dict(lr=-1e-3), dict(lr=float("nan")), dict(eps=-1.0), dict(eps=float("inf")), dict(betas=(1.0, 0.999)),
               dict(betas=(0.9, -0.1)), dict(betas=(float("nan"), 0.5)), dict(max_grad_norm=-0.5),
               dict(max_grad_norm=float("nan"))):
        with pytest.raises(ValueError):
            optim._check_hyper(**{**dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None), **kw})
    assert optim._check_hyper(3e-4, (0.9, 0.999), 1e-8, None) == (3e-4, (0.9, 0.999), 1e-8, -1.0)
    assert optim._check_hyper(3e-4, (0.0, 0.5), 0.0, 0)[3] == 0.0
