"""The device-resident counters without a GPU: the step-scalar formula of usv_adam_step_dev's clock block
(adam_clock_scalars, gym-usv_amd/csrc/usv_optim_math.hpp) and the counter's wrap through a stand-alone host program
built with AddressSanitizer and UBSan, compared with the host's adam_scalars and with tests/optim_ref.py's restatement;
the argument refusals of the new C entries, which are reached before any HIP call; and the ValueError / RuntimeError
paths of the capturable classes that need no device."""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest

import optim_ref as R

STEPS = tuple(range(1, 2049)) + (10 ** 4, 10 ** 5, 10 ** 6, 2 ** 31)
BETAS = ((0.9, 0.999), (0.0, 0.0), (0.5, 0.9999))
LRS = (3e-4, 1e-4)
EPS = 1e-8
ULPS = 1            # a double pow that is off in its last place moves the float32 cast by at most one ulp
# cases of the sweep in which the formula's step_size or bc2_sqrt is not bit-equal to adam_scalars' (printed by the
# test): on the host the two run the same libm, the device's pow is another library (tests/test_gpu_graph.py)
MEASURED = {"differing": 0, "cases": len(STEPS) * len(BETAS) * len(LRS)}

MAIN = r"""
#include <cstdio>
#include "usv_optim_math.hpp"
using namespace usv;

// stdin, repeated until the end of the input: int64 t, then f64 lr, beta1, beta2, eps.
// stdout per case: 4 f32: adam_scalars' step_size and bc2_sqrt, then adam_clock_scalars'.
int main() {
  static_assert(sizeof(AdamClock) == 32 && alignof(AdamClock) == 16, "the clock block");
  int64_t t;
  while (std::fread(&t, 8, 1, stdin) == 1) {
    double d[4];
    if (t < 1 || std::fread(d, 8, 4, stdin) != 4) return 3;
    if (!adam_rate_ok(d[0]) || !adam_rate_ok(d[3]) || !adam_beta_ok(d[1]) || !adam_beta_ok(d[2])) return 4;
    const AdamScalars s = adam_scalars(t, d[0], d[1], d[2], d[3]);
    float out[4] = {s.step_size, s.bc2_sqrt, 0.0f, 0.0f};
    adam_clock_scalars(t, d[0], d[1], d[2], out[2], out[3]);
    std::fwrite(out, 4, 4, stdout);
  }
  std::fprintf(stderr, "wrap %u %u %u\n", counter_added(0xFFFFFFFFu, 1u), counter_added(0xFFFFFFFEu, 3u),
               counter_added(7u, 0u));
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program with AddressSanitizer + UBSan: a stand-alone host binary, run directly."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("clock_math")
    src, exe = d / "clock.cpp", d / "clock_san"
    src.write_text(MAIN)
    subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g", f"-I{CSRC}",
                    "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


def ulps(a, b):
    """The distance of two arrays of positive finite float32 in units in the last place."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (a > 0).all() and (b > 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_step_scalars_equal_the_hosts_within_one_ulp_and_the_counter_wraps(program):
    cases = list(itertools.product(STEPS, BETAS, LRS))
    assert len(cases) == MEASURED["cases"]
    data = b"".join(np.array([t], np.int64).tobytes() + np.array([lr, b1, b2, EPS], np.float64).tobytes()
                    for t, (b1, b2), lr in cases)
    p = subprocess.run([program], input=data, capture_output=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    assert p.stderr.decode().strip() == "wrap 0 1 7"        # 0xFFFFFFFF + 1 = 0
    out = np.frombuffer(p.stdout, np.float32).reshape(len(cases), 4)
    host, dev = out[:, :2], out[:, 2:]
    d = ulps(host, dev)
    differing = int((d.max(axis=1) > 0).sum())
    print(f"clock formula against adam_scalars: {differing} of {len(cases)} cases differ, at most {int(d.max())} ulp")
    assert d.max() <= ULPS
    assert differing == MEASURED["differing"]
    # ... and adam_scalars is what the restatement's Python doubles give, so the GPU test may feed either
    for (t, (b1, b2), lr), h in zip(cases, host):
        s = R.scalars(t, lr, b1, b2, EPS)
        assert ulps([s["step_size"], s["bc2_sqrt"]], h).max() <= ULPS, (t, b1, b2, lr)


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_new_entries_refuse_bad_arguments_without_gpu(lib):
    """A NULL clock, epoch or counter pointer, a misaligned one and a clock block that is too small are refused with
    USV_ERR_ARG and a message that names them: before the buffers' device is asked for, so before any HIP call."""
    from gym_usv_amd import _lib
    buf = (ctypes.c_uint8 * 512)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    T = _lib.UsvAdamTensor
    clock_bytes = lib.usv_adam_clock_bytes()
    assert clock_bytes == 32

    def refused(word, rc):
        assert rc == -1 and word in lib.usv_last_error(), (word, rc, lib.usv_last_error())

    good = (T * 1)(T(p, p + 64, 8))
    adam = lambda clock, nbytes, n=1: lib.usv_adam_step_dev(good, n, p, p, 1 << 20, clock, nbytes, 0.9, 0.999, 1e-8,    # noqa: E731
                                                            0.5, p, 1 << 20, p, None)
    refused(b"null clock block", adam(None, clock_bytes))
    refused(b"clock block is not 16-B aligned", adam(p + 8, clock_bytes))
    refused(b"clock block is too small", adam(p, clock_bytes - 1))
    refused(b"clock block is too small", adam(p, 0))
    refused(b"usv_adam_step_dev: n must be >= 1", adam(p, clock_bytes, n=0))      # ... and usv_adam_step's own refusals
    refused(b"usv_adam_step_dev: the betas must be in [0, 1)",
            lib.usv_adam_step_dev(good, 1, p, p, 1 << 20, p, clock_bytes, 1.0, 0.999, 1e-8, 0.5, p, 1 << 20, p, None))

    refused(b"usv_counter_add: null word_dev", lib.usv_counter_add(None, 1, None))
    refused(b"usv_counter_add: word_dev is not 4-B aligned", lib.usv_counter_add(p + 2, 1, None))

    sde = _lib.UsvSde(4, 8, 2, 0, 1, 0, (ctypes.c_float * 4)(-1, -1), (ctypes.c_float * 4)(1, 1))
    s = ctypes.byref(sde)
    calls = {
        "usv_sde_sample_dev": lambda e: lib.usv_sde_sample_dev(s, e, p, p, 8, p, p, p, p, None),
        "usv_sde_weights_dev": lambda e: lib.usv_sde_weights_dev(s, e, p, p, None),
        "usv_sde_squash_forward_dev": lambda e: lib.usv_sde_squash_forward_dev(s, e, p, p, 8, p, p, p, p, p, p, None),
        "usv_sde_squash_backward_dev": lambda e: lib.usv_sde_squash_backward_dev(s, e, p, p, 8, p, p, p, p, p, p, p, 8, p,
                                                                                 p, None),
        "usv_caps_perturb_dev": lambda e: lib.usv_caps_perturb_dev(3, 5, p, p, 0.1, 1, e, None),
    }
    for name, call in calls.items():
        refused(name.encode() + b": null epoch_dev", call(None))
        refused(name.encode() + b": epoch_dev is not 4-B aligned", call(p + 1))
    # ... and with a good word the entry's own refusals come first, as the entry without _dev has them
    sde.latent_dim = 6
    refused(b"latent_dim must be a multiple of 4", calls["usv_sde_sample_dev"](p))
    refused(b"usv_caps_perturb_dev: rows must be >= 1", lib.usv_caps_perturb_dev(0, 5, p, p, 0.1, 1, p, None))

    pair = (_lib.UsvPolyakPair * 1)(_lib.UsvPolyakPair(p, p + 64, 8))
    refused(b"usv_polyak_prepare: null table", lib.usv_polyak_prepare(pair, 1, None, 64))
    refused(b"usv_polyak_prepare: the table is too small", lib.usv_polyak_prepare(pair, 1, p, 8))
    refused(b"usv_polyak_prepare: n_pairs must be >= 1", lib.usv_polyak_prepare(pair, 0, p, 64))


def test_python_paths_that_need_no_device():
    import torch
    import gym_usv_amd
    from gym_usv_amd import graph, optim
    assert gym_usv_amd.capture_step is graph.capture_step and "capture_step" in gym_usv_amd.__all__
    a = torch.zeros(3, 4)
    with pytest.raises(ValueError):
        gym_usv_amd.DeviceAdam([a], capturable=True)          # float32, but on the CPU: no fallback in either form
    for warmup in (0, -1):
        with pytest.raises(ValueError):
            gym_usv_amd.capture_step(lambda: None, warmup=warmup)
    with pytest.raises(RuntimeError):                          # UsvLibError: no CPU fallback
        gym_usv_amd.DeviceSDE(4, 8, 2, "cpu", 1, [-1, -1], [1, 1], capturable=True)
    with pytest.raises(RuntimeError):
        gym_usv_amd.DeviceCAPS("cpu", 1, capturable=True)
    with pytest.raises(ValueError):
        gym_usv_amd.DeviceCAPS("cpu", 1, eps_s=-1.0, capturable=True)
    # the block's layout as optim.py reads it: lr at word 0 as f64, the step at word 1, the two scalars at f32 4 and 5
    block = torch.zeros(4, dtype=torch.int64)
    block[0:1].view(torch.float64).fill_(3e-4)
    block[1:2].fill_(2 ** 31)
    block.view(torch.float32)[4:6] = torch.tensor([0.25, 0.5])
    raw = block.numpy().tobytes()
    assert np.frombuffer(raw, np.float64, 1, 0)[0] == 3e-4 and np.frombuffer(raw, np.int64, 1, 8)[0] == 2 ** 31
    assert tuple(np.frombuffer(raw, np.float32, 2, 16)) == (0.25, 0.5)
    # a word holds a uint32 in an int32 tensor
    from gym_usv_amd import _lib
    w = torch.zeros(1, dtype=torch.int32)
    for v in (0, 1, 2 ** 31 - 1, 2 ** 31, 0xFFFFFFFF, 2 ** 32 + 5):
        _lib.word_write(w, v)
        assert _lib.word_read(w) == v % 2 ** 32
    assert optim._check_hyper(1e-4, (0.0, 0.0), 0.0, None)[0] == 1e-4     # what a capturable lr assignment checks
