"""The mirrored frame ring of the fused wrappers (gym-usv_amd/csrc/usv_wrap_layout.hpp) and the shape
checks of usv_wrap_step / usv_wrap_reset, without a GPU.

usv_wrap_layout.hpp is plain host C++: a stand-alone program replays a scripted sequence (per-step obs and
done masks) on host arrays using ONLY the header's index functions, and dumps every step's window.  The
expected windows are SB3's StackedObservations (stable_baselines3/common/vec_env/stacked_observations.py,
channels-last, 1-D obs) restated in NumPy below; the comparison is bitwise.
"""
import ctypes
import subprocess

import numpy as np
import pytest

KS, DS, N = (1, 2, 5), (1, 6, 143), 7


class NpFrameStack:
    """StackedObservations: reset = zeros with the obs last; update = roll by one obs, zero the done
    envs' stacks, write the new obs last."""

    def __init__(self, n, d, k):
        self.s = np.zeros((n, k * d), np.float32)
        self.d = d

    def reset(self, obs):
        self.s[...] = 0
        self.s[:, -self.d:] = obs
        return self.s.copy()

    def update(self, obs, dones):
        self.s = np.roll(self.s, -self.d, axis=-1)
        self.s[dones] = 0
        self.s[:, -self.d:] = obs
        return self.s.copy()


def steps_of(k):
    return 3 * k + 2                                 # the ring wraps three times


def script(k, d):
    """obs [T + 1, N, d] (obs[0] is the reset obs) and done [T, N]: env 0 never done, env 1 done at step
    0, env 2 done on consecutive steps (1, 2, 3), env 3 done every step, the others at random."""
    T = steps_of(k)
    rng = np.random.default_rng(1000 * k + d)
    obs = rng.standard_normal((T + 1, N, d)).astype(np.float32)
    done = rng.random((T, N)) < 0.25
    done[:, 0] = False
    done[0, 1] = True
    done[:, 2] = False
    done[1:4, 2] = True
    done[:, 3] = True
    return obs, done


MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "usv_wrap_layout.hpp"
using namespace usv;

// argv: k D N T; stdin: obs [T + 1][N][D] f32 then done [T][N] u8; stdout: per frame counter j = 0 .. T the
// windows [N][k D] f32; stderr line "S stride slots maxidx bad" (bad = writes outside [0, stride)).
static size_t g_max = 0, g_bad = 0;
static void put(std::vector<float>& row, size_t stride, size_t i, float v) {
  if (i > g_max) g_max = i;
  if (i >= stride) { ++g_bad; return; }
  row[i] = v;
}
static void restart(std::vector<float>& row, size_t stride, int64_t j, int k, int D) {
  for (int q = 0; q < wrap_ring_slots(k); ++q)
    if (wrap_clears_slot(j, k, q))
      for (int c = 0; c < D; ++c) put(row, stride, (size_t)q * D + c, 0.0f);
}
static void push(std::vector<float>& row, size_t stride, int64_t j, int k, int D, const float* o) {
  for (int c = 0; c < D; ++c) put(row, stride, (size_t)wrap_slot(j, k) * D + c, o[c]);
  if (wrap_mirror_slot(j, k) >= 0)
    for (int c = 0; c < D; ++c) put(row, stride, (size_t)wrap_mirror_slot(j, k) * D + c, o[c]);
}
int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int k = std::atoi(argv[1]), D = std::atoi(argv[2]), N = std::atoi(argv[3]), T = std::atoi(argv[4]);
  std::vector<float> obs((size_t)(T + 1) * N * D);
  std::vector<unsigned char> done((size_t)T * N);
  if (std::fread(obs.data(), 4, obs.size(), stdin) != obs.size()) return 3;
  if (std::fread(done.data(), 1, done.size(), stdin) != done.size()) return 3;
  const size_t stride = wrap_ring_stride(D, k);
  // rows start as garbage: everything a window shows must have been written
  std::vector<std::vector<float>> ring(N, std::vector<float>(stride, -12345.0f));
  for (int64_t j = 0; j <= T; ++j) {
    for (int e = 0; e < N; ++e) {
      if (j == 0 || done[(size_t)(j - 1) * N + e]) restart(ring[e], stride, j, k, D);
      push(ring[e], stride, j, k, D, &obs[((size_t)j * N + e) * D]);
      const size_t off = wrap_window_offset(D, k, j);
      if (off + (size_t)k * D > stride) { ++g_bad; continue; }
      std::fwrite(ring[e].data() + off, 4, (size_t)k * D, stdout);
    }
  }
  std::fprintf(stderr, "S %zu %d %zu %zu\n", stride, wrap_ring_slots(k), g_max, g_bad);
  return g_bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """The replay program, plain and with AddressSanitizer + UBSan (both stand-alone host binaries)."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("wrap_layout")
    src = d / "replay.cpp"
    src.write_text(MAIN)
    out = {}
    for name, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / f"replay_{name}"
        subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", *flags, f"-I{CSRC}", "-o", str(exe),
                        str(src)], check=True)
        out[name] = str(exe)
    return out


def replay(exe, k, d):
    obs, done = script(k, d)
    T = steps_of(k)
    p = subprocess.run([exe, str(k), str(d), str(N), str(T)], input=obs.tobytes() + done.astype(np.uint8).tobytes(),
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    stride, slots, max_idx, bad = (int(x) for x in p.stderr.decode().split("S ", 1)[1].split())
    win = np.frombuffer(p.stdout, dtype=np.float32).reshape(T + 1, N, k * d)
    return win, stride, slots, max_idx, bad


def expected(k, d):
    obs, done = script(k, d)
    st = NpFrameStack(N, d, k)
    out = [st.reset(obs[0])]
    for t in range(steps_of(k)):
        out.append(st.update(obs[t + 1], done[t]))
    return np.stack(out)


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("build", ["plain", "san"])
def test_ring_windows_equal_stacked_observations(programs, build, k, d):
    """Every step's window of the ring, bitwise, against StackedObservations; no write index outside
    [0, stride); the stride holds 2k - 1 slots and is a multiple of 4 floats.  `san` is the same program
    under AddressSanitizer and UBSan, run directly."""
    win, stride, slots, max_idx, bad = replay(programs[build], k, d)
    assert bad == 0 and max_idx < stride
    assert slots == 2 * k - 1 and stride == (slots * d + 3) // 4 * 4
    assert max_idx == slots * d - 1                     # the last slot is used, the padding never
    want = expected(k, d)
    assert win.shape == want.shape
    assert np.array_equal(win.view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_library_queries_agree_with_the_header(programs, lib):
    """usv_wrap_ring_stride / usv_wrap_window_offset of the built library = the header program's values
    (the offset: where the newest frame sits, found in the replayed windows' source ring by value)."""
    for k in KS:
        for d in DS:
            _, stride, slots, _, _ = replay(programs["plain"], k, d)
            assert lib.usv_wrap_ring_stride(d, k) == stride
            for j in range(3 * k + 2):
                assert lib.usv_wrap_window_offset(d, k, j) == ((j + 1) % k) * d
                assert lib.usv_wrap_window_offset(d, k, j) + k * d <= stride
    assert lib.usv_wrap_ring_stride(0, 5) == 0 and lib.usv_wrap_ring_stride(143, 0) == 0
    assert lib.usv_wrap_ring_stride(143, 5) == 1288     # 9 slots of 143 floats, rounded up to 4


def test_wrap_calls_refuse_bad_shapes_without_gpu(lib):
    """n <= 0, obs_dim <= 0, n_stack < 1 and a NULL ring are refused with USV_ERR_ARG and a message before
    any HIP call (so also on a machine without a GPU)."""
    from gym_usv_amd import _lib
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)

    def wrap(**kw):
        f = dict(n=4, obs_dim=6, n_stack=2, reward_bytes=4, ring=p, ep_ret=p, ep_len=p, episode=None,
                 cum_ret=None, cum_len=None, cum_eps=None)
        f.update(kw)
        return _lib.UsvWrap(**f)

    for kw in (dict(n=0), dict(n=-3), dict(obs_dim=0), dict(obs_dim=-1), dict(n_stack=0), dict(n_stack=-2),
               dict(ring=None)):
        w = wrap(**kw)
        assert lib.usv_wrap_step(ctypes.byref(w), 1, p, p, p, None, None, None) == -1, kw
        msg = lib.usv_last_error()
        assert b"usv_wrap" in msg and (b"ring" in msg if "ring" in kw else b"n_stack" in msg), (kw, msg)
        assert lib.usv_wrap_reset(ctypes.byref(w), 0, None, p, None) == -1, kw
        assert b"usv_wrap" in lib.usv_last_error(), kw
    assert lib.usv_wrap_step(None, 1, p, p, p, None, None, None) == -1
    assert lib.usv_wrap_reset(None, 0, None, p, None) == -1
    w = wrap()
    assert lib.usv_wrap_step(ctypes.byref(w), -1, p, p, p, None, None, None) == -1     # j < 0
    assert lib.usv_wrap_step(ctypes.byref(w), 1, None, p, p, None, None, None) == -1   # no obs
    assert lib.usv_wrap_step(ctypes.byref(wrap(reward_bytes=2)), 1, p, p, p, None, None, None) == -1
    assert lib.usv_wrap_step(ctypes.byref(wrap(flags=2)), 1, p, p, p, None, None, None) == -1     # unknown flag
    assert b"flags" in lib.usv_last_error()
    assert ctypes.sizeof(_lib.UsvWrap) == 80


def test_fused_adapter_needs_the_gpu_library():
    """Sb3VecEnv(fused=True) over a CPU venv raises UsvLibError (no CPU fallback); the default does not."""
    import torch
    import gym_usv_amd
    from gym_usv_amd.sb3 import DeviceFrameStack, Sb3VecEnv
    from gym_usv_amd.spaces import Box

    class Venv:
        num_envs, obs_dim, act_dim = 4, 6, 2
        device = torch.device("cpu")
        single_observation_space = Box(-1, 1, shape=(6,))
        single_action_space = Box(-1, 1, shape=(2,))

    with pytest.raises(gym_usv_amd.UsvLibError):
        Sb3VecEnv(venv=Venv(), frame_stack=5, fused=True)
    assert isinstance(Sb3VecEnv(venv=Venv(), frame_stack=5)._stack, DeviceFrameStack)
