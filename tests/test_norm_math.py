"""The arithmetic and the work split of the fused VecNormalize (gym-usv_amd/csrc/usv_norm_math.hpp) and
the argument checks of usv_wrap_step_norm / usv_wrap_reset_norm, without a GPU.

usv_norm_math.hpp is plain C++: a stand-alone program that includes nothing else replays the kernels'
work split and combination order (chunk -> wave groups -> wave order -> the finalising tree -> the
merge) on host arrays over a scripted [T, N, D] sequence and dumps the running statistics after every
step.  They are compared with SB3's RunningMeanStd / VecNormalize restated in NumPy
(tests/vecnormalize_ref.py) at bounds derived from the arithmetic, not measured:
  f64 mean of n terms, combined in another order than NumPy's   2 n 2^-53 max|x|
  variance                                                      8 n 2^-53 max|x|^2
  running statistics after t updates                            t times these
(n = 257, |x| <= 10: 6e-13 and 2e-11; an indexing or merge bug is many orders larger.)
"""
import ctypes
import subprocess

import numpy as np
import pytest

import vecnormalize_ref as R

T = 6
GAMMA, EPS = 0.99, 1e-8
EDGES, THREE = R.edge_sizes()
NS = EDGES + [THREE]
DS = (1, 3, 6, 143)

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "usv_norm_math.hpp"
using namespace usv;

// argv: N D T gamma; stdin: obs [T][N][D] f32, rew [T][N] f32, done [T][N] u8.  Every step is
// usv_wrap_step_norm's statistics side with training, norm_obs and norm_reward on.  stdout, per step, f64:
// batch mean [D + 1], batch M2 [D + 1] (column D: the returns), obs_mean [D], obs_var [D], obs_count,
// ret_mean, ret_var, ret_count, returns [N] (after the done envs' were zeroed).
// stderr: "C group_rows block_rows partials chunk_rows".
template <typename F>
static NormMoments column(int64_t N, F x) {               // x(row) -> double
  const int P = norm_num_partials(N);
  std::vector<NormMoments> part(P);
  for (int b = 0; b < P; ++b) {                           // norm_moments_kernel, block b
    NormMoments acc[kNormWaves];
    for (int w = 0; w < kNormWaves; ++w) acc[w] = NormMoments{0.0, 0.0, 0.0};
    for (int gi = 0; gi < norm_chunk_groups(N); ++gi) {
      const int nr = norm_group_rows(N, b, gi);
      if (nr <= 0) break;
      const int64_t r0 = norm_group_begin(N, b, gi);
      NormMoments g{0.0, 0.0, 0.0};
      for (int i = 0; i < nr; ++i) norm_group_add(g, x(r0 + i), i);
      NormMoments& a = acc[norm_group_wave(gi)];
      a = norm_combine(a, g);
    }
    NormMoments t = acc[0];
    for (int w = 1; w < kNormWaves; ++w) t = norm_combine(t, acc[w]);
    if (t.n != (double)(norm_chunk_end(N, b) - norm_chunk_begin(N, b))) std::exit(4);
    part[b] = t;
  }
  NormMoments lane[kNormLanes];                            // norm_finalise_kernel
  for (int l = 0; l < kNormLanes; ++l) {
    int p0, p1;
    norm_final_run(P, l, &p0, &p1);
    NormMoments m{0.0, 0.0, 0.0};
    for (int p = p0; p < p1; ++p) m = norm_combine(m, part[p]);
    lane[l] = m;
  }
  for (int s = 1; s < kNormLanes; s <<= 1)
    for (int l = 0; l < kNormLanes; ++l)
      if ((l & (2 * s - 1)) == 0) lane[l] = norm_combine(lane[l], lane[l + s]);
  return lane[0];
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int64_t N = std::atoll(argv[1]);
  const int D = std::atoi(argv[2]), T = std::atoi(argv[3]);
  const double gamma = std::atof(argv[4]);
  std::vector<float> obs((size_t)T * N * D), rew((size_t)T * N);
  std::vector<unsigned char> done((size_t)T * N);
  if (std::fread(obs.data(), 4, obs.size(), stdin) != obs.size()) return 3;
  if (std::fread(rew.data(), 4, rew.size(), stdin) != rew.size()) return 3;
  if (std::fread(done.data(), 1, done.size(), stdin) != done.size()) return 3;
  std::vector<double> mean(D, 0.0), var(D, 1.0), returns(N, 0.0), bm(D + 1), b2(D + 1);
  double count = 1e-4, rmean = 0.0, rvar = 1.0, rcount = 1e-4;
  for (int t = 0; t < T; ++t) {
    const float* o = &obs[(size_t)t * N * D];
    for (int c = 0; c < D; ++c) {
      const NormMoments m = column(N, [&](int64_t r) { return (double)o[(size_t)r * D + c]; });
      bm[c] = m.mean;
      b2[c] = m.m2;
      norm_merge(mean[c], var[c], count, m);
    }
    count = norm_count_after(count, (double)N);
    for (int64_t e = 0; e < N; ++e) returns[e] = norm_discount(returns[e], gamma, (double)rew[(size_t)t * N + e]);
    const NormMoments m = column(N, [&](int64_t r) { return returns[r]; });
    bm[D] = m.mean;
    b2[D] = m.m2;
    norm_merge(rmean, rvar, rcount, m);
    rcount = norm_count_after(rcount, (double)N);
    for (int64_t e = 0; e < N; ++e)
      if (done[(size_t)t * N + e]) returns[e] = 0.0;
    std::fwrite(bm.data(), 8, D + 1, stdout);
    std::fwrite(b2.data(), 8, D + 1, stdout);
    std::fwrite(mean.data(), 8, D, stdout);
    std::fwrite(var.data(), 8, D, stdout);
    const double tail[4] = {count, rmean, rvar, rcount};
    std::fwrite(tail, 8, 4, stdout);
    std::fwrite(returns.data(), 8, N, stdout);
  }
  std::fprintf(stderr, "C %d %d %d %d\n", kNormGroupRows, kNormBlockRows, norm_num_partials(N), norm_chunk_rows(N));
  return 0;
}
"""


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """The replay program, plain and with AddressSanitizer + UBSan (both stand-alone host binaries)."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("norm_math")
    src = d / "replay.cpp"
    src.write_text(MAIN)
    out = {}
    for name, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / f"replay_{name}"
        subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", *flags, f"-I{CSRC}", "-o", str(exe),
                        str(src)], check=True)
        out[name] = str(exe)
    return out


def special_columns(d):
    """column -> kind, leaving column 0 ordinary: the last columns are constant / all 1.0 / mean 5 with
    spread 1e-3, as many as fit."""
    kinds = ("const", "ones", "tight")
    return {d - 1 - i: kinds[i] for i in range(min(3, d - 1))}


def script(n, d, special=None):
    rng = np.random.default_rng(7000 + 10 * n + d)
    obs = np.clip(rng.standard_normal((T, n, d)) * 2.5, -10, 10).astype(np.float32)
    for c, kind in (special_columns(d) if special is None else special).items():
        if kind == "const":
            obs[:, :, c] = np.float32(-3.7)
        elif kind == "ones":
            obs[:, :, c] = 1.0                           # the sensors under ignore_obstacles
        else:
            obs[:, :, c] = (5 + 1e-3 * rng.standard_normal((T, n))).astype(np.float32)
    rew = rng.standard_normal((T, n)).astype(np.float32)
    done = rng.random((T, n)) < 0.25
    return obs, rew, done


def replay(exe, n, d, obs, rew, done):
    p = subprocess.run([exe, str(n), str(d), str(T), repr(GAMMA)],
                       input=obs.tobytes() + rew.tobytes() + done.astype(np.uint8).tobytes(), capture_output=True,
                       timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    consts = [int(x) for x in p.stderr.decode().split("C ", 1)[1].split()]
    a = np.frombuffer(p.stdout, dtype=np.float64).reshape(T, 2 * (d + 1) + 2 * d + 4 + n)
    o = 2 * (d + 1)
    return dict(bm=a[:, :d + 1], b2=a[:, d + 1:o], mean=a[:, o:o + d], var=a[:, o + d:o + 2 * d],
                count=a[:, o + 2 * d], rmean=a[:, o + 2 * d + 1], rvar=a[:, o + 2 * d + 2], rcount=a[:, o + 2 * d + 3],
                returns=a[:, o + 2 * d + 4:]), consts


def check(exe, n, d, special=None):
    obs, rew, done = script(n, d, special)
    got, consts = replay(exe, n, d, obs, rew, done)
    g, b = R.header_constants()
    assert consts[:2] == [g, b] and consts[2] == -(-n // consts[3]) and consts[3] % b == 0
    ref = R.NpVecNormalize(n, d, gamma=GAMMA, epsilon=EPS)
    xmax = float(np.abs(obs).max())
    rmax = 0.0
    for t in range(T):
        after = ref.step(obs[t], rew[t], done[t])
        rmax = max(rmax, float(np.abs(after).max()))
        u = t + 1                                         # updates so far
        key = f"n {n} d {d} step {t}"
        # the batch itself (one update's bound), then the running statistics
        assert np.abs(got["bm"][t, :d] - obs[t].astype(np.float64).mean(0)).max() <= R.mean_bound(n, 1, xmax), key
        assert np.abs(got["b2"][t, :d] / n - obs[t].astype(np.float64).var(0)).max() <= R.var_bound(n, 1, xmax), key
        assert (got["b2"][t] >= 0).all(), key
        assert np.abs(got["mean"][t] - ref.obs_rms.mean).max() <= R.mean_bound(n, u, xmax), key
        assert np.abs(got["var"][t] - ref.obs_rms.var).max() <= R.var_bound(n, u, xmax), key
        assert got["count"][t] == ref.obs_rms.count and got["rcount"][t] == ref.ret_rms.count, key   # exact
        assert abs(got["rmean"][t] - ref.ret_rms.mean) <= R.mean_bound(n, u, rmax), key
        assert abs(got["rvar"][t] - ref.ret_rms.var) <= R.var_bound(n, u, rmax), key
        assert np.abs(got["returns"][t] - ref.returns).max() <= 4 * T * R.U * rmax, key
        assert not got["returns"][t][done[t]].any(), key
        for c, kind in (special_columns(d) if special is None else special).items():
            if kind in ("const", "ones"):                 # a constant column: M2 == 0 and the mean exact
                assert got["b2"][t, c] == 0.0 and got["bm"][t, c] == float(obs[t, 0, c]), (key, c, kind)
    return consts


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_replayed_statistics_match_running_mean_std(programs, n, d):
    consts = check(programs["plain"], n, d)
    if n == THREE:
        assert consts[2] == 3 and n % consts[3] not in (0, consts[0])    # three partials, a ragged last one


@pytest.mark.parametrize("kind", ["const", "ones", "tight"])
def test_single_special_column(programs, kind):
    """D = 1 has no room for a special column next to an ordinary one: each kind on its own."""
    check(programs["plain"], 65, 1, {0: kind})


def test_replay_under_sanitizers(programs):
    """The same program built with -fsanitize=address,undefined, run directly (a stand-alone binary)."""
    check(programs["san"], THREE, 143)
    check(programs["san"], 17, 3)


def test_chunks_grow_so_that_partials_stay_bounded(programs):
    """norm_chunk_rows / norm_num_partials through the program's stderr would need 2^23 rows of input;
    the rule is restated instead and checked against the header's constants at the sizes it documents."""
    src = open(R.HEADER).read()
    assert "kNormMaxPartials = 1024" in src
    g, b = R.header_constants()
    for n, rows in ((1, b), (65536, 64), (65537, 128), (1 << 23, 8192)):
        per = b * 1024
        assert b * max(1, -(-n // per)) == rows and -(-n // rows) <= 1024


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_scratch_bytes(lib):
    g, b = R.header_constants()
    assert lib.usv_norm_scratch_bytes(0, 143) == 0 and lib.usv_norm_scratch_bytes(64, 0) == 0
    assert lib.usv_norm_scratch_bytes(THREE, 143) == 2 * 3 * 144 * 8
    assert lib.usv_norm_scratch_bytes(65536, 143) == 2 * 1024 * 144 * 8
    assert lib.usv_norm_scratch_bytes(1 << 23, 143) == 2 * 1024 * 144 * 8


def test_norm_calls_refuse_bad_arguments_without_gpu(lib):
    """Everything usv_wrap_step_norm / usv_wrap_reset_norm can refuse before a HIP call is refused with
    USV_ERR_ARG and a message (so also on a machine without a GPU)."""
    from gym_usv_amd import _lib
    buf = (ctypes.c_uint8 * 128)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 8
    w = _lib.UsvWrap(n=4, obs_dim=6, n_stack=2, reward_bytes=4, ring=p, ep_ret=p, ep_len=p)

    def norm(**kw):
        f = dict(n=4, obs_dim=6, flags=7, reserved=0, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8,
                 obs_mean=p, obs_var=p, obs_inv_std=p, obs_count=p, ret_mean=p, ret_var=p, ret_inv_std=p, ret_count=p,
                 returns=p, scratch=p)
        f.update(kw)
        return _lib.UsvNorm(**f)

    def both(z, word):
        zp = ctypes.byref(z) if z is not None else None
        assert lib.usv_wrap_step_norm(ctypes.byref(w), zp, 1, p, p, p, None, None, p, None) == -1, word
        assert word in lib.usv_last_error(), (word, lib.usv_last_error())
        assert lib.usv_wrap_reset_norm(ctypes.byref(w), zp, 0, None, p, None) == -1, word
        assert word in lib.usv_last_error(), (word, lib.usv_last_error())

    both(None, b"null usv_norm")
    for kw, word in ((dict(n=0), b"n and obs_dim"), (dict(obs_dim=-1), b"n and obs_dim"), (dict(n=5), b"equal"),
                     (dict(obs_dim=7), b"equal"), (dict(obs_dim=5000), b"4096"), (dict(flags=8), b"flags"),
                     (dict(reserved=1), b"flags"), (dict(clip_obs=-1.0), b"clip"), (dict(clip_reward=-0.5), b"clip"),
                     (dict(clip_obs=float("nan")), b"clip"), (dict(gamma=1.5), b"gamma"), (dict(gamma=-0.1), b"gamma"),
                     (dict(epsilon=0.0), b"epsilon"), (dict(epsilon=-1e-8), b"epsilon"), (dict(obs_var=None), b"null"),
                     (dict(returns=None), b"null"), (dict(scratch=None), b"null"), (dict(ret_var=p + 4), b"aligned"),
                     (dict(obs_mean=p + 1), b"aligned")):
        both(norm(**kw), word)
    # a good usv_norm next to a bad usv_wrap: the usv_wrap checks still answer
    bad = _lib.UsvWrap(n=4, obs_dim=6, n_stack=0, reward_bytes=4, ring=p, ep_ret=p, ep_len=p)
    assert lib.usv_wrap_step_norm(ctypes.byref(bad), ctypes.byref(norm()), 1, p, p, p, None, None, p, None) == -1
    assert b"n_stack" in lib.usv_last_error()
    assert lib.usv_wrap_step_norm(None, ctypes.byref(norm()), 1, p, p, p, None, None, p, None) == -1
    assert lib.usv_wrap_step_norm(ctypes.byref(w), ctypes.byref(norm()), -1, p, p, p, None, None, p, None) == -1
    assert ctypes.sizeof(_lib.UsvNorm) == 16 + 4 * 8 + 10 * 8


def test_device_wrappers_normalize_settings_are_checked_first():
    """Bad settings raise ValueError / TypeError before the device is looked at; good ones then meet
    the no-CPU-fallback rule."""
    import torch
    import gym_usv_amd
    from gym_usv_amd.wrappers import DeviceWrappers, NormalizeConfig
    cpu = torch.device("cpu")
    for bad in (dict(clip_obs=-1), dict(clip_reward=-1), dict(gamma=1.01), dict(gamma=-0.5), dict(epsilon=0),
                dict(clip=3)):
        with pytest.raises(ValueError):
            DeviceWrappers(4, 6, 2, cpu, normalize=bad)
    with pytest.raises(TypeError):
        DeviceWrappers(4, 6, 2, cpu, normalize=True)
    cfg = NormalizeConfig.of({})
    assert (cfg.training, cfg.norm_obs, cfg.norm_reward, cfg.clip_obs, cfg.clip_reward, cfg.gamma, cfg.epsilon) == \
        (True, True, True, 10.0, 10.0, 0.99, 1e-8)                      # SB3's defaults
    assert NormalizeConfig.of(NormalizeConfig(gamma=0.9)).gamma == 0.9
    with pytest.raises(gym_usv_amd.UsvLibError):
        DeviceWrappers(4, 6, 2, cpu, normalize={})


def test_adapter_normalize_needs_fused():
    import torch
    from gym_usv_amd.sb3 import Sb3VecEnv
    from gym_usv_amd.spaces import Box

    class Venv:
        num_envs, obs_dim, act_dim = 4, 6, 2
        device = torch.device("cpu")
        single_observation_space = Box(-1, 1, shape=(6,))
        single_action_space = Box(-1, 1, shape=(2,))

    with pytest.raises(ValueError, match="fused=True"):
        Sb3VecEnv(venv=Venv(), frame_stack=5, normalize={})
    env = Sb3VecEnv(venv=Venv(), frame_stack=5)          # untouched without it
    with pytest.raises(AttributeError):
        env.obs_rms
