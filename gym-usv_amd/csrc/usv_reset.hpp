// usv_reset.hpp -- in-kernel episode resets (Philox, custom experiment, NumPy-exact) and the autoreset
// kernels that follow a step.
#pragma once

#include "usv_state.hpp"

namespace usv {

// --------------------------------------------------------------------------- reset
// In-kernel episode reset of env e, executed by one whole wave (wave-parallel), and
// distributionally identical to UsvSimpleEnv.reset (simple_env.py:228-308).
//
// Random numbers: lane l runs two Philox4x32-10 blocks keyed by the run seed with counter
// (global env id, episode, l) and (global env id, episode, l + 64): four 53-bit uniforms
// U[l][0..3].  Lane j < 32 draws obstacle j (x, y, radius); lanes 32..36 draw the scalars.
// The reference's draw order cannot be reproduced with Philox anyway (PCG64 + ziggurat), so
// parity of resets is distributional (KS tests); the stream is fixed per (seed, env, episode),
// independent of sharding, precision and kernel.
// last_action is NOT reset (reference quirk) and sensor_data stays stale (the caller keeps the
// scan in the obs row).  Writes the reset-obs header into row[0:15].
// Four uniforms in [0, 1) per lane: one Philox block (24-bit floats) for the f32 build, two
// blocks (53-bit doubles) for the f64 build.
template <typename R> struct Uni4 { R u[4]; };
__device__ __forceinline__ void philox_uniforms(Philox& g, int l, Uni4<float>& o) {
  uint32_t a[4];
  g.c3 = (uint32_t)l;
  g.block(a[0], a[1], a[2], a[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) o.u[i] = (float)(a[i] >> 8) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ void philox_uniforms(Philox& g, int l, Uni4<double>& o) {
  uint32_t a[4], b[4];
  g.c3 = (uint32_t)l;
  g.block(a[0], a[1], a[2], a[3]);
  g.c3 = (uint32_t)l + 64u;
  g.block(b[0], b[1], b[2], b[3]);
  const double k = 1.0 / 9007199254740992.0;
  o.u[0] = (double)((((uint64_t)a[0] << 32) | a[1]) >> 11) * k;
  o.u[1] = (double)((((uint64_t)a[2] << 32) | a[3]) >> 11) * k;
  o.u[2] = (double)((((uint64_t)b[0] << 32) | b[1]) >> 11) * k;
  o.u[3] = (double)((((uint64_t)b[2] << 32) | b[3]) >> 11) * k;
}

// Reset info row _get_info(-1, zeros(3)) (simple_env.py:102-115, :305); reward terms 0.
template <typename R>
__device__ __forceinline__ void reset_info(R* info, R x, R y, R psi, R u, R v, R r, R px0, R py0,
                                           R px1, R py1, R ye, R angle_n) {
  const R vals[USV_INFO_DIM] = {x, y, psi, u, v, r, px0, py0, px1, py1, R(0), R(0),
                                ye, angle_n, R(0), R(0), R(0), R(0), R(0), R(0), R(0), R(0)};
#pragma unroll
  for (int i = 0; i < USV_INFO_DIM; ++i) info[i] = vals[i];
}

// cross-track error of (x, y) w.r.t. the path (simple_env.py:133-137); sin/cos of the path angle
// a_k = atan2(dy, dx) are dy/|d| and dx/|d|
template <typename R>
__device__ __forceinline__ R path_ye(R x, R y, R x0, R y0, R x1, R y1) {
  const R dx = x1 - x0, dy = y1 - y0;
  const R inv_len = R(1) / m_sqrt(dx * dx + dy * dy);
  return -(x - x0) * (dy * inv_len) + (y - y0) * (dx * inv_len);
}
// ye of a boat on its path start: -0 * sin(a_k) + 0 * cos(a_k), a zero that is negative where the path
// points into the second quadrant (sin > 0 > cos).  The f64 build returns the reference's zero (a path
// exactly along -x, dy = +0, is left at +0: the draws do not produce one); the f32 build keeps +0.
template <typename R> __device__ __forceinline__ R start_ye(R dx, R dy) {
  if constexpr (std::is_same<R, float>::value) return R(0);
  else return (dx < R(0) && dy > R(0)) ? R(-0.0) : R(0);
}

// run_custom_experiment (simple_env.py:292-300): after the usual draws of a reset, the drawn
// obstacles, path and pose are replaced by the experiment's; target, velocity and action limits
// stay drawn.  One lane per env: it re-derives the drawn scalars of episode `ep` from their Philox
// lanes (33..35 of reset_wave), then rewrites obstacles, state, the obs header and info.  Run by
// the reset kernel after reset_wave and, for same-step autoresets, by exp_autoreset_kernel after
// the step (kept out of the step kernels, whose pair loop it would make spill).
template <typename R>
__device__ __forceinline__ void reset_experiment(const State<R>& S, int e, int ep, float* row, R* info) {
  const R* X = S.exp;
  R tx, ty, u, v, r, mu, mr, refv;
  {
    Philox g(S.seed, S.gid0 + (uint64_t)e, (uint32_t)ep);
    Uni4<R> U33, U34, U35;
    philox_uniforms(g, 33, U33);
    philox_uniforms(g, 34, U34);
    philox_uniforms(g, 35, U35);
    tx = R(kBound) * U33.u[1]; ty = R(kBound) * U33.u[2];
    u = R(0.15) * U33.u[3]; v = R(0.15) * U34.u[0]; r = R(0.15) * U34.u[1];
    mu = R(1.5) + R(1.5) * U34.u[2];
    mr = R(3) + R(3) * U34.u[3];
    refv = R(0.75) + (mu - R(0.75)) * U35.u[0];
  }
  const int cnt = (int)X[kExpN];
  R* ob = S.orow(e);
  for (int j = 0; j < S.cap; ++j) {
    ob[j] = j < cnt ? X[kExpObs + j] : R(0);
    ob[S.ostride + j] = j < cnt ? X[kExpObs + S.cap + j] : R(0);
    ob[2 * S.ostride + j] = j < cnt ? X[kExpObs + 2 * S.cap + j] : R(0);
  }
  const R ps0 = X[kExpPS], ps1 = X[kExpPS + 1];
  R sx2, cx2;
  m_sincos(X[kExpAngle], &sx2, &cx2);
  const R pe0 = ps0 + cx2 * R(100), pe1 = ps1 + sx2 * R(100);                     // :296
  const R px = X[kExpPose], py = X[kExpPose + 1], psi = X[kExpPose + 2];
  S.F(F_X)[e] = px; S.F(F_Y)[e] = py;
  store_heading<R>(S, e, psi);
  S.F(F_PX0)[e] = ps0; S.F(F_PY0)[e] = ps1;
  S.F(F_PX1)[e] = pe0; S.F(F_PY1)[e] = pe1;
  S.I(I_NOBS)[e] = cnt;
  const R angle = wrap_angle(m_atan2(ty - py, tx - px) - psi);                    // :302, :63-80
  const R dst = m_hypot(px - tx, py - ty);
  const R ye = path_ye(px, py, ps0, ps1, pe0, pe1);
  float h[kHdr];
  make_header<R>(h, u, v, r, angle, dst, ye, refv, R(0), R(0), mu, mr);
  for (int i = 0; i < kHdr; ++i) row[i] = h[i];
  if (info) reset_info<R>(info, px, py, psi, u, v, r, ps0, ps1, pe0, pe1, ye, cdiv(angle, kPi));
}

// `ep` (wave-uniform): env e's episode counter, the Philox counter of this reset's draws
template <typename R, int MODE>
__device__ __forceinline__ void reset_wave_ep(const State<R>& S, int e, int ep, float* row, R* info = nullptr,
                                              int kpath = 0) {
  if (S.np_reset) return;                  // NumPy-exact mode: np_autoreset_kernel resets after the step
  const int l = lane_id();
  Philox g(S.seed, S.gid0 + (uint64_t)e, (uint32_t)ep);
  Uni4<R> U;
  philox_uniforms(g, l, U);
  // scalar draws (uniform across the wave, held in SGPRs):
  //   lane 32: path-start normal pair (Box-Muller) (:234-235), psi (:238), path angle (:241)
  //   lane 33: path length (:242), target x, y (:245), u0 (:246)
  //   lane 34: v0, r0 (:246), max_action[0] (:249), max_action[2] (:250)
  //   lane 35: ref_v (:251), obstacle count (:257), fallback obstacle x, y (:273)
  //   lane 36: fallback obstacle radius (:290)
  const R bm = m_sqrt(R(-2) * log(R(1) - bcast(U.u[0], 32)));
  R sb, cb;
  m_sincos(R(2 * kPi) * bcast(U.u[1], 32), &sb, &cb);
  const R sx = R(kBound / 2) + R(0.5) * bm * cb, sy = R(kBound / 2) + R(0.5) * bm * sb;
  const R tx = R(kBound) * bcast(U.u[1], 33), ty = R(kBound) * bcast(U.u[2], 33);
  const R mu = R(1.5) + R(1.5) * bcast(U.u[2], 34);
  const int n = min(15 + (int)(bcast(U.u[1], 35) * R(15)), 29);
  // obstacles: lane j < n draws (x, y) in [0, 20]^2 (:258) and its radius (:290); drop those
  // within 0.5 of the start or the target (:261-268), order kept; none left -> one fallback
  const R ox = R(kBound) * U.u[0], oy = R(kBound) * U.u[1], orad = R(0.15) + R(0.35) * U.u[2];
  const bool keep = (l < n) && !(m_hypot(sx - ox, sy - oy) < R(0.5) || m_hypot(tx - ox, ty - oy) < R(0.5));
  const unsigned long long ball = ballot(keep);
  int cnt = __popcll(ball);
  const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(ball >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ball, 0));
  R* ob = S.orow(e);
  const int os = S.ostride;
  if (keep) { ob[pos] = ox; ob[os + pos] = oy; ob[2 * os + pos] = orad; }
  if (cnt == 0) {
    const R fx = R(kBound) * bcast(U.u[2], 35), fy = R(kBound) * bcast(U.u[3], 35);
    const R fr = R(0.15) + R(0.35) * bcast(U.u[0], 36);
    if (l == 0) { ob[0] = fx; ob[os] = fy; ob[2 * os] = fr; }
    cnt = 1;
  }
  const R ang = R(-kPi) + R(2 * kPi) * bcast(U.u[3], 32);
  if (kpath > 0) {
    // options['place_obstacles_on_path'] (:276-288): k obstacles at N(path_start + (cos, sin)(angle)
    // * U(0, hypot(0, 20) = 20), 1) per axis, appended unfiltered; lane j draws obstacle j from the
    // Philox block at counter j + 128 (explicit resets only: the step kernels pass kpath = 0)
    R sa, ca;
    m_sincos(ang, &sa, &ca);
    Uni4<R> P;
    philox_uniforms(g, l + 128, P);
    const R mag = R(kBound) * P.u[0];
    const R bq = m_sqrt(R(-2) * log(R(1) - P.u[1]));
    R s2, c2;
    m_sincos(R(2 * kPi) * P.u[2], &s2, &c2);
    const R lx = (ca * mag + sx) + bq * c2, ly = (sa * mag + sy) + bq * s2;
    const R lr = R(0.15) + R(0.35) * P.u[3];
    if (l < kpath) { ob[cnt + l] = lx; ob[os + cnt + l] = ly; ob[2 * os + cnt + l] = lr; }
    cnt += kpath;
  }
  if (l >= cnt && l < S.cap) { ob[l] = R(0); ob[os + l] = R(0); ob[2 * os + l] = R(0); }
  if (MODE == USV_MODE_ASMC_SIMPLE && l < kAsmcN) S.asmc[(size_t)l * S.N + e] = R(0);  // simple_env_asmc.py:15
  if (l == 0) {
    const R psi = R(-kPi) + R(2 * kPi) * bcast(U.u[2], 32);
    const R dist = R(100) + R(10) * bcast(U.u[0], 33);
    const R u = R(0.15) * bcast(U.u[3], 33), v = R(0.15) * bcast(U.u[0], 34), r = R(0.15) * bcast(U.u[1], 34);
    const R mr = R(3) + R(3) * bcast(U.u[3], 34);
    const R refv = R(0.75) + (mu - R(0.75)) * bcast(U.u[0], 35);
    R sa, ca;
    m_sincos(ang, &sa, &ca);
    S.F(F_X)[e] = sx; S.F(F_Y)[e] = sy;
    store_heading<R>(S, e, psi);
    S.F(F_U)[e] = u; S.F(F_V)[e] = v; S.F(F_R)[e] = r;
    S.F(F_PROGRESS)[e] = R(0);
    S.F(F_PX0)[e] = sx; S.F(F_PY0)[e] = sy;
    S.F(F_PX1)[e] = sx + ca * dist; S.F(F_PY1)[e] = sy + sa * dist;                // :243
    S.F(F_MAX_U)[e] = mu; S.F(F_MAX_R)[e] = mr; S.F(F_REF_V)[e] = refv;
    S.I(I_NOBS)[e] = cnt;
    S.I(I_ELAPSED)[e] = 0;
    S.I(I_EPISODE)[e] = ep + 1;
    S.I(I_SCAN)[e] = 0;
    // reset obs: _get_obs(zeros(3)) with the random target_position (:302, :72-80); position
    // == path_start, so ye is a zero (start_ye: its sign)
    const R ye0 = start_ye<R>((sx + ca * dist) - sx, (sy + sa * dist) - sy);
    const R angle = wrap_angle(m_atan2(ty - sy, tx - sx) - psi);
    const R dst = m_hypot(sx - tx, sy - ty);
    float h[kHdr];
    make_header<R>(h, u, v, r, angle, dst, ye0, refv, R(0), R(0), mu, mr);
#pragma unroll
    for (int i = 0; i < kHdr; ++i) row[i] = h[i];
    if (info) reset_info<R>(info, sx, sy, psi, u, v, r, sx, sy, sx + ca * dist, sy + sa * dist, ye0, cdiv(angle, kPi));
  }
}

// The same with the episode counter loaded here.  (The block-queue step passes its own, staged in LDS
// before any store: this load, issued after a pair's stores, would wait for every one of their acks.)
template <typename R, int MODE>
__device__ __forceinline__ void reset_wave(const State<R>& S, int e, float* row, R* info = nullptr,
                                           int kpath = 0) {
  if (S.np_reset) return;
  reset_wave_ep<R, MODE>(S, e, uniform(S.I(I_EPISODE)[e]), row, info, kpath);
}

// sin/cos of the heading used by the lidar; the step kernel and the reset kernel (stale scan)
// must use this same function so their scans are bit-identical
template <typename R> __device__ __forceinline__ void heading_sincos(R psi, R* s, R* c) { fx_sincos(psi, s, c); }


// --------------------------------------------------------------------------- NumPy-exact reset
// numpy.random.Generator(PCG64) as the reference's reset uses it (simple_env.py:234-290), one lane
// per env, draws in the reference order: PCG64 (128-bit LCG, XSL-RR output, stepped before each
// output), next_uint32 buffering the high half, next_double = (next64 >> 11) * 2^-53, the
// ziggurat standard normal over NumPy's tables, uniform = lo + (hi - lo) * next_double and
// Lemire's 32-bit bounded integers.  oracle/np_rng.py restates it and is checked against numpy.
#include "np_ziggurat.inc"
struct NpPcg64 {
  uint64_t sh, sl, ih, il;
  uint32_t has32, u32;
  __device__ uint64_t next64() {
    constexpr uint64_t kMh = 2549297995355413924ULL, kMl = 4865540595714422341ULL;
    const uint64_t lo = sl * kMl;
    const uint64_t hi = __umul64hi(sl, kMl) + sl * kMh + sh * kMl;
    const uint64_t nlo = lo + il;
    sh = hi + ih + (nlo < lo ? 1ULL : 0ULL);
    sl = nlo;
    const uint64_t x = sh ^ sl;
    const unsigned rot = (unsigned)(sh >> 58);
    return (x >> rot) | (x << ((64u - rot) & 63u));
  }
  __device__ uint32_t next32() {
    if (has32) { has32 = 0; return u32; }
    const uint64_t v = next64();
    has32 = 1;
    u32 = (uint32_t)(v >> 32);
    return (uint32_t)v;
  }
  __device__ double next_double() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }
  __device__ double standard_normal() {
    constexpr double kR = 3.6541528853610088, kInvR = 0.27366123732975828;
    for (;;) {
      uint64_t r = next64();
      const int idx = (int)(r & 0xff);
      r >>= 8;
      const bool neg = r & 1;
      const uint64_t rabs = (r >> 1) & 0x000fffffffffffffULL;
      double x = (double)rabs * kNpZigWi[idx];
      if (neg) x = -x;
      if (rabs < kNpZigKi[idx]) return x;
      if (idx == 0) {
        for (;;) {
          const double xx = -kInvR * log1p(-next_double());
          const double yy = -log1p(-next_double());
          if (yy + yy > xx * xx) return ((rabs >> 8) & 1) ? -(kR + xx) : kR + xx;
        }
      }
      if ((kNpZigFi[idx - 1] - kNpZigFi[idx]) * next_double() + kNpZigFi[idx] < exp(-0.5 * x * x)) return x;
    }
  }
  __device__ double uniform(double lo, double hi) { return lo + (hi - lo) * next_double(); }
  __device__ int integers(int lo, int hi) {                  // [lo, hi), hi - lo <= 2^32
    const uint32_t rng = (uint32_t)(hi - 1 - lo), excl = rng + 1;
    uint64_t m = (uint64_t)next32() * excl;
    uint32_t left = (uint32_t)m;
    if (left < excl) {
      const uint32_t thr = (0xFFFFFFFFu - rng) % excl;
      while (left < thr) { m = (uint64_t)next32() * excl; left = (uint32_t)m; }
    }
    return lo + (int)(m >> 32);
  }
};

template <typename R>
__device__ __forceinline__ NpPcg64 np_load(const State<R>& S, int e) {
  auto w = [&](int i) { return (uint64_t)S.nprng[(size_t)i * S.fstride + e]; };
  return NpPcg64{w(0) | (w(1) << 32), w(2) | (w(3) << 32), w(4) | (w(5) << 32), w(6) | (w(7) << 32),
                 (uint32_t)w(8), (uint32_t)w(9)};
}
template <typename R>
__device__ __forceinline__ void np_store(const State<R>& S, int e, const NpPcg64& g) {
  const uint32_t v[10] = {(uint32_t)g.sh, (uint32_t)(g.sh >> 32), (uint32_t)g.sl, (uint32_t)(g.sl >> 32),
                          (uint32_t)g.ih, (uint32_t)(g.ih >> 32), (uint32_t)g.il, (uint32_t)(g.il >> 32),
                          g.has32, g.u32};
  for (int i = 0; i < 10; ++i) S.nprng[(size_t)i * S.fstride + e] = v[i];
}

// UsvSimpleEnv.reset (simple_env.py:228-308) with the env's own Generator; usv-asmc-simple also
// zeroes the ASMC state (simple_env_asmc.py:14-16).  Writes the reset obs header into `row`
// (its sensor half, the stale scan, is the caller's).  Draws in double, stored as R.
template <typename R, int MODE>
__device__ void np_reset(const State<R>& S, int e, float* row, R* info = nullptr, int kpath = 0) {
  NpPcg64 g = np_load(S, e);
  const double sx = 0.5 * g.standard_normal() + kBound / 2;                      // :234-235
  const double sy = 0.5 * g.standard_normal() + kBound / 2;
  (void)g.standard_normal(); (void)g.standard_normal(); (void)g.next_double();   // :236-237, discarded
  const double psi = g.uniform(-kPi, kPi);                                       // :238
  const double ang = g.uniform(-kPi, kPi), dist = g.uniform(100, 110);           // :241-242
  const double tx = g.uniform(0, kBound), ty = g.uniform(0, kBound);             // :245
  const double u = g.uniform(0.0, 0.15), v = g.uniform(0.0, 0.15), r = g.uniform(0.0, 0.15);  // :246
  const double mu = g.uniform(1.50, 3);                                          // :249
  (void)g.next_double(); (void)g.next_double();                                  // max_action[1], [2]
  const double mr = g.uniform(3, 6);                                             // :250
  const double refv = g.uniform(0.75, mu);                                       // :251
  const int n = g.integers(15, 30);                                              // :257
  R* ob = S.orow(e);
  const int os = S.ostride;
  int cnt = 0;
  for (int j = 0; j < n; ++j) {                                                  // :258-268
    const double ox = g.uniform(0, kBound), oy = g.uniform(0, kBound);
    if (!(hypot(sx - ox, sy - oy) < 0.5 || hypot(tx - ox, ty - oy) < 0.5)) {
      ob[cnt] = R(ox); ob[os + cnt] = R(oy); ++cnt;
    }
  }
  if (cnt == 0) {                                                                // :270-274
    const double ox = g.uniform(0, kBound), oy = g.uniform(0, kBound);
    ob[0] = R(ox); ob[os] = R(oy); cnt = 1;
  }
  if (kpath > 0) {                                                               // :276-288
    // mag = uniform(0, hypot(*env_bounds) = hypot(0, 20), k); line_x = normal(cos(angle) * mag +
    // path_start[0], 1); line_y likewise: k uniforms, then k normals per axis
    // (the k magnitudes are re-drawn from copies of the generator instead of being buffered)
    const double ca = cos(ang), sa = sin(ang);
    NpPcg64 gx = g, gy = g;
    for (int j = 0; j < kpath; ++j) (void)g.next_double();
    for (int j = 0; j < kpath; ++j) ob[cnt + j] = R((ca * gx.uniform(0, kBound) + sx) + g.standard_normal());
    for (int j = 0; j < kpath; ++j) ob[os + cnt + j] = R((sa * gy.uniform(0, kBound) + sy) + g.standard_normal());
    cnt += kpath;
  }
  for (int j = 0; j < cnt; ++j) ob[2 * os + j] = R(g.uniform(0.15, 0.5));      // :290
  np_store(S, e, g);
  double ps0 = sx, ps1 = sy, pe0 = sx + cos(ang) * dist, pe1 = sy + sin(ang) * dist;   // :243
  double px = sx, py = sy, pp = psi;
  if (const R* X = S.exp) {                                                      // :292-300
    cnt = (int)X[kExpN];
    for (int j = 0; j < cnt; ++j) {
      ob[j] = X[kExpObs + j]; ob[os + j] = X[kExpObs + S.cap + j]; ob[2 * os + j] = X[kExpObs + 2 * S.cap + j];
    }
    ps0 = (double)X[kExpPS]; ps1 = (double)X[kExpPS + 1];
    pe0 = ps0 + cos((double)X[kExpAngle]) * 100; pe1 = ps1 + sin((double)X[kExpAngle]) * 100;
    px = (double)X[kExpPose]; py = (double)X[kExpPose + 1]; pp = (double)X[kExpPose + 2];
  }
  for (int j = cnt; j < S.cap; ++j) { ob[j] = R(0); ob[os + j] = R(0); ob[2 * os + j] = R(0); }
  if (MODE == USV_MODE_ASMC_SIMPLE)
    for (int i = 0; i < kAsmcN; ++i) S.asmc[(size_t)i * S.N + e] = R(0);
  const R x0 = R(px), y0 = R(py), ps = R(pp);
  S.F(F_X)[e] = x0; S.F(F_Y)[e] = y0;
  store_heading<R>(S, e, ps);
  S.F(F_U)[e] = R(u); S.F(F_V)[e] = R(v); S.F(F_R)[e] = R(r);
  S.F(F_PROGRESS)[e] = R(0);
  S.F(F_PX0)[e] = R(ps0); S.F(F_PY0)[e] = R(ps1);
  S.F(F_PX1)[e] = R(pe0); S.F(F_PY1)[e] = R(pe1);
  S.F(F_MAX_U)[e] = R(mu); S.F(F_MAX_R)[e] = R(mr); S.F(F_REF_V)[e] = R(refv);
  S.I(I_NOBS)[e] = cnt;
  S.I(I_ELAPSED)[e] = 0;
  S.I(I_EPISODE)[e] = S.I(I_EPISODE)[e] + 1;
  S.I(I_SCAN)[e] = 0;
  const R angle = wrap_angle(m_atan2(R(ty) - y0, R(tx) - x0) - ps);             // :302, :63-80
  const R dst = m_hypot(x0 - R(tx), y0 - R(ty));
  const R ye = S.exp ? path_ye(x0, y0, R(ps0), R(ps1), R(pe0), R(pe1)) : start_ye<R>(R(pe0) - R(ps0), R(pe1) - R(ps1));
  float h[kHdr];
  make_header<R>(h, R(u), R(v), R(r), angle, dst, ye, R(refv), R(0), R(0), R(mu), R(mr));
  for (int i = 0; i < kHdr; ++i) row[i] = h[i];
  if (info) reset_info<R>(info, x0, y0, ps, R(u), R(v), R(r), R(ps0), R(ps1), R(pe0), R(pe1), ye, cdiv(angle, kPi));
}

// Same-step autoreset in NumPy-exact mode, after the step kernel: envs that ended this step get
// a reset header; their obs row keeps the step's scan as the stale sensors (simple_env.py:302).
template <typename R, int MODE>
__global__ __launch_bounds__(kBlock) void np_autoreset_kernel(State<R> S, IO<R> io) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= S.N || !(io.term[e] | io.trunc[e])) return;
  np_reset<R, MODE>(S, e, io.obs + (size_t)e * kObsDim);
}

// Same-step autoreset with a custom experiment installed (Philox resets): after the step kernel,
// envs that ended this step get the experiment's obstacles, path and pose (simple_env.py:292-300).
template <typename R>
__global__ __launch_bounds__(kBlock) void exp_autoreset_kernel(State<R> S, IO<R> io) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= S.N || !(io.term[e] | io.trunc[e])) return;
  reset_experiment<R>(S, e, S.I(I_EPISODE)[e] - 1, io.obs + (size_t)e * kObsDim, nullptr);
}

}  // namespace usv
