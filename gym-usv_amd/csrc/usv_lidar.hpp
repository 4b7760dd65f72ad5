// usv_lidar.hpp -- the 128-ray lidar, wave-per-env: brute force, the f32 / f64 angular windows, lidar_wave,
// and the LDS head (ray table, slots) the step kernels share.
#pragma once

#include "usv_state.hpp"

namespace usv {

// --------------------------------------------------------------------------- lidar
// 128-ray lidar of one env at pose (px, py, heading sin/cos), wave-per-env.  Lane l owns rays
// l and l+64; lane j holds obstacle j (`o`).  Restates compute_sensor_measurments /
// compute_obstacle_positions / _compute_sensor_distances (usv_asmc_ca_env.py:411-461,
// 500-519): per ray, the hit obstacle with the smallest key d_j = |c_j - p| - r_j, which is
// the reference's first hit in argsort(d) order.  Every product is an explicit fma or a
// rounded multiply and every variant evaluates the identical per-(ray, obstacle) arithmetic,
// so all variants -- and the step and reset kernels -- produce bit-identical scans.
template <typename R> struct Ray { R c, s, bk; int bj; };

template <typename R> __device__ __forceinline__ R l_sqrt(R x) { return m_sqrt(x); }
template <> __device__ __forceinline__ float l_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
template <typename R> __device__ __forceinline__ R l_norm(R x) { return x / R(kSensorMax); }
template <> __device__ __forceinline__ float l_norm(float x) { return x * 0.01f; }

// Ray frame.  Obstacles are rotated once into the frame of ray 0 (heading - 120 deg): a along
// ray 0, b to its left; ray i is then (cos i*res, sin i*res) from the table, and for every
// (ray, obstacle) pair proj = a cos + b sin, perp = a sin - b cos -- the reference's projection
// (usv_asmc_ca_env.py:506-518) with both vectors in that frame, so no per-pair rotation.
template <typename R> __device__ __forceinline__ R ray_c(R cp, R sp, R co, R so) { return m_fma(cp, co, -(sp * so)); }
template <typename R> __device__ __forceinline__ R ray_s(R cp, R sp, R co, R so) { return m_fma(sp, co, cp * so); }
template <typename R> __device__ __forceinline__ void to_ray0(R dx, R dy, R c0, R s0, R& a, R& b) {
  a = m_fma(dx, c0, dy * s0);
  b = m_fma(dy, c0, -(dx * s0));
}

template <typename R, bool RANGE_CHECK>
__device__ __forceinline__ void ray_pair(Ray<R>& ra, R jdx, R jdy, R jr2, R jk, int j) {
  const R proj = m_fma(jdx, ra.c, jdy * ra.s);    // obstacle x in the ray frame (:506-517)
  const R perp = m_fma(jdx, ra.s, -(jdy * ra.c)); // obstacle y, mirrored (:518)
  const R delta = m_fma(-perp, perp, jr2);        // r^2 - y^2 (:453)
  bool hit = (proj >= R(0)) & (delta >= R(0)) & (jk < ra.bk);
  if (RANGE_CHECK) hit = hit && (proj - l_sqrt(delta)) < R(kSensorMax);   // :458
  ra.bk = hit ? jk : ra.bk;
  ra.bj = hit ? j : ra.bj;
}

// (the lidar variant bits LID, kLidSkip / kLidUnroll2 / kLidWindow: usv_variant.hpp)

template <typename R, bool RANGE_CHECK, bool UNROLL2>
__device__ __forceinline__ void ray_loop(Ray<R>& r0, Ray<R>& r1, R dx, R dy, R r2, R key, int n) {
  if (UNROLL2) {
    for (int j = 0; j < n; j += 2) {             // n even (padded with a never-hit obstacle)
      const R adx = bcast(dx, j), ady = bcast(dy, j), ar2 = bcast(r2, j), ak = bcast(key, j);
      const R bdx = bcast(dx, j + 1), bdy = bcast(dy, j + 1), br2 = bcast(r2, j + 1), bk = bcast(key, j + 1);
      ray_pair<R, RANGE_CHECK>(r0, adx, ady, ar2, ak, j);
      ray_pair<R, RANGE_CHECK>(r1, adx, ady, ar2, ak, j);
      ray_pair<R, RANGE_CHECK>(r0, bdx, bdy, br2, bk, j + 1);
      ray_pair<R, RANGE_CHECK>(r1, bdx, bdy, br2, bk, j + 1);
    }
  } else {
    for (int j = 0; j < n; ++j) {                // n wave-uniform: scalar loop, v_readlane bcast
      const R jdx = bcast(dx, j), jdy = bcast(dy, j), jr2 = bcast(r2, j), jk = bcast(key, j);
      ray_pair<R, RANGE_CHECK>(r0, jdx, jdy, jr2, jk, j);
      ray_pair<R, RANGE_CHECK>(r1, jdx, jdy, jr2, jk, j);
    }
  }
}

template <typename R>
__device__ __forceinline__ R reading_of(R c, R s, int bj, R dx, R dy, R r2) {
  const int src = bj < 0 ? 0 : bj;
  const R gdx = __shfl(dx, src, kWave), gdy = __shfl(dy, src, kWave), gr2 = __shfl(r2, src, kWave);
  const R proj = m_fma(gdx, c, gdy * s);
  const R perp = m_fma(gdx, s, -(gdy * c));
  const R delta = m_fma(-perp, perp, gr2);
  return bj >= 0 ? proj - l_sqrt(delta) : R(kSensorMax);                        // :457-459
}

// Rays span [psi - 120deg, psi + 118.125deg]; the blind sector between them has half-width
// 60.9375deg around psi + 179.0625deg.  An obstacle (distance d > r) can be hit by no ray if
// its angular extent [phi - a, phi + a], a = asin(r/d), lies inside that sector with a
// 2-ray (3.75deg) margin:  dot(c - p, w) > cos(h)*sqrt(d^2 - r^2) + sin(h)*r  and r < d*sin(h)
// with h = 57.1875deg.  Skipping such obstacles never changes a reading.
constexpr double kBlindC = -0.99985057700379, kBlindS = 0.01636173162648;  // cos/sin(179.0625deg)
constexpr double kBlindCosH = 0.54212310917132, kBlindSinH = 0.84029769328406;  // h = 57.1875deg
constexpr double kRes = (4.0 * kPi / 3.0) / kSensors;
constexpr double kStartC = -0.5, kStartS = -0.86602540378443865;                 // cos/sin(-120deg)

// Per-env lidar outputs: readings of this lane's two rays and the three wave-uniform flags the
// step needs (simple_env.py:153-155, :334; the "< max range" test of :458 only matters if an
// obstacle is ~100 m away).
template <typename R> struct Scan { R rd0, rd1; bool term, far; };

// |atan2(y, x)| error < 7e-4 rad = 0.02 ray (degree-5 minimax on [0,1] + octant folding), well inside
// the quarter-ray window margin; only used to size the conservative ray windows, never for a reading.
// atan2 to |err| <= 6.1e-4 rad (degree-5 odd minimax on [0, 1] plus octant folding)
__device__ __forceinline__ float fast_atan2(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(fmaxf(ax, ay), 1e-30f), mn = fminf(ax, ay);
  const float t = mn * __builtin_amdgcn_rcpf(mx);
  const float s = t * t;
  float p = fmaf(fmaf(0.0793406442f, s, -0.288691819f), s, 0.995358229f) * t;
  p = ay > ax ? 1.57079633f - p : p;
  p = x < 0.0f ? 3.14159265f - p : p;
  return y < 0.0f ? -p : p;
}

constexpr double kWinMargin = 0.05;   // ray-window margin of the window lidar, in rays (lidar_window)
// armed (no-hit) slot of lidar_window2: key bits all ones (above every ord_key of a finite or
// infinite key, so any hit wins the ds_min_u64) and reading bits of the max range 100.0f
constexpr unsigned long long kSlotArm = 0xFFFFFFFF42C80000ull;
static_assert(kSensorMax == 100.0, "kSlotArm's reading half is 100.0f");

__device__ __forceinline__ unsigned ord_key(float k) {   // float -> order-preserving uint
  const unsigned u = __float_as_uint(k);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Exclusive prefix from an inclusive one: the value of lane l - 1 (DPP wave_shr:1; lane 0 gets 0).
__device__ __forceinline__ int wave_excl_of(int incl) {
  return __builtin_amdgcn_update_dpp(0, incl, 0x138, 0xF, 0xF, true);
}
// Inclusive prefix sum over the 64 lanes (DPP row scans + row carries).
__device__ __forceinline__ int wave_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
  return v;
}

template <typename R, int LID>
__device__ __forceinline__ void lidar_brute(R dx, R dy, R r2, R key, R d, R rr, bool valid, int n,
                                            bool far, R sp, R cp, R co0, R so0, R co1, R so1,
                                            Scan<R>& out) {
  const int l = lane_id();
  int m = n;
  R a, b;
  to_ray0(dx, dy, ray_c(cp, sp, R(kStartC), R(kStartS)), ray_s(cp, sp, R(kStartC), R(kStartS)), a, b);
  if (LID & kLidSkip) {
    const R wx = cp * R(kBlindC) - sp * R(kBlindS), wy = sp * R(kBlindC) + cp * R(kBlindS);
    const R dot = dx * wx + dy * wy;
    const R lim = R(kBlindCosH) * l_sqrt(m_abs(d * d - rr * rr)) + R(kBlindSinH) * rr;
    const bool blind = (d > rr) & (rr < d * R(kBlindSinH)) & (dot > lim);
    const bool keep = valid & !blind;
    // stream-compact the kept obstacles (order preserved, so min-key ties still resolve to
    // the lowest original index)
    const unsigned long long ball = ballot(keep);
    m = __popcll(ball);
    const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(ball >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ball, 0));
    const int dst = keep ? pos : 63;               // dropped lanes all land in lane 63 (unused)
    a = __builtin_bit_cast(R, permute(dst, __builtin_bit_cast(typename Bits<R>::T, a)));
    b = __builtin_bit_cast(R, permute(dst, __builtin_bit_cast(typename Bits<R>::T, b)));
    r2 = __builtin_bit_cast(R, permute(dst, __builtin_bit_cast(typename Bits<R>::T, r2)));
    key = __builtin_bit_cast(R, permute(dst, __builtin_bit_cast(typename Bits<R>::T, key)));
  }
  if (LID & kLidUnroll2) {
    if (l >= m) { r2 = R(-1); key = big<R>(); }    // padding obstacle: delta < 0, never hit
    m = (m + 1) & ~1;
  }
  Ray<R> r0{co0, so0, big<R>(), -1};
  Ray<R> r1{co1, so1, big<R>(), -1};
  if (!far) ray_loop<R, false, (LID & kLidUnroll2) != 0>(r0, r1, a, b, r2, key, m);
  else ray_loop<R, true, (LID & kLidUnroll2) != 0>(r0, r1, a, b, r2, key, m);
  out.rd0 = reading_of(r0.c, r0.s, r0.bj, a, b, r2);
  out.rd1 = reading_of(r1.c, r1.s, r1.bj, a, b, r2);
}

// Angular-window lidar (f32).  Lane j computes the ray-index windows its obstacle can touch
// (conservative: a quarter ray of margin around an upper bound of asin(r/d), pi/2 when the boat is
// inside it), the (obstacle, ray) pairs are expanded over the lanes (prefix sum; each pair's
// owner found with LDS start markers and a max-scan), each pair runs the same exact test as
// the brute loop, and the hit with the smallest key per ray wins through an LDS ds_min_u64 on
// (order-preserving key bits << 32 | hit distance bits) -- the min-key rule, and the winner's
// reading rides along as the payload.  Bit-identical to lidar_brute except on an exact key tie
// between two different obstacles (measure zero; brute then takes the lower index, this the
// nearer hit, and the reference's own argsort tie order is unspecified).  ~50 pair tests per
// env instead of 128 x n.
struct WinLds {
  unsigned long long* slot;   // [128] per wave, ~0 between envs
  int* mark;                  // [64]  per wave (cross-lane through LDS: ordered by a wave fence)
  const float2* rayoff;       // [128] block-shared ray offset table
};

// One env's obstacle row in LDS: the x, y, r planes (the global row copied verbatim by LDS-DMA,
// or staged through registers by the reset kernel).
template <typename R> struct RowSoA {
  const R* x; const R* y; const R* r;
  __device__ __forceinline__ void get(int j, R& X, R& Y, R& Rr) const { X = x[j]; Y = y[j]; Rr = r[j]; }
};

// Inclusive max-scan over the 64 lanes of non-negative values (DPP row scans + row_bcast
// carries; identity 0, so bound_ctrl zero-fill folds each step into one v_max_i32_dpp).
__device__ __forceinline__ int wave_incl_max(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true));   // row_shr:1
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true));   // row_shr:2
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true));   // row_shr:4
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true));   // row_shr:8
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false));  // row_bcast:15
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false));  // row_bcast:31
  return v;
}

// The same scan as fused DPP maxes in one asm block: a lane whose row is masked off by row_bcast keeps
// its value (vdst = src1), so no zero-filled temporaries are needed.  s_nop 1 before each DPP read
// of the VGPR the previous VALU wrote (gfx9 DPP hazard).
// floor(x) converted to int in one instruction (|x| well inside the int range here)
__device__ __forceinline__ int cvt_flr_i32(float x) {
  int r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

__device__ __forceinline__ int wave_incl_max_asm(int v) {
  asm volatile("s_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"
               : "+v"(v));
  return v;
}

// Two independent max-scans interleaved in one asm block: each DPP read of a VGPR the previous
// VALU wrote needs two wait states, here the other chain's instruction plus one s_nop 0.
__device__ __forceinline__ void wave_incl_max2_asm(int& a, int& b) {
  asm volatile("s_nop 1\n\t"
               "v_max_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
               "v_max_i32_dpp %1, %1, %1 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0\n\t"
               "v_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
               "v_max_i32_dpp %1, %1, %1 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0\n\t"
               "v_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
               "v_max_i32_dpp %1, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0\n\t"
               "v_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
               "v_max_i32_dpp %1, %1, %1 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 0\n\t"
               "v_max_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
               "v_max_i32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 0\n\t"
               "v_max_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
               "v_max_i32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf"
               : "+v"(a), "+v"(b));
}

template <bool RANGE_CHECK, typename Row>
__device__ __forceinline__ void lidar_window(float dx, float dy, float key, float d, float rr, bool valid,
                                             float px, float py, float sp, float cp, const WinLds& L,
                                             const Row& row, Scan<float>& out) {
  const int l = lane_id();
  const float c0r = ray_c(cp, sp, (float)kStartC, (float)kStartS);
  const float s0r = ray_s(cp, sp, (float)kStartC, (float)kStartS);
  float a, b;
  to_ray0(dx, dy, c0r, s0r, a, b);
  const float phi = fast_atan2(b, a);                 // CCW angle from ray 0; ray i at i*res
  // |err| of the window edges: fast_atan2 <= 6.1e-4 rad (0.019 ray), float rounding ~1e-6 rad; a
  // ray 1e-5 rad outside the true extent already fails the exact test by ~r*d*1e-5 >> ulp.  The
  // margin (0.05 ray = 1.6e-3 rad) covers both 2.6x over.
  const float margin = (float)(kWinMargin * kRes);
  const bool inside = d <= rr * 1.001f;
  // asin(x) <= x + (pi/2 - 1) x^3 on [0, 1] (Taylor coefficients >= 0 summing to pi/2 at x = 1)
  const float x = fminf(rr * __builtin_amdgcn_rcpf(d), 1.0f);
  const float half = inside ? (float)(kPi / 2) + margin
                            : fmaf((float)(kPi / 2 - 1) * x, x * x, x) + margin;
  // in ray units; the second window is the first shifted by one turn = 2 pi / res = 192 rays
  // exactly (rounding of the shifted float edges would only move an edge that lies within
  // ~1e-5 ray of an integer, i.e. well inside the quarter-ray margin)
  const float inv = (float)(1.0 / kRes);
  const float pr = phi * inv, hr = half * inv;
  const int a1 = (int)ceilf(pr - hr), b1 = (int)floorf(pr + hr);
  static_assert(kSensors * 3 == 2 * 192, "192 rays per turn");
  const int lo1 = max(0, a1), hi1 = min(127, b1);
  const int lo2 = max(0, a1 + 192), hi2 = min(127, b1 + 192);
  const int len1 = valid ? max(0, hi1 - lo1 + 1) : 0, len2 = valid ? max(0, hi2 - lo2 + 1) : 0;
  const int cnt = len1 + len2;
  const int incl = wave_incl_scan(cnt);
  const int off = incl - cnt;
  const int W = __builtin_amdgcn_readlane(incl, 63);
  const int meta = lo1 | (len1 << 8) | (lo2 << 16);
  const unsigned ok = ord_key(key);
  int carry = 0;                                      // owner marks are lane + 1; 0 = none
  for (int base = 0; base < W; base += kWave) {       // wave-uniform pass count
    // owner of pair q = base + l: the obstacle whose run of pairs starts at or before q
    L.mark[l] = 0;
    if (cnt > 0 && off >= base && off < base + kWave) L.mark[off - base] = l + 1;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // other lanes' marks must be read
    __builtin_amdgcn_wave_barrier();
    const int j1 = max(wave_incl_max(L.mark[l]), carry);
    carry = __builtin_amdgcn_readlane(j1, 63);
    const int j = j1 - 1;
    const int q = base + l;
    const int jj = j < 0 ? 0 : j;
    const int k = q - __shfl(off, jj, kWave);
    const int mj = __shfl(meta, jj, kWave);
    const unsigned gk = (unsigned)__shfl((int)ok, jj, kWave);
    const int l1 = mj & 255, n1 = (mj >> 8) & 255, l2 = mj >> 16;
    const int i = min(max((k < n1 ? l1 : l2 - n1) + k, 0), 127);
    float gx, gy, gr, ga, gb;
    row.get(jj, gx, gy, gr);
    to_ray0(gx - px, gy - py, c0r, s0r, ga, gb);
    const float2 cs = L.rayoff[i];
    const float proj = fmaf(ga, cs.x, gb * cs.y);
    const float perp = fmaf(ga, cs.y, -(gb * cs.x));
    const float delta = fmaf(-perp, perp, gr * gr);
    const float dist = proj - l_sqrt(delta);                 // reading if this pair wins (:457)
    bool hit = (q < W) & (proj >= 0.0f) & (delta >= 0.0f);
    if (RANGE_CHECK) hit = hit && dist < (float)kSensorMax;   // :458
    if (hit)
      atomicMin(&L.slot[i], ((unsigned long long)gk << 32) | __float_as_uint(dist));
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");     // all lanes' ds_min_u64 landed
  __builtin_amdgcn_wave_barrier();
  const unsigned long long v0 = L.slot[l], v1 = L.slot[l + 64];
  L.slot[l] = kSlotArm;                               // re-arm for this wave's next env
  L.slot[l + 64] = kSlotArm;
  out.rd0 = __uint_as_float((unsigned)v0);           // no hit: the armed payload, max range
  out.rd1 = __uint_as_float((unsigned)v1);
}

// Two envs per wave (f32 window path, <= 32 obstacles each): lanes 0..31 hold env A's
// obstacles, lanes 32..63 env B's, both envs' (obstacle, ray) pairs go into ONE expanded list,
// and each pair takes the pose of its owner's env.  The per-obstacle setup, the scans and the
// pass overhead are shared by the two envs; each pair runs the identical exact test, so the
// readings are bit-identical to one-env-per-wave.  Slots [256]: env A rays, then env B rays.
//
// The obstacle lanes leave (a, b, r^2, key bits) records in the rows buffer (lane j at slot j;
// written after every lane's row reads, which the wave's LDS instructions complete in order),
// and each pair reads its owner's record: no pose select, no rotation and no re-read of the row.
// Each lane brings its own env's ray-0 direction (c0r, s0r) = (cos, sin)(psi - 120 deg).
// One ray window per obstacle: phi is taken in [-32.5, 159.5) rays from ray 0, i.e. with the branch
// cut in the middle of the rear blind sector (rays cover [0, 127], the blind sector (127, 192)), so a
// window of half-width < 32.5 rays never wraps onto the rays; wider ones (an obstacle closer than
// r / sin(61 deg), or the boat inside it) take all 128 rays, the exact test sorting them out.
// `far` (wave-uniform): some obstacle is >= 99 m away, where the reference's `< max range` test
// (usv_asmc_ca_env.py:458) can matter; it is applied to every pair then.
// rotA / rotB (wave-uniform, 0..63): lane l receives env A's readings of rays (l - rotA) & 63 and
// 64 + ((l - rotA) & 63) (env B likewise with rotB), i.e. the scan rotated across lanes for free (the
// slot reads take the rotated addresses); the block-queue step stores an env pair's obs rows as
// 32-B-aligned spans this way.
__device__ __forceinline__ void lidar_window2(float dx, float dy, float key, float d, float rr, bool valid, bool far,
                                              float c0r, float s0r, float4* rec, const WinLds& L, int* mark2,
                                              Scan<float>& A, Scan<float>& B, QProf* qp = nullptr,
                                              int rotA = 0, int rotB = 0, int* wout = nullptr) {
  const int l = lane_id();
  float a, b;
  to_ray0(dx, dy, c0r, s0r, a, b);
  const float inv = (float)(1.0 / kRes);
  float pr = fast_atan2(b, a) * inv;                  // CCW angle from ray 0 in rays, (-96, 96]
  pr = pr < -32.5f ? pr + 192.0f : pr;                // -> [-32.5, 159.5)
  const float margin = (float)(kWinMargin * kRes);    // see lidar_window
  const float x = fminf(rr * __builtin_amdgcn_rcpf(d), 1.0f);
  // asin(x) <= x + (pi/2 - 1) x^3 (see lidar_window); boat inside: all rays
  const float hr = (fmaf((float)(kPi / 2 - 1) * x, x * x, x) + margin) * inv;
  // all rays when the window reaches 32 rays: that includes the boat inside the obstacle (x = 1
  // gives hr = 32.05), and a narrower window never wraps onto the rays.  ceil(v) = -floor(-v)
  // (v_cvt_flr_i32_f32: floor and convert in one instruction)
  const bool wide = hr >= 32.0f;
  // both converts unconditionally (the conversion saturates on a wide window's large operands): with a
  // convert inside each select arm the compiler branches on exec around it, twice per env pair
  const int flo = cvt_flr_i32(hr - pr), fhi = cvt_flr_i32(pr + hr);
  const int lo = wide ? 0 : max(0, -flo);
  const int hi = wide ? 127 : min(127, fhi);
  const int cnt = valid ? max(0, hi - lo + 1) : 0;
  const int incl = wave_incl_scan(cnt);
  const int off = wave_excl_of(incl);
  const int W = __builtin_amdgcn_readlane(incl, 63);
  if (wout) *wout = W;                                 // (diagnostic builds: the pair's window size)
  // Segment marks: obstacle lane l's run of pairs starts at off and maps pair q to slot
  // q + (lo - off) + 128 [env B], i.e. ray (slot & 127).  Its mark, written at off, is
  // l << 16 | (lo - off + 128 [env B] + 32768): the owner in the high bits keeps the max-scan in
  // run order and the slot offset rides in the low bits (in [24704, 33023]), so a pair finds its
  // owner, its ray and its slot from one max-scan, with no per-pair gather of the owner's window.
  // A cleared mark is 0, below every mark (the low bits are > 0), and pair 0 always has one (the
  // first obstacle with pairs starts at 0), so every pair's scan result names an owner.
  const int mk0 = (l << 16) | (lo - off + (l >= 32 ? 128 : 0) + 32768);
  rec[l] = make_float4(a, b, rr * rr, __uint_as_float(ord_key(key)));
  // The marks are cleared once per call (below), not per pass: a mark left by an earlier pass of
  // this call is <= that pass's carry, which the max-scan folds in anyway.
  // the pass that holds this obstacle's mark (-1: no pairs) and the mark's index in it
  const int mpass = cnt > 0 ? off >> 6 : -1;
  int* const mslot = L.mark + (off & (kWave - 1));
  int carry = 0;
  QMARK(2);
  // pair q = base + l of a pass whose max-scanned mark is mk: owner, ray, exact test, ds_min.
  // pair_ld reads the owner's record and the ray, pair_do tests and takes the ds_min; the two-pass
  // case issues both passes' reads before either test (one LDS round trip for both).
  struct PairIn { float4 o; float2 cs; int si; };
  auto pair_ld = [&](int base, int mk) {
    const int jj = mk >> 16;                          // owner obstacle lane
    // slot of (owner env, ray) of pair q = base + l: q + (mk & 0xffff) - 32768, of which only the
    // low 8 bits are used (= those of q + mk); exact for q < W, other lanes (no hit) read some
    // ray's offsets
    const int si = base + l + mk;
    return PairIn{rec[jj], L.rayoff[si & 127], si};   // owner's (a, b, r^2, key bits), ray (cos, sin)
  };
  auto pair_do = [&](int base, const PairIn& p) {
    const float4 o = p.o;
    const float2 cs = p.cs;
    // the key half of the payload before the hit branch (the whole record is read by one
    // ds_read_b128: the key is not re-read inside the branch)
    unsigned long long* const sl = &L.slot[p.si & 255];
    const unsigned kb = __float_as_uint(o.w);
    asm volatile("" :: "v"(kb));
    const float proj = fmaf(o.x, cs.x, o.y * cs.y);
    const float perp = fmaf(o.x, cs.y, -(o.y * cs.x));
    const float delta = fmaf(-perp, perp, o.z);
    const float dist = proj - l_sqrt(delta);
    const bool hit = (l < W - base) & (proj >= 0.0f) & (delta >= 0.0f) & (!far | (dist < (float)kSensorMax));  // :458
    if (hit)                                          // slots: env A's rays, then env B's
      atomicMin(sl, ((unsigned long long)kb << 32) | __float_as_uint(dist));
  };
  auto pair = [&](int base, int mk) { pair_do(base, pair_ld(base, mk)); };
  int base = 0, pass = 0;
  if (W > kWave) {
    // passes 0 and 1 at once (1.65 passes per env pair on average at C3): pass 1's marks go to mark2, 64 ints
    // that no DMA touches (the tail of the row buffer the next pair's 768 B of rows land in; it
    // held records last time, so it is cleared first -- LDS ops of a wave complete in order),
    // and the two max-scans run interleaved; pass 1's carry is pass 0's last mark (18.88 -> 18.70 us
    // per step at 65 536 envs, tools/exp_step_ab.sh)
    QCOUNT(9, 2);
    // One masked write for both passes' marks, its destination selected on the LDS address (a write
    // per pass is a three-way exec nest); the marks of passes >= 2 are written by the loop below.
    mark2[l] = 0;
    int* const mdst = (mpass == 1 ? mark2 : L.mark) + (off & (kWave - 1));
    if ((unsigned)mpass <= 1u) *mdst = mk0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // marks and records visible
    __builtin_amdgcn_wave_barrier();
    int m0 = L.mark[l], m1 = mark2[l];
    wave_incl_max2_asm(m0, m1);
    m1 = max(m1, __builtin_amdgcn_readlane(m0, 63));
    carry = __builtin_amdgcn_readlane(m1, 63);
    const PairIn p0 = pair_ld(0, m0), p1 = pair_ld(kWave, m1);
    pair_do(0, p0);
    pair_do(kWave, p1);
    base = 2 * kWave;
    pass = 2;
  }
  for (; base < W; base += kWave, ++pass) {           // wave-uniform pass count
    QCOUNT(9, 1);
    if (mpass == pass) *mslot = mk0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // marks and records visible
    __builtin_amdgcn_wave_barrier();
    const int mk = max(wave_incl_max_asm(L.mark[l]), carry);
    carry = __builtin_amdgcn_readlane(mk, 63);
    pair(base, mk);
  }
  QMARK(3);
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");     // all lanes' ds_min_u64 landed
  __builtin_amdgcn_wave_barrier();
  const int la = (l - rotA) & (kWave - 1), lb = (l - rotB) & (kWave - 1);
  const unsigned long long a0 = L.slot[la], a1s = L.slot[la + 64];
  const unsigned long long b0 = L.slot[128 + lb], b1s = L.slot[192 + lb];
  // re-arm for this wave's next pair (after every lane's reads: a wave's LDS ops complete in order)
  L.slot[l] = kSlotArm; L.slot[l + 64] = kSlotArm;
  L.slot[128 + l] = kSlotArm; L.slot[192 + l] = kSlotArm;
  L.mark[l] = 0;
  A.rd0 = __uint_as_float((unsigned)a0);              // no hit: the armed payload, max range
  A.rd1 = __uint_as_float((unsigned)a1s);
  B.rd0 = __uint_as_float((unsigned)b0);
  B.rd1 = __uint_as_float((unsigned)b1s);
  QMARK(4);
}

// rows: LDS buffer (>= 1 KiB, reused for the per-obstacle records) holding env A's obstacle row
// (planes x, y, r of stride os) at rows[0] and env B's at rows[3 os].  Per lane: its env's pose
// (px, py), ray-0 direction (c0r, s0r) and obstacle count nl (0: no env in this half).
__device__ __forceinline__ void lidar_wave2(float* rows, int os, int nl, float px, float py, float c0r,
                                            float s0r, const float2* rayoff, unsigned long long* slot,
                                            int* mark, int* mark2, Scan<float>& A, Scan<float>& B,
                                            QProf* qp = nullptr, int rotA = 0, int rotB = 0, int* wout = nullptr) {
  const int l = lane_id();
  const int jl = l & 31;
  const bool valid = jl < nl;
  const float* rb = rows + (l >= 32 ? 3 * os : 0);
  // read unconditionally: lanes past their env's obstacles (or of an absent env B) get slot padding
  // or stale LDS, and every use below is masked by `valid`
  const float ox = rb[jl], oy = rb[os + jl], rr = rb[2 * os + jl];
  const float dx = ox - px, dy = oy - py;
  const float d = l_sqrt(m_fma(dx, dx, dy * dy));
  const float key = valid ? d - rr : big<float>();                              // simple_env.py:205-206
  // ballots of plain compares ANDed on the SALU (a ballot of an ANDed condition makes the compiler
  // materialise it per lane first), and their halves tested there too (ballot_halves)
  const unsigned long long vm = ballot(valid);
  const BallotHalves tb = ballot_halves(vm & ballot(key < (float)kTermDist));   // :334
  A.term = tb.lo != 0u; B.term = tb.hi != 0u;
  A.far = B.far = false;
  const BallotHalves fb = ballot_halves(vm & ballot(d >= (float)(0.99 * kSensorMax)));
  const bool far = (fb.lo | fb.hi) != 0u;
  lidar_window2(dx, dy, key, d, rr, valid, far, c0r, s0r, reinterpret_cast<float4*>(rows), WinLds{slot, mark, rayoff},
                mark2, A, B, qp, rotA, rotB, wout);
}

// Angular-window lidar for the f64 build (one env per wave).  The ray windows are sized in float from
// the f64 geometry (the 0.05-ray margin dwarfs the float rounding of the inputs), and every
// (obstacle, ray) pair in a window runs lidar_brute's exact f64 test on the same ray-0-frame operands
// (a, b, r^2 and the ray table), so the hits are brute's.  The winner per ray is the smallest key:
// ds_min_u64 on the order-preserving key bits with the low 6 bits replaced by the obstacle lane, i.e.
// keys equal to within 64 ulps resolve to the lower lane (brute: exact ties only; the reference's own
// tie order is unspecified).  The winner's reading is then recomputed exactly as lidar_brute does
// (reading_of), so readings are bit-identical to the brute loop.
struct WinLdsD {
  unsigned long long* slot;   // [128] per wave, armed with kSlotArm between envs
  int* mark;                  // [64]  per wave
  const double2* rayoff;      // [128] block-shared ray offset table (f64)
};
__device__ __forceinline__ unsigned long long ord_key64(double k) {   // double -> order-preserving u64
  const unsigned long long b = (unsigned long long)__double_as_longlong(k);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
template <bool RANGE_CHECK>
__device__ __forceinline__ void lidar_window_d(double dx, double dy, double key, double d, double rr, bool valid,
                                               double sp, double cp, const WinLdsD& L, Scan<double>& out) {
  const int l = lane_id();
  double a, b;
  to_ray0(dx, dy, ray_c(cp, sp, double(kStartC), double(kStartS)), ray_s(cp, sp, double(kStartC), double(kStartS)), a, b);
  const double r2 = rr * rr;
  const float inv = (float)(1.0 / kRes);
  float pr = fast_atan2((float)b, (float)a) * inv;    // as lidar_window2: branch cut in the blind sector
  pr = pr < -32.5f ? pr + 192.0f : pr;
  const float margin = (float)(kWinMargin * kRes);
  const float x = fminf((float)rr * __builtin_amdgcn_rcpf((float)d), 1.0f);
  const float hr = (fmaf((float)(kPi / 2 - 1) * x, x * x, x) + margin) * inv;
  const bool wide = (d <= rr * 1.001) | (hr >= 32.5f);
  const int lo = wide ? 0 : max(0, (int)ceilf(pr - hr));
  const int hi = wide ? 127 : min(127, (int)floorf(pr + hr));
  const int cnt = valid ? max(0, hi - lo + 1) : 0;
  const int incl = wave_incl_scan(cnt);
  const int off = wave_excl_of(incl);
  const int W = __builtin_amdgcn_readlane(incl, 63);
  const int mk0 = ((l + 1) << 16) | (lo - off + 32768);
  const unsigned long long kq = (ord_key64(key) & ~63ull) | (unsigned long long)l;
  const unsigned kq_lo = (unsigned)kq, kq_hi = (unsigned)(kq >> 32);
  int carry = 0;
  for (int base = 0; base < W; base += kWave) {       // wave-uniform pass count
    L.mark[l] = 0;                                    // (callers' LDS need not be cleared)
    if (cnt > 0 && off >= base && off < base + kWave) L.mark[off - base] = mk0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int mk = max(wave_incl_max_asm(L.mark[l]), carry);
    carry = __builtin_amdgcn_readlane(mk, 63);
    const int q = base + l;
    const int jj = max((mk >> 16) - 1, 0);
    const int si = (q + (mk & 0xffff) - 32768) & 127;
    const double ja = __shfl(a, jj, kWave), jb = __shfl(b, jj, kWave), jr2 = __shfl(r2, jj, kWave);
    const unsigned long long jk = ((unsigned long long)(unsigned)__shfl((int)kq_hi, jj, kWave) << 32) |
                                  (unsigned)__shfl((int)kq_lo, jj, kWave);
    const double2 cs = L.rayoff[si];
    const double proj = m_fma(ja, cs.x, jb * cs.y);    // ray_pair's arithmetic
    const double perp = m_fma(ja, cs.y, -(jb * cs.x));
    const double delta = m_fma(-perp, perp, jr2);
    bool hit = (q < W) & (proj >= 0.0) & (delta >= 0.0);
    if (RANGE_CHECK) hit = hit && (proj - l_sqrt(delta)) < double(kSensorMax);   // :458
    if (hit) atomicMin(&L.slot[si], jk);
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const unsigned long long v0 = L.slot[l], v1 = L.slot[l + 64];
  L.slot[l] = kSlotArm;
  L.slot[l + 64] = kSlotArm;
  L.mark[l] = 0;
  const int bj0 = v0 == kSlotArm ? -1 : (int)(v0 & 63), bj1 = v1 == kSlotArm ? -1 : (int)(v1 & 63);
  const double2 t0 = L.rayoff[l], t1 = L.rayoff[l + 64];
  out.rd0 = reading_of(t0.x, t0.y, bj0, a, b, r2);
  out.rd1 = reading_of(t1.x, t1.y, bj1, a, b, r2);
}

// Two envs per wave for the f64 window lidar (<= 32 obstacles each), lidar_window_d's arithmetic with
// lidar_window2's layout: lanes 0..31 hold env A's obstacles, lanes 32..63 env B's, each lane in the
// ray-0 frame of its own env's pose; both envs' (obstacle, ray) pairs go into one expanded list whose
// slots are env A's rays then env B's [256].  The winner payload's low 6 bits are the obstacle lane
// (0..63, so it names the env too), and each reading is recomputed from the winner's (a, b, r^2) as
// lidar_brute does: readings bit-identical to lidar_window_d and to the brute loop.
__device__ __forceinline__ void lidar_wave2_d(const double* rows, int os, int nl, double px, double py, double sp,
                                              double cp, const double2* rayoff, unsigned long long* slot,
                                              int* mark, double4* rec, Scan<double>& A, Scan<double>& B) {
  const int l = lane_id();
  const int jl = l & 31;
  const bool valid = jl < nl;
  const double* rb = rows + (l >= 32 ? 3 * os : 0);
  // read unconditionally (lanes past their env's obstacles get padding; every use is masked by valid)
  const double ox = rb[jl], oy = rb[os + jl], rr = rb[2 * os + jl];
  const double dx = ox - px, dy = oy - py;
  const double d = l_sqrt(m_fma(dx, dx, dy * dy));
  const double key = valid ? d - rr : big<double>();                          // simple_env.py:205-206
  const unsigned long long vm = ballot(valid);
  const unsigned long long tb = vm & ballot(key < kTermDist);                  // :334
  A.term = (unsigned)tb != 0u; B.term = (unsigned)(tb >> 32) != 0u;
  A.far = B.far = false;
  const bool far = (vm & ballot(d >= 0.99 * kSensorMax)) != 0;               // :458 matters
  double a, b;
  to_ray0(dx, dy, ray_c(cp, sp, double(kStartC), double(kStartS)), ray_s(cp, sp, double(kStartC), double(kStartS)), a, b);
  const double r2 = rr * rr;
  const float inv = (float)(1.0 / kRes);
  float pr = fast_atan2((float)b, (float)a) * inv;    // branch cut in the blind sector (lidar_window2)
  pr = pr < -32.5f ? pr + 192.0f : pr;
  const float margin = (float)(kWinMargin * kRes);
  const float x = fminf((float)rr * __builtin_amdgcn_rcpf((float)d), 1.0f);
  const float hr = (fmaf((float)(kPi / 2 - 1) * x, x * x, x) + margin) * inv;
  const bool wide = (d <= rr * 1.001) | (hr >= 32.5f);
  const int lo = wide ? 0 : max(0, (int)ceilf(pr - hr));
  const int hi = wide ? 127 : min(127, (int)floorf(pr + hr));
  const int cnt = valid ? max(0, hi - lo + 1) : 0;
  const int incl = wave_incl_scan(cnt);
  const int off = wave_excl_of(incl);
  const int W = __builtin_amdgcn_readlane(incl, 63);
  // mark: owner lane + 1 in the high bits, slot offset (env B: + 128) in the low bits
  const int mk0 = ((l + 1) << 16) | (lo - off + (l >= 32 ? 128 : 0) + 32768);
  const unsigned long long kq = (ord_key64(key) & ~63ull) | (unsigned long long)l;
  // per-obstacle record as two 16-B planes (a, b) [64] and (r^2, key | lane) [64]: lane l's halves at a
  // 16-B stride, so the stores and the owners' gathers are bank-conflict free (a 32-B record stride
  // put lanes 4 apart on the same banks; round 5)
  double2* const recA = reinterpret_cast<double2*>(rec);
  double2* const recB = recA + kWave;
  recA[l] = make_double2(a, b);
  recB[l] = make_double2(r2, __longlong_as_double((long long)kq));
  const int mpass = cnt > 0 ? off >> 6 : -1;
  int carry = 0;
  for (int base = 0, pass = 0; base < W; base += kWave, ++pass) {   // wave-uniform pass count
    if (mpass == pass) mark[off & (kWave - 1)] = mk0;   // marks of earlier passes are <= carry
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int mk = max(wave_incl_max_asm(mark[l]), carry);
    carry = __builtin_amdgcn_readlane(mk, 63);
    const int q = base + l;
    const int jj = max((mk >> 16) - 1, 0);
    const int si = (q + (mk & 0xffff) - 32768) & 255;
    const double2 oa = recA[jj], ob = recB[jj];
    const double4 o = make_double4(oa.x, oa.y, ob.x, ob.y);   // owner's (a, b, r^2, key | lane)
    const unsigned long long jk = (unsigned long long)__double_as_longlong(o.w);
    const double2 cs = rayoff[si & 127];
    const double proj = m_fma(o.x, cs.x, o.y * cs.y);  // ray_pair's arithmetic
    const double perp = m_fma(o.x, cs.y, -(o.y * cs.x));
    const double delta = m_fma(-perp, perp, o.z);
    bool hit = (q < W) & (proj >= 0.0) & (delta >= 0.0);
    if (far) hit = hit && (proj - l_sqrt(delta)) < double(kSensorMax);       // :458 (wave-uniform)
    if (hit) atomicMin(&slot[si], jk);
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const unsigned long long v0 = slot[l], v1 = slot[l + 64], v2 = slot[128 + l], v3 = slot[192 + l];
  slot[l] = kSlotArm; slot[l + 64] = kSlotArm; slot[128 + l] = kSlotArm; slot[192 + l] = kSlotArm;
  mark[l] = 0;
  // reading of the winner (reading_of's arithmetic, the winner's record from LDS)
  auto reading = [&](double c, double sn, unsigned long long v) {
    const double2 wa = recA[(int)(v & 63)], wb = recB[(int)(v & 63)];
    const double4 w = make_double4(wa.x, wa.y, wb.x, wb.y);
    const double proj = m_fma(w.x, c, w.y * sn);
    const double perp = m_fma(w.x, sn, -(w.y * c));
    const double delta = m_fma(-perp, perp, w.z);
    return v != kSlotArm ? proj - l_sqrt(delta) : double(kSensorMax);     // :457-459
  };
  const double2 t0 = rayoff[l], t1 = rayoff[l + 64];
  A.rd0 = reading(t0.x, t0.y, v0);
  A.rd1 = reading(t1.x, t1.y, v1);
  B.rd0 = reading(t0.x, t0.y, v2);
  B.rd1 = reading(t1.x, t1.y, v3);
  // the records are read by every lane above before the caller's next writes to this buffer (the
  // wave's LDS instructions complete in order)
}

template <typename R, int LID, typename Row>
__device__ __forceinline__ void lidar_wave(const Row& E, int n, R px, R py, R sp, R cp,
                                           const typename Vec2<R>::T* rayoff, unsigned long long* slot,
                                           int* mark, Scan<R>& out) {
  const int l = lane_id();
  const bool valid = l < n;
  R ox = R(0), oy = R(0), rr = R(0);
  if (valid) E.get(l, ox, oy, rr);
  const R dx = ox - px, dy = oy - py, r2 = rr * rr;
  const R d = l_sqrt(m_fma(dx, dx, dy * dy));
  const R key = valid ? d - rr : big<R>();                                      // simple_env.py:205-206
  out.term = ballot(valid & (key < R(kTermDist))) != 0;                       // :334
  out.far = ballot(valid & (d >= R(0.99 * kSensorMax))) != 0;
  if constexpr (std::is_same<R, float>::value && (LID & kLidWindow) != 0) {
    const WinLds W{slot, mark, rayoff};
    if (!out.far) lidar_window<false>(dx, dy, key, d, rr, valid, px, py, sp, cp, W, E, out);
    else lidar_window<true>(dx, dy, key, d, rr, valid, px, py, sp, cp, W, E, out);
    return;
  }
  if constexpr (std::is_same<R, double>::value && (LID & kLidWindow) != 0) {
    const WinLdsD W{slot, mark, rayoff};
    if (!out.far) lidar_window_d<false>(dx, dy, key, d, rr, valid, sp, cp, W, out);
    else lidar_window_d<true>(dx, dy, key, d, rr, valid, sp, cp, W, out);
    return;
  }
  const auto t0 = rayoff[l], t1 = rayoff[l + 64];
  lidar_brute<R, LID & (kLidSkip | kLidUnroll2)>(dx, dy, r2, key, d, rr, valid, n, out.far, sp, cp,
                                                  t0.x, t0.y, t1.x, t1.y, out);
}

// Reset-kernel LDS carve (16-B aligned pieces):
//   [ray offset table 128 x Vec2][pair slots 4 waves x 128 x u64][owner marks 4 x 64 x i32]
//   [one obstacle row per wave: x[64], y[64], r[64]]
template <typename R> __host__ __device__ constexpr size_t lds_rayoff_bytes() { return 128 * 2 * sizeof(R); }
constexpr size_t kLdsSlotBytes = (size_t)kWaves * 128 * 8;
constexpr size_t kLdsMarkBytes = (size_t)kWaves * 64 * 4;
template <typename R> __host__ __device__ constexpr size_t lds_head_bytes() {
  return lds_rayoff_bytes<R>() + kLdsSlotBytes + kLdsMarkBytes;
}

// Block prologue shared by the step and reset kernels: ray-offset table and slot init.
template <typename R>
__device__ __forceinline__ void lds_prologue(const State<R>& S, char* lds, int tid) {
  auto* rayoff = reinterpret_cast<typename Vec2<R>::T*>(lds);
  auto* slots = reinterpret_cast<unsigned long long*>(lds + lds_rayoff_bytes<R>());
  if (tid < kSensors) rayoff[tid] = typename Vec2<R>::T{S.ray_tab[2 * tid], S.ray_tab[2 * tid + 1]};
  for (int i = tid; i < kWaves * 128; i += kBlock) slots[i] = kSlotArm;
}

}  // namespace usv
