// usv_legacy.hpp -- usv-asmc-v0 and the legacy float64 family (usv-asmc-ye-int-v0, usv-pid-v0): lane-per-env,
// no lidar.
#pragma once

#include "usv_reset.hpp"

namespace usv {

// --------------------------------------------------------------------------- usv-asmc-v0
// Legacy UsvAsmcEnv (id usv-asmc-v0, usv_asmc_env.py:14-401): one 0.01 s ASMC + plant step per
// env step, lane-per-env, no lidar.  The reference stores its state as float32 after every
// step (:247-251) and builds T, CRB, CA, Dl, Dn, J as float32 arrays (:191-222); NumPy 2 keeps
// scalar arithmetic on float32 operands in float32.  Those rounding points are reproduced
// (q32 / float arithmetic) so the f64 build tracks the reference to float32 rounding; the
// first step after a reset runs on the float64 reset state (:258-300), flagged by elapsed == 0.
constexpr double kV0MinSpeed = 0.3, kV0KAk = 5.72, kV0KYe = 0.5, kV0SigmaYe = 1.0;
constexpr double kV0CAction = 1.0 / (((kPi / 2) / 2 - (-kPi / 2) / 2) / H * (((kPi / 2) / 2 - (-kPi / 2) / 2) / H));
constexpr double kV0WAction = 0.2, kV0TMin = -30.0, kV0TMax = 36.5;
constexpr int kFamV0 = 0, kFamYeInt = 1, kFamPid = 2;   // usv-asmc-v0, usv-asmc-ye-int-v0, usv-pid-v0
constexpr double kYvK = 1.1 + 0.0045 * (1.01 / 0.09) - 0.1 * (0.27 / 0.09) + 0.016 * ((0.27 / 0.09) * (0.27 / 0.09));

template <typename R> __device__ __forceinline__ R q32(R x) { return R((float)x); }

// sin / cos of the legacy path angle ak.  The legacy resets put the target on the start's line
// (yd = y0, usv_asmc_env.py:277-282), so ak = atan2(0, xd - x0) = +0 in every episode: a wave whose
// lanes all hold ak = 0 takes sin 0 = 0, cos 0 = 1 (the values libm returns) without the two libm calls.
template <typename R> __device__ __forceinline__ void v0_path_sincos(R ak, R& sa, R& ca) {
  if (__builtin_amdgcn_ballot_w64(ak != R(0)) == 0) { sa = R(0); ca = R(1); }
  else { sa = m_sin(ak); ca = m_cos(ak); }
}

template <typename R>
__device__ __forceinline__ void v0_obs(float* row, R u, R v_ak, R r, R ye, R psi_ak, R a_last) {
  row[0] = (float)u; row[1] = (float)v_ak; row[2] = (float)r;
  row[3] = (float)ye; row[4] = (float)psi_ak; row[5] = (float)a_last;
}

// UsvAsmcEnv.reset (usv_asmc_env.py:258-300); Philox draws replace np.random.uniform.
// FAM 1 / 2 are the float64 legacy envs on the same template: UsvAsmcYeIntEnv.reset
// (usv_asmc_ye_int_env.py:256-296: x, y ~ U(-5, 5), speed ~ U(0.4, 1.4)) and UsvPidEnv.reset
// (usv_pid_env.py:236-276: speed ~ U(0.4, 1.4)); the draw order is the same in all three.
// NumPy-exact mode: np.random.uniform on the legacy global RandomState (MT19937, seeded by
// np.random.seed), one lane per env, key[624] + pos kept in S.npmt.  uniform = lo + (hi - lo) *
// ((a >> 5) * 2^26 + (b >> 6)) / 2^53 over two 32-bit draws (numpy's mt19937 next_double).
struct NpMt {
  uint32_t* k;     // key word i of this env at k[i * stride]
  size_t stride;
  __device__ uint32_t& key(int i) const { return k[(size_t)i * stride]; }
  __device__ void twist() const {
    constexpr uint32_t kA = 0x9908b0dfu, kU = 0x80000000u, kL = 0x7fffffffu;
    int i = 0;
    for (; i < 624 - 397; ++i) {
      const uint32_t y = (key(i) & kU) | (key(i + 1) & kL);
      key(i) = key(i + 397) ^ (y >> 1) ^ ((0u - (y & 1u)) & kA);
    }
    for (; i < 623; ++i) {
      const uint32_t y = (key(i) & kU) | (key(i + 1) & kL);
      key(i) = key(i + 397 - 624) ^ (y >> 1) ^ ((0u - (y & 1u)) & kA);
    }
    const uint32_t y = (key(623) & kU) | (key(0) & kL);
    key(623) = key(396) ^ (y >> 1) ^ ((0u - (y & 1u)) & kA);
    key(624) = 0;
  }
  __device__ uint32_t next32() const {
    if (key(624) >= 624) twist();
    const uint32_t p = key(624);
    key(624) = p + 1;
    uint32_t y = key((int)p);
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
  __device__ double uniform(double lo, double hi) const {
    const uint32_t a = next32() >> 5, b = next32() >> 6;
    return lo + (hi - lo) * ((a * 67108864.0 + b) / 9007199254740992.0);
  }
};

template <typename R, int FAM, typename G>
__device__ void v0_reset_draws(const State<R>& S, int e, float* row, int ep, G&& g);

template <typename R, int FAM = kFamV0>
__device__ void v0_reset(const State<R>& S, int e, float* row) {
  const int ep = S.I(I_EPISODE)[e];
  if (S.np_reset) {
    v0_reset_draws<R, FAM>(S, e, row, ep, NpMt{S.npmt + e, (size_t)S.fstride});
  } else {
    v0_reset_draws<R, FAM>(S, e, row, ep, Philox(S.seed, S.gid0 + (uint64_t)e, (uint32_t)ep));
  }
}

template <typename R, int FAM, typename G>
__device__ void v0_reset_draws(const State<R>& S, int e, float* row, int ep, G&& g) {
  const double lim = FAM == kFamYeInt ? 5.0 : 2.5;
  const double x = g.uniform(-lim, lim), y = g.uniform(-lim, lim);               // :260-261
  const double psi = g.uniform(-kPi, kPi);                                        // :262
  const double x0 = g.uniform(-2.5, 2.5), y0 = g.uniform(-2.5, 2.5);             // :275-276
  const double xd = g.uniform(15.0, 30.0), yd = y0;                              // :277-278
  const double ds = FAM == kFamV0 ? g.uniform(1.4, 2.4) : g.uniform(0.4, 1.4);   // :279
  const double ak = (double)(float)atan2(yd - y0, xd - x0);                       // :281-282
  const double psi_ak = (double)(float)wrap_once(psi - ak);                       // :284-286
  const double ye = -(x - x0) * sin(ak) + (y - y0) * cos(ak);                     // :287
  S.F(F_X)[e] = R(x); S.F(F_Y)[e] = R(y); S.F(F_PSI)[e] = R(psi);
  S.F(F_U)[e] = R(0); S.F(F_V)[e] = R(0); S.F(F_R)[e] = R(0);
  for (int i = 0; i < kV0Target; ++i) S.V(i)[e] = R(0);                          // last, aux
  const double tg[6] = {x0, y0, ds, ak, xd, yd};
  for (int i = 0; i < 6; ++i) S.V(kV0Target + i)[e] = R(tg[i]);
  S.V(kV0ALast)[e] = R(0);
  S.V(kV0Ye)[e] = R(0); S.V(kV0Ye + 1)[e] = R(0);                                 // ye_int, ye_last
  S.I(I_ELAPSED)[e] = 0;
  S.I(I_EPISODE)[e] = ep + 1;
  v0_obs<R>(row, R(0), R(0), R(0), R(ye), R(psi_ak), R(0));                      // :289-298
}

// The plant's f, C = CRB + CA and D = Dl - Dn (:132-145, :193-212) in the arithmetic the reference's state has: T =
// float on stored float32 state, T = R on the float64 reset state (the first step).  C and D are float32 arrays
// either way: each entry is computed in T and rounded, then the two arrays are added / subtracted in float32.
struct V0Mats { float c02, c12, c20, c21, d00, d11, d12, d21, d22; };

template <typename R, typename T>
__device__ __forceinline__ void v0_plant(T u, T v, T r, R xu, R xuu, R& fu, R& fpsi, V0Mats& m) {
  const T au = m_abs(u), av = m_abs(v), ar = m_abs(r);
  const T mag = m_sqrt(u * u + v * v);
  // :132-133 the factor holds np.power(0.27 / 0.09, 2), a float64 scalar: the last product is float64
  const R yv = R(T(0.5) * (T(-40 * 1000) * av)) * R(kYvK);
  const T yr = ((T(6 * (-3.141592 * 1000)) * mag) * T(0.09)) * T(0.09) * T(1.01);               // :134
  const T nv = ((T(0.06 * (-3.141592 * 1000)) * mag) * T(0.09)) * T(0.09) * T(1.01);            // :136
  const T nr = ((T(0.02 * (-3.141592 * 1000)) * mag) * T(0.09)) * T(0.09) * T(1.01) * T(1.01);  // :138
  fu = R((T(MASS - Y_V_DOT) * v * r + (T(xuu) * au + T(xu) * u)) / T(MASS - X_U_DOT));           // :144
  fpsi = R((T(-X_U_DOT + Y_V_DOT) * u * v + (nr * r)) / T(IZ - N_R_DOT));                        // :145
  const T k = T((Y_R_DOT + N_V_DOT) / 2);
  m.c02 = (float)(T(0) - T(MASS) * v) + (float)(T(2) * (T(Y_V_DOT) * v + k * r));
  m.c12 = (float)(T(MASS) * u) + (float)(T(0) - T(X_U_DOT * MASS) * u);
  m.c20 = (float)(T(MASS) * v) + (float)(T(2) * ((T(0 - Y_V_DOT) * v) - k * r));
  m.c21 = (float)(T(0) - T(MASS) * u) + (float)(T(X_U_DOT * MASS) * u);
  m.d00 = (float)(0 - xu) - (float)(T(xuu) * au);                                                // :207
  m.d11 = (float)(R(0) - yv) - (float)(T(YVV) * av + T(YVR) * ar);
  m.d12 = (float)(T(0) - yr) - (float)(T(YRV) * av + T(YRR) * ar);
  m.d21 = (float)(T(0) - nv) - (float)(T(NVV) * av + T(NVR) * ar);
  m.d22 = (float)(T(0) - nr) - (float)(T(NRV) * av + T(NRR) * ar);
}

// T - C nu - D nu (:214-215).  float32 nu: a float32 matmul, whose last row OpenBLAS's sgemv fused when the fixtures
// were written, fma(a22, x2, fma(a20, x0, a21 * x1)), rows 0 and 1 summed product by product; the fixture
// (tests/golden/legacy_scenes.npz) is the authority for that pattern.  float64 nu (first step): C and D are promoted
// and nothing is fused.
__device__ __forceinline__ void v0_rhs(const V0Mats& m, float t0, float t2, float u, float v, float r, float (&rhs)[3]) {
  rhs[0] = (t0 - m.c02 * r) - m.d00 * u;
  rhs[1] = (0.0f - m.c12 * r) - (m.d11 * v + m.d12 * r);
  rhs[2] = (t2 - __builtin_fmaf(m.c20, u, m.c21 * v)) - __builtin_fmaf(m.d22, r, m.d21 * v);
}
__device__ __forceinline__ void v0_rhs(const V0Mats& m, float t0, float t2, double u, double v, double r, double (&rhs)[3]) {
  rhs[0] = ((double)t0 - (double)m.c02 * r) - (double)m.d00 * u;
  rhs[1] = (0.0 - (double)m.c12 * r) - ((double)m.d11 * v + (double)m.d12 * r);
  rhs[2] = ((double)t2 - ((double)m.c20 * u + (double)m.c21 * v)) - ((double)m.d21 * v + (double)m.d22 * r);
}

template <typename R>
__global__ __launch_bounds__(kBlock) void v0_step_kernel(State<R> S, IO<R> io) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= S.N) return;
  const bool first = S.I(I_ELAPSED)[e] == 0;        // reference state still float64 (reset arrays)
  const float af = io.act[e];
  const R a = R(af);
  R u = S.F(F_U)[e], v = S.F(F_V)[e], r = S.F(F_R)[e];
  R x = S.F(F_X)[e], y = S.F(F_Y)[e], psi = S.F(F_PSI)[e];
  R e_u_int = S.V(kV0Aux)[e], ka_u = S.V(kV0Aux + 1)[e], ka_psi = S.V(kV0Aux + 2)[e];
  const R xd_l = S.V(0)[e], yd_l = S.V(1)[e], pd_l = S.V(2)[e];
  const R ud_l = S.V(3)[e], vd_l = S.V(4)[e], rd_l = S.V(5)[e];
  const R e_u_last = S.V(6)[e], kdu_l = S.V(7)[e], kdp_l = S.V(8)[e];
  const R x0 = S.V(kV0Target)[e], y0 = S.V(kV0Target + 1)[e], ds = S.V(kV0Target + 2)[e];
  const R ak = S.V(kV0Target + 3)[e];
  const R a_last = S.V(kV0ALast)[e];
  // action_dot (:120): float32 arithmetic once the stored state is float32
  const R action_dot = first ? (a - a_last) / R(H) : R((af - (float)a_last) / (float)H);
  const R psi_d = wrap_once(a + ak);                                             // :123-124
  const float uf = (float)u, vf = (float)v, rf = (float)r;                       // the stored float32 state
  // :128 and :164-165 compare a float32 scalar with a Python float once the state is float32: NumPy makes the
  // constant float32, so u = float32(1.2) is not fast and Ka = float32(kmin) is not above its minimum
  const bool fast = first ? m_abs(u) > R(1.2) : fabsf(uf) > 1.2f;                // :126-130
  const R xu = fast ? R(64.55) : R(-25.0), xuu = fast ? R(-70.92) : R(0.0);
  R fu, fpsi;
  V0Mats m;
  if (first) v0_plant<R, R>(u, v, r, xu, xuu, fu, fpsi, m);
  else v0_plant<R, float>(uf, vf, rf, xu, xuu, fu, fpsi, m);
  const R e_psi = wrap_once(psi_d - psi);                                        // :147-148
  const R e_psi_dot = R(0) - r;                                                  // :149
  const R u_psi = R(1) / (R(1) + m_exp(R(10) * (m_abs(e_psi) * R(2 / kPi) - R(0.5))));  // :153
  const R u_d = (ds - R(kV0MinSpeed)) * u_psi + R(kV0MinSpeed);                  // :155-156
  const R e_u = u_d - u;                                                         // :158
  e_u_int = R(H) * (e_u + e_u_last) / R(2) + e_u_int;                            // :159 (e_u_last stale)
  const R sig_u = e_u + R(LAMBDA_U) * e_u_int;                                   // :161
  const R sig_p = e_psi_dot + R(LAMBDA_PSI) * e_psi;                             // :162
  const bool up_u = first ? ka_u > R(KMIN_U) : (float)ka_u > (float)KMIN_U;
  const bool up_p = first ? ka_psi > R(KMIN_PSI) : (float)ka_psi > (float)KMIN_PSI;
  const R kdu = up_u ? R(K_U) * m_sign(m_abs(sig_u) - R(MU_U)) : R(KMIN_U);      // :164
  const R kdp = up_p ? R(K_PSI) * m_sign(m_abs(sig_p) - R(MU_PSI)) : R(KMIN_PSI);
  ka_u = R(H) * (kdu + kdu_l) / R(2) + ka_u;                                     // :167
  ka_psi = R(H) * (kdp + kdp_l) / R(2) + ka_psi;                                 // :170
  const R ua_u = -ka_u * m_sqrt(m_abs(sig_u)) * m_sign(sig_u) - R(K2_U) * sig_u;           // :173
  const R ua_p = -ka_psi * m_sqrt(m_abs(sig_p)) * m_sign(sig_p) - R(K2_PSI) * sig_p;       // :174
  const R tx = (R(LAMBDA_U) * e_u - fu - ua_u) / R(1.0 / (MASS - X_U_DOT));     // :176
  const R tz = (R(LAMBDA_PSI) * e_psi - fpsi - ua_p) / R(1.0 / (IZ - N_R_DOT));
  const R tport = m_clip(tx / R(2) + tz / R(B_TH), R(kV0TMin), R(kV0TMax));      // :179-185
  const R tstbd = m_clip(tx / R(2 * C_TH) - tz / R(B_TH * C_TH), R(kV0TMin), R(kV0TMax));
  const float t0 = (float)(tport + R(C_TH) * tstbd);                             // :191 float32 T
  const float t2 = (float)(R(0.5 * B_TH) * (tport - R(C_TH) * tstbd));
  R rhs0, rhs1, rhs2;
  if (first) {
    R q[3];
    v0_rhs(m, t0, t2, u, v, r, q);
    rhs0 = q[0]; rhs1 = q[1]; rhs2 = q[2];
  } else {
    float q[3];
    v0_rhs(m, t0, t2, uf, vf, rf, q);
    rhs0 = R(q[0]); rhs1 = R(q[1]); rhs2 = R(q[2]);
  }
  const R ud = R(MI00) * rhs0;                                                   // :214 M^-1 (f64)
  const R vd = R(MI11) * rhs1 + R(MI12) * rhs2;
  const R rd = R(MI21) * rhs1 + R(MI22) * rhs2;
  u = R(H) * (ud + ud_l) / R(2) + u;                                             // :216-217
  v = R(H) * (vd + vd_l) / R(2) + v;
  r = R(H) * (rd + rd_l) / R(2) + r;
  // J as float32 (:220-222): of the float32 heading, or the float64 reset heading rounded
  const R cj = first ? R((float)m_cos(psi)) : R(cosf((float)psi));
  const R sj = first ? R((float)m_sin(psi)) : R(sinf((float)psi));
  const R xd = cj * u - sj * v, yd = sj * u + cj * v, pd = r;                    // :224
  x = R(H) * (xd + xd_l) / R(2) + x;                                             // :225
  y = R(H) * (yd + yd_l) / R(2) + y;
  psi = wrap_once(R(H) * (pd + pd_l) / R(2) + psi);                              // :228-229
  const R psi_ak = wrap_once(psi - ak);                                          // :231-232
  R sak, cak;
  v0_path_sincos(ak, sak, cak);
  const R ye = -(x - x0) * sak + (y - y0) * cak;                                 // :234
  const R ye_abs = m_abs(ye);
  // compute_reward (:364-374)
  const R pa = m_abs(psi_ak);
  // c_action is a float64 scalar (np.power, :77): only the square is float32 on float32 state
  const R cad = R(-kV0CAction) * (first ? action_dot * action_dot : R((float)action_dot * (float)action_dot));
  const R r_act = R(kV0WAction) * tanh(cad);
  const R r_ye = ye_abs > R(kV0SigmaYe) ? m_exp(R(-kV0KYe) * ye_abs) : m_exp(R(-kV0KYe) * (ye_abs * ye_abs) / R(kV0SigmaYe));
  const R r_ak = -m_exp(R(kV0KAk) * (pa - R(kPi)));
  const R v_ak = m_sin(psi_ak) * u + m_cos(psi_ak) * v;                          // body_to_path :376-390
  const bool done = ye_abs > R(10) || m_abs(x) > R(30);                          // :241-245
  const int el = S.I(I_ELAPSED)[e] + 1;
  const bool trunc = !done && S.limit > 0 && el >= S.limit;
  io.rew[e] = done ? R(-1) : (pa < R(kPi / 2) ? r_act + r_ye : r_ak);
  io.term[e] = done;
  io.trunc[e] = trunc;
  if (io.done) io.done[e] = done | trunc;
  float* row = io.obs + (size_t)e * 6;
  // stored state (float32, :247-251)
  S.F(F_U)[e] = q32(u); S.F(F_V)[e] = q32(v); S.F(F_R)[e] = q32(r);
  S.F(F_X)[e] = q32(x); S.F(F_Y)[e] = q32(y); S.F(F_PSI)[e] = q32(psi);
  S.V(kV0Aux)[e] = q32(e_u_int); S.V(kV0Aux + 1)[e] = q32(ka_u); S.V(kV0Aux + 2)[e] = q32(ka_psi);
  S.V(0)[e] = q32(xd); S.V(1)[e] = q32(yd); S.V(2)[e] = q32(pd);
  S.V(3)[e] = q32(ud); S.V(4)[e] = q32(vd); S.V(5)[e] = q32(rd);
  S.V(6)[e] = q32(e_u_last); S.V(7)[e] = q32(kdu); S.V(8)[e] = q32(kdp);
  S.V(kV0ALast)[e] = a;
  S.I(I_ELAPSED)[e] = el;
  v0_obs<R>(row, u, v_ak, r, ye, psi_ak, a);
  if (done || trunc) {
    if (io.fobs) v0_obs<R>(io.fobs + (size_t)e * 6, u, v_ak, r, ye, psi_ak, a);
    if (S.autoreset == USV_AUTORESET_SAME_STEP) v0_reset<R, kFamV0>(S, e, row);
  }
}

template <typename R, int FAM>
__global__ __launch_bounds__(kBlock) void v0_reset_kernel(State<R> S, IO<R> io) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= S.N || (io.mask && !io.mask[e])) return;
  v0_reset<R, FAM>(S, e, io.obs + (size_t)e * 6);
}

// --------------------------------------------------------------------------- float64 legacy family
// UsvAsmcYeIntEnv (usv-asmc-ye-int-v0, usv_asmc_ye_int_env.py:92-253) and UsvPidEnv (usv-pid-v0,
// usv_pid_env.py:89-233): the usv-asmc-v0 plant with the state kept in float64 (no float32
// arrays), so the whole step runs in R.  Lane per env.  Statement order follows the reference
// (contraction is off in this translation unit), so the f64 build tracks it to libm ulps.
// Citations are usv_asmc_ye_int_env.py lines; usv_pid_env.py has the same statements 4 lines
// earlier (its control law: :148-155).
constexpr double kYeIntKI = 0.001;                                               // ye_int :51
constexpr double kPidKpU = 1.1, kPidKiU = 0.2, kPidKdU = 0.1, kPidKpPsi = 0.8, kPidKdPsi = 3.0;  // pid :40-44

template <typename R, int FAM>
__global__ __launch_bounds__(kBlock) void legacy_step_kernel(State<R> S, IO<R> io) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= S.N) return;
  const R a = R(io.act[e]);
  R u = S.F(F_U)[e], v = S.F(F_V)[e], r = S.F(F_R)[e];
  R x = S.F(F_X)[e], y = S.F(F_Y)[e], psi = S.F(F_PSI)[e];
  R e_u_int = S.V(kV0Aux)[e], ka_u = S.V(kV0Aux + 1)[e], ka_psi = S.V(kV0Aux + 2)[e];
  const R xd_l = S.V(0)[e], yd_l = S.V(1)[e], pd_l = S.V(2)[e];
  const R ud_l = S.V(3)[e], vd_l = S.V(4)[e], rd_l = S.V(5)[e];
  const R e_u_last = S.V(6)[e];
  R kdu = S.V(7)[e], kdp = S.V(8)[e];
  const R x0 = S.V(kV0Target)[e], y0 = S.V(kV0Target + 1)[e], ds = S.V(kV0Target + 2)[e];
  const R ak = S.V(kV0Target + 3)[e];
  const R action_dot = (a - S.V(kV0ALast)[e]) / R(H);                           // :113
  const R psi_d = wrap_once(a + ak);                                             // :116-117
  const bool fast = m_abs(u) > R(1.2);                                           // :119-123
  const R xu = fast ? R(64.55) : R(-25.0), xuu = fast ? R(-70.92) : R(0.0);
  const R mag = m_sqrt(u * u + v * v);                                           // :125-132
  const R yv = (R(0.5) * (R(-40 * 1000) * m_abs(v))) * R(kYvK);
  const R yr = (((R(6 * (-3.141592 * 1000)) * mag) * R(0.09)) * R(0.09)) * R(1.01);
  const R nv = (((R(0.06 * (-3.141592 * 1000)) * mag) * R(0.09)) * R(0.09)) * R(1.01);
  const R nr = ((((R(0.02 * (-3.141592 * 1000)) * mag) * R(0.09)) * R(0.09)) * R(1.01)) * R(1.01);
  const R f_u = ((R(MASS - Y_V_DOT) * v * r) + (xuu * m_abs(u) + xu * u)) / R(MASS - X_U_DOT);    // :137
  const R f_psi = ((R(-X_U_DOT + Y_V_DOT) * u * v) + (nr * r)) / R(IZ - N_R_DOT);                 // :138
  const R e_psi = wrap_once(psi_d - psi);                                        // :140-141
  const R e_psi_dot = R(0) - r;                                                  // :142
  const R u_psi = R(1) / (R(1) + m_exp(R(10) * (m_abs(e_psi) * R(2 / kPi) - R(0.5))));  // :146
  const R u_d = (ds - R(kV0MinSpeed)) * u_psi + R(kV0MinSpeed);                  // :148-149
  const R e_u = u_d - u;                                                         // :151
  e_u_int = R(H) * (e_u + e_u_last) / R(2) + e_u_int;                            // :152 (e_u_last stale)
  R tx, tz;
  if constexpr (FAM == kFamYeInt) {                                              // ASMC :154-170
    const R sig_u = e_u + R(LAMBDA_U) * e_u_int;
    const R sig_p = e_psi_dot + R(LAMBDA_PSI) * e_psi;
    const R kdu_n = ka_u > R(KMIN_U) ? R(K_U) * m_sign(m_abs(sig_u) - R(MU_U)) : R(KMIN_U);
    const R kdp_n = ka_psi > R(KMIN_PSI) ? R(K_PSI) * m_sign(m_abs(sig_p) - R(MU_PSI)) : R(KMIN_PSI);
    ka_u = R(H) * (kdu_n + kdu) / R(2) + ka_u;
    ka_psi = R(H) * (kdp_n + kdp) / R(2) + ka_psi;
    kdu = kdu_n; kdp = kdp_n;
    const R ua_u = (-ka_u * m_sqrt(m_abs(sig_u)) * m_sign(sig_u)) - R(K2_U) * sig_u;
    const R ua_p = (-ka_psi * m_sqrt(m_abs(sig_p)) * m_sign(sig_p)) - R(K2_PSI) * sig_p;
    tx = ((R(LAMBDA_U) * e_u) - f_u - ua_u) / R(1.0 / (MASS - X_U_DOT));
    tz = ((R(LAMBDA_PSI) * e_psi) - f_psi - ua_p) / R(1.0 / (IZ - N_R_DOT));
  } else {                                                                       // PID, pid :148-155
    const R e_u_dot = (e_u - e_u_last) / R(H);
    const R ua_u = (R(kPidKpU) * e_u) + (R(kPidKiU) * e_u_int) + (R(kPidKdU) * e_u_dot);
    const R ua_p = (R(kPidKpPsi) * e_psi) + (R(kPidKdPsi) * e_psi_dot);
    tx = (-f_u + ua_u) / R(1.0 / (MASS - X_U_DOT));
    tz = (-f_psi + ua_p) / R(1.0 / (IZ - N_R_DOT));
  }
  R tport = tx / R(2) + tz / R(B_TH);                                            // :172-178
  R tstbd = tx / R(2 * C_TH) - tz / R(B_TH * C_TH);
  tport = tport > R(kV0TMax) ? R(kV0TMax) : tport;
  tport = tport < R(kV0TMin) ? R(kV0TMin) : tport;
  tstbd = tstbd > R(kV0TMax) ? R(kV0TMax) : tstbd;
  tstbd = tstbd < R(kV0TMin) ? R(kV0TMin) : tstbd;
  const R t0 = tport + R(C_TH) * tstbd;                                          // :184
  const R t2 = R(0.5 * B_TH) * (tport - R(C_TH) * tstbd);
  // C = CRB + CA, D = Dl - Dn (:186-205): their non-zero entries
  const R c02 = (R(0) - R(MASS) * v) + R(2) * ((R(Y_V_DOT) * v) + R((Y_R_DOT + N_V_DOT) / 2) * r);
  const R c12 = (R(MASS) * u) + (R(0) - R(X_U_DOT * MASS) * u);
  const R c20 = (R(MASS) * v) + R(2) * ((R(0 - Y_V_DOT) * v) - R((Y_R_DOT + N_V_DOT) / 2) * r);
  const R c21 = (R(0) - R(MASS) * u) + (R(X_U_DOT * MASS) * u);
  const R av = m_abs(v), ar = m_abs(r);
  const R d00 = (R(0) - xu) - xuu * m_abs(u);
  const R d11 = (R(0) - yv) - (R(YVV) * av + R(YVR) * ar);
  const R d12 = (R(0) - yr) - (R(YRV) * av + R(YRR) * ar);
  const R d21 = (R(0) - nv) - (R(NVV) * av + R(NVR) * ar);
  const R d22 = (R(0) - nr) - (R(NRV) * av + R(NRR) * ar);
  const R rhs0 = (t0 - c02 * r) - d00 * u;                                       // :207-208
  const R rhs1 = (R(0) - c12 * r) - (d11 * v + d12 * r);
  const R rhs2 = (t2 - (c20 * u + c21 * v)) - (d21 * v + d22 * r);
  const R ud = R(MI00) * rhs0;                                                   // M^-1 (block form)
  const R vd = R(MI11) * rhs1 + R(MI12) * rhs2;
  const R rd = R(MI21) * rhs1 + R(MI22) * rhs2;
  u = R(H) * (ud + ud_l) / R(2) + u;                                             // :209-211
  v = R(H) * (vd + vd_l) / R(2) + v;
  r = R(H) * (rd + rd_l) / R(2) + r;
  const R cj = m_cos(psi), sj = m_sin(psi);                                      // J(psi) :213-215
  const R xd = cj * u - sj * v, yd = sj * u + cj * v, pd = r;
  x = R(H) * (xd + xd_l) / R(2) + x;                                             // :217-219
  y = R(H) * (yd + yd_l) / R(2) + y;
  psi = wrap_once(R(H) * (pd + pd_l) / R(2) + psi);                              // :221-222
  const R psi_ak = wrap_once(psi - ak);                                          // :224-225
  R sak, cak;
  v0_path_sincos(ak, sak, cak);
  const R ye = -(x - x0) * sak + (y - y0) * cak;                                 // :227
  const R ye_abs = m_abs(ye);
  const R pa = m_abs(psi_ak);
  const R r_act = R(kV0WAction) * tanh(R(-kV0CAction) * (action_dot * action_dot));
  const R r_ak = -m_exp(R(kV0KAk) * (pa - R(kPi)));
  R ye_obs = ye, reward;
  if constexpr (FAM == kFamYeInt) {
    R ye_int = S.V(kV0Ye)[e];
    const R ye_last = S.V(kV0Ye + 1)[e];
    if (m_sign(ye) != m_sign(ye_last)) ye_int = R(0);                            // :230-231
    ye_int = R(H) * (ye + ye_last) + ye_int;                                     // :232
    ye_obs = ye + R(kYeIntKI) * ye_int;                                          // ye_ss :235
    S.V(kV0Ye)[e] = ye_int;
    S.V(kV0Ye + 1)[e] = ye;
    reward = r_act + (pa < R(kPi / 2) ? m_exp(R(-kV0KYe) * ye_abs) : r_ak);      // :350-360
  } else {
    const R r_ye = ye_abs > R(kV0SigmaYe) ? m_exp(R(-kV0KYe) * ye_abs)
                                          : m_exp(R(-kV0KYe) * (ye_abs * ye_abs) / R(kV0SigmaYe));
    reward = pa < R(kPi / 2) ? r_act + r_ye : r_ak;                              // pid :329-338
  }
  const R v_ak = m_sin(psi_ak) * u + m_cos(psi_ak) * v;                          // body_to_path :239
  const bool done = ye_abs > R(10) || x < R(-10);                                // :241-245
  const int el = S.I(I_ELAPSED)[e] + 1;
  const bool trunc = !done && S.limit > 0 && el >= S.limit;
  io.rew[e] = done ? R(-1) : reward;
  io.term[e] = done;
  io.trunc[e] = trunc;
  if (io.done) io.done[e] = done | trunc;
  S.F(F_U)[e] = u; S.F(F_V)[e] = v; S.F(F_R)[e] = r;                             // :247-251
  S.F(F_X)[e] = x; S.F(F_Y)[e] = y; S.F(F_PSI)[e] = psi;
  S.V(kV0Aux)[e] = e_u_int; S.V(kV0Aux + 1)[e] = ka_u; S.V(kV0Aux + 2)[e] = ka_psi;
  S.V(0)[e] = xd; S.V(1)[e] = yd; S.V(2)[e] = pd;
  S.V(3)[e] = ud; S.V(4)[e] = vd; S.V(5)[e] = rd;
  S.V(7)[e] = kdu; S.V(8)[e] = kdp;
  S.V(kV0ALast)[e] = a;
  S.I(I_ELAPSED)[e] = el;
  float* row = io.obs + (size_t)e * 6;
  v0_obs<R>(row, u, v_ak, r, ye_obs, psi_ak, a);
  if (done || trunc) {
    if (io.fobs) v0_obs<R>(io.fobs + (size_t)e * 6, u, v_ak, r, ye_obs, psi_ak, a);
    if (S.autoreset == USV_AUTORESET_SAME_STEP) v0_reset<R, FAM>(S, e, row);
  }
}

}  // namespace usv
