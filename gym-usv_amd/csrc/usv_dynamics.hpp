// usv_dynamics.hpp -- UsvAsmc.compute on its own (asmc_compute_kernel), the env step's ASMC chain and the
// per-env dynamics, reward terms and truncation (env_dynamics).
#pragma once

#include "usv_state.hpp"

namespace usv {

// --------------------------------------------------------------------------- UsvAsmc.compute
// The controller on its own (gym_usv/control/usv_asmc.py:53-244), lane per controller: `calls`
// back-to-back compute() calls of 10 substeps each on [n][3] poses / velocities and the [16][n]
// state (asmc_substep's layout).  Same substep functions as the env step; the f32 build applies
// asmc_substep_f32's per-call pose accumulation (10 substeps here, 20 in an env step).
template <typename R>
__global__ __launch_bounds__(kBlock) void asmc_compute_kernel(int n, const R* __restrict__ act, R* pos, R* vel,
                                                              R* st, int* pstep, int perturb, int calls) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  R s[kAsmcN];
#pragma unroll
  for (int i = 0; i < kAsmcN; ++i) s[i] = st[(size_t)i * n + e];
  R x = pos[3 * (size_t)e], y = pos[3 * (size_t)e + 1], psi = pos[3 * (size_t)e + 2];
  R u = vel[3 * (size_t)e], v = vel[3 * (size_t)e + 1], r = vel[3 * (size_t)e + 2];
  const R a0 = act[2 * (size_t)e], a1 = act[2 * (size_t)e + 1];
  int ps = pstep ? pstep[e] : 0;
  const bool pert = perturb != 0;
  for (int c = 0; c < calls; ++c) {
    if constexpr (std::is_same<R, float>::value) {
      float xl = 0.0f, yl = 0.0f, pl = 0.0f;
      const float kt = rintf(psi * 0.159154943f);
      const AsmcRun e0 = asmc_run_begin(s, psi);
      for (int k = 0; k < 10; ++k) asmc_substep_f32(s, a0, a1, x, y, psi, u, v, r, xl, yl, pl, kt, ps + k, pert);
      asmc_run_end(x, y, psi, xl, yl, pl, e0, s);
    } else {
      for (int k = 0; k < 10; ++k) asmc_substep<R>(s, a0, a1, x, y, psi, u, v, r, ps + k, pert);
    }
    ps += 10;                                                   // perturb_step (:199)
  }
#pragma unroll
  for (int i = 0; i < kAsmcN; ++i) st[(size_t)i * n + e] = s[i];
  pos[3 * (size_t)e] = x; pos[3 * (size_t)e + 1] = y; pos[3 * (size_t)e + 2] = psi;
  vel[3 * (size_t)e] = u; vel[3 * (size_t)e + 1] = v; vel[3 * (size_t)e + 2] = r;
  if (pstep) pstep[e] = ps;
}

// --------------------------------------------------------------------------- phase 1
// usv-asmc-simple's two UsvAsmc.compute calls (simple_env_asmc.py:19-25, usv_asmc.py:53-244) on env
// e's pose and velocity, in registers; the ASMC state is loaded and stored here.
template <typename R>
__device__ __forceinline__ void asmc_env_chain(const State<R>& S, int e, int el0, float a_u, float a_r, R& x,
                                               R& y, R& psi, R& u, R& v, R& r, R* psi_d_last = nullptr) {
  // psi_d_last given: row 0 (psi_d_last) is returned there and not stored (the caller rebases it)
  {
    R s[kAsmcN];
#pragma unroll
    for (int i = 0; i < kAsmcN; ++i) s[i] = S.asmc[(size_t)i * S.N + e];
    const R c0 = R(a_u), c1 = R(a_r);
    // perturb_step of the episode's UsvAsmc: 2 compute() x 10 substeps per env step (usv_asmc.py:199)
    const bool pert = S.perturb != 0;
    if constexpr (std::is_same<R, float>::value) {
      float xl = 0.0f, yl = 0.0f, pl = 0.0f;        // position sums, heading compensation (asmc_substep_f32)
      const float kt = rintf(psi * 0.159154943f);    // whole turns of the heading (asmc_substep_f32's J)
      const AsmcRun e0 = asmc_run_begin(s, psi);    // eta_dot_last and psi before the run (asmc_run_end)
      // perturbation hoisted out of the substep loop, so the common loop unrolls (by 4): no
      // loop-carried register rotation (the s[1..3], s[4..9] moves) and the scheduler fills one
      // substep's hazard nops with the next one's independent work (dyn_rec_kernel 13.6 -> 11.4 us
      // at 65 536 envs)
      if (pert) {
        for (int k = 0; k < 20; ++k) asmc_substep_f32(s, c0, c1, x, y, psi, u, v, r, xl, yl, pl, kt, 20 * el0 + k, true);
      } else {
#pragma unroll 4
        for (int k = 0; k < 20; ++k) asmc_substep_f32(s, c0, c1, x, y, psi, u, v, r, xl, yl, pl, kt, 0, false);
      }
      asmc_run_end(x, y, psi, xl, yl, pl, e0, s);
    } else {
      if (pert) {
        for (int k = 0; k < 20; ++k) asmc_substep<R>(s, c0, c1, x, y, psi, u, v, r, 20 * el0 + k, true);
      } else {
#pragma unroll 4
        for (int k = 0; k < 20; ++k) asmc_substep<R>(s, c0, c1, x, y, psi, u, v, r, 0, false);
      }
    }
#pragma unroll
    for (int i = psi_d_last ? 1 : 0; i < kAsmcN; ++i) S.asmc[(size_t)i * S.N + e] = s[i];
    if (psi_d_last) *psi_d_last = s[0];
  }
}

// UsvSimpleEnv.step kinematics..reward terms (simple_env.py:310-346); for usv-asmc-simple
// first 2x UsvAsmc.compute (simple_env_asmc.py:18-27) and then step(zeros(2)).
// Also returns sin/cos of the new heading so the wave-per-env lidar does not recompute them.
// CHAIN = false (usv-asmc-simple only): asmc_chain_kernel already ran the two compute() calls and
// stored the pose and velocity they left; this is then UsvSimpleEnv.step(zeros(2)) on them.
template <typename R, int MODE, bool CHAIN = true>
__device__ void env_dynamics(const State<R>& S, int e, float a_u, float a_r, float (&hdr)[kHdr],
                             R& px, R& py, R& psp, R& pcp, R& partial, bool& trunc, R* info = nullptr) {
  R x = S.F(F_X)[e], y = S.F(F_Y)[e], psi = S.F(F_PSI)[e];
  R u = S.F(F_U)[e], v = S.F(F_V)[e], r = S.F(F_R)[e];
  const int el0 = S.I(I_ELAPSED)[e];
  constexpr bool kF32 = std::is_same<R, float>::value;
  constexpr bool kAsmc = MODE == USV_MODE_ASMC_SIMPLE;
  int k0 = 0;                                        // f32: the heading's whole turns (store_heading)
  R pdl = R(0);                                      // f32 usv-asmc-simple: psi_d_last, phi's frame
  if constexpr (kF32) {
    k0 = S.I(I_TURNS)[e];
    if constexpr (kAsmc && !CHAIN) pdl = S.asmc[e];
  }
  // every load of the step before its first store (the state stores go out early, below): with one
  // in-order vmcnt counter a load issued after a store returns only once that store is acknowledged
  const R lu = S.F(F_LAST_U)[e], lr = S.F(F_LAST_R)[e];
  const R mu = S.F(F_MAX_U)[e], mr = S.F(F_MAX_R)[e], refv = S.F(F_REF_V)[e];
  const R x0 = S.F(F_PX0)[e], y0 = S.F(F_PY0)[e];
  const R x1 = S.F(F_PX1)[e], y1 = S.F(F_PY1)[e];
  const R prog0 = S.F(F_PROGRESS)[e];
  if (kAsmc) {
    if constexpr (CHAIN) asmc_env_chain<R>(S, e, el0, a_u, a_r, x, y, psi, u, v, r, kF32 ? &pdl : nullptr);
    a_u = 0.0f;                                                                   // step(zeros(2))
    a_r = 0.0f;
  }
  // action = max_action * insert(action, 1, 0); filtered 0.8/0.2 (:311-317)
  const R a3u = R(0.8) * lu + R(0.2) * (mu * R(a_u));
  const R a3r = R(0.8) * lr + R(0.2) * (mr * R(a_r));
  // per-step acceleration clip, then speed clip; max_action[1] = 0 pins v to 0 (:320-321)
  const R dvu = m_clip(a3u - u, R(-kMaxAccU), R(kMaxAccU));
  const R dvr = m_clip(a3r - r, R(-kMaxAccR), R(kMaxAccR));
  u = m_clip(u + dvu, -mu, mu);
  v = R(0);
  r = m_clip(r + dvr, -mr, mr);
  R sp, cp;
  fx_sincos(psi, &sp, &cp);
  x = x + (u * cp) * R(kDt);                                                      // :322-324
  y = y + (u * sp) * R(kDt);
  psi = psi + r * R(kDt);
  // _get_closest_point (:139-148)
  const R dx = x1 - x0, dy = y1 - y0;
  const R det = dx * dx + dy * dy;
  R a = dyn_div(dy * (y - y0) + dx * (x - x0), det);
  a = a + R(kLookahead);
  a = m_clip(a, prog0, R(1));
  const int el = el0 + 1;
  // the state stores, as soon as the new state exists (their acknowledgements then overlap the rest
  // of phase 1; a same-step reset by another wave orders itself after them: step_q_body)
  {
    R ps = psi;
    if constexpr (kF32) {                            // the rebase (see the heading representation)
      // branch-free and stored unconditionally (n = 0 leaves both values unchanged, bit for bit): a
      // conditional store made the compiler sink the k0 load into its branch, and a wave with one
      // rebasing lane then waited a memory round trip in the middle of phase 1
      const float n = turns_of(psi);
      ps = sub_turns(psi, n);
      S.I(I_TURNS)[e] = k0 + (int)n;
      if constexpr (kAsmc) S.asmc[e] = sub_turns(pdl, n);   // (the chain left row 0 to this store)
    }
    S.F(F_X)[e] = x; S.F(F_Y)[e] = y; S.F(F_PSI)[e] = ps;
    S.F(F_U)[e] = u; S.F(F_V)[e] = v; S.F(F_R)[e] = r;
    S.F(F_LAST_U)[e] = a3u; S.F(F_LAST_R)[e] = a3r;
    S.F(F_PROGRESS)[e] = a;
    S.I(I_ELAPSED)[e] = el;
    S.I(I_SCAN)[e] = 1;
  }
  const R tx = x0 + a * dx, ty = y0 + a * dy;
  // _get_ye (:133-137): sin/cos of the path angle a_k = atan2(dy, dx) are dy/|d|, dx/|d|
  const R inv_len = dyn_div(R(1), dyn_sqrt(det));
  const R sak = dy * inv_len, cak = dx * inv_len;
  const R ye = -(x - x0) * sak + (y - y0) * cak;
  // _get_angle_to_target (:67-69), distance (:74)
  const R angle = wrap_angle(fx_atan2(ty - y, tx - x) - psi);
  const R ddx = x - tx, ddy = y - ty;
  const R dist = dyn_sqrt(ddx * ddx + ddy * ddy);
  trunc = (x > R(kBound)) | (x < R(0)) | (y > R(kBound)) | (y < R(0)) |   // :336
          (S.limit > 0 && el >= S.limit);                                 // TimeLimit
  make_header<R>(hdr, u, v, r, angle, dist, ye, refv, lu, lr, mu, mr);   // obs uses PREVIOUS action
  // _get_reward without the collision term (:150-186)
  const R dact = m_abs(lu - a3u) + m_abs(lr - a3r);
  const R yk = cdiv(ye, kYeK);
  const R e1 = fx_exp(-m_abs(yk)), e2 = fx_exp(-(yk * yk));
  const R ye_r = e1 > e2 ? e1 : e2;
  const R ang_r = fx_exp(-m_abs(angle));
  const R vel_r = fx_exp(-m_abs(dyn_sqrt(u * u + v * v) - refv)) * R(0.05);
  const R dact_r = -(dact / R(2)) * R(0.15);
  partial = ye_r + ang_r + vel_r + dact_r;
  if (info) {                                        // _get_info + reward_info (:102-115, :189-199)
    const R vals[USV_INFO_DIM] = {x, y, heading_abs(psi, k0), u, v, r,
                                  x0, y0, x1, y1, a3u, a3r, ye,
                                  cdiv(angle, kPi), ye_r, ang_r, dact_r, dact, vel_r, refv, lu, lu - refv};
#pragma unroll
    for (int i = 0; i < USV_INFO_DIM; ++i) info[i] = vals[i];
  }
  px = x; py = y;
  heading_sincos(psi, &psp, &pcp);
}

}  // namespace usv
