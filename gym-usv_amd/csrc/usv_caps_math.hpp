// usv_caps_math.hpp -- the arithmetic of the CAPS smoothness regulariser (usv_caps.hpp): Conditioning for Action
// Policy Smoothness (Mysore et al., ICRA 2021), the lambda_t / lambda_s / eps_s keys of the reference's config_sac.
// Plain C++ marked __host__ __device__, no HIP types: the kernels and a stand-alone host program
// (tests/test_caps_math.py) run the same functions in the same order.  All f32, every operation rounded on its own
// (contraction is off in every function here).
//
// Perturbation (caps_block_normals, caps_near):  element j of row r of a [B, W] array takes normal j % 4 of Philox
// block j / 4 with
//   key     = (seed lo, seed hi)              the caller's 64-bit seed, unmodified
//   counter = (r lo, r hi, epoch, j / 4)      usv_sde_math.hpp's sde_block(seed, r, epoch, j / 4) and sde_normals
//   out     = obs + (eps z)
// A row's noise depends on its index alone, not on B.
//
// Loss, per row i of B with A <= kCapsMaxAct elements, k ascending (caps_row):
//   a_k = squash ? tanhf(mean_k) : mean_k;  b_k from mean_next, c_k from mean_near likewise
//   dt_k = a_k - b_k;  ds_k = a_k - c_k
//   nT = sqrtf(sum_k dt_k dt_k);  nS = sqrtf(sum_k ds_k ds_k)       the sums ascending from +0.0f
//   temporal = S(nT) / B;  spatial = S(nS) / B                      S: usv_sac_math.hpp's sum over rows, / float(B)
//   loss = (lambda_t temporal) + (lambda_s spatial)                 (caps_loss)
// The gradients of loss at unit upstream:
//   wT = nT == 0 ? 0 : (lambda_t / B) / nT;  wS likewise            torch's subgradient 0 of a norm at 0; NaN stays
//   eT_k = wT dt_k;  eS_k = wS ds_k
//   g_mean_k = (eT_k + eS_k) da_k;  g_next_k = (-eT_k) db_k;  g_near_k = (-eS_k) dc_k
//   da_k = 1 - a_k a_k when squashing (db_k, dc_k likewise); without squashing the factor is left out.
#pragma once

#include "usv_sac_math.hpp"

namespace usv {

constexpr int kCapsMaxAct = 8;

USV_SAC_HD bool caps_act_ok(int64_t A) { return A >= 1 && A <= kCapsMaxAct; }
// eps, lambda_t, lambda_s: finite and >= 0
USV_SAC_HD bool caps_weight_ok(float w) { return w >= 0.0f && w <= 3.40282346638528859812e38f; }
USV_SAC_HD int64_t caps_row_blocks(int64_t W) { return (W + 3) / 4; }

// The four normals of block b of row r.
USV_SAC_HD void caps_block_normals(uint64_t seed, uint64_t r, uint32_t epoch, uint32_t b, float (&z)[4]) {
  uint32_t o[4];
  sde_block(seed, r, epoch, b, o);
  sde_normals(o, z);
}

USV_SAC_HD float caps_near(float obs, float eps, float z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return obs + (eps * z);
}

// One action of a row: pi and, when squashing, d pi / d mean.
USV_SAC_HD void caps_pi(float m, bool squash, float& a, float& da) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  a = squash ? tanhf(m) : m;
  da = squash ? 1.0f - a * a : 1.0f;
}

USV_SAC_HD float caps_unit_weight(float lambda, float n, int64_t B) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return n == 0.0f ? 0.0f : (lambda / (float)B) / n;
}

// One row: the two distances (the terms of the two sums) and, where g is set, the three unit gradients.
template <int A>
USV_SAC_HD void caps_row(const float (&m)[A], const float (&mn)[A], const float (&mr)[A], bool squash, float lambda_t,
                         float lambda_s, int64_t B, float& nT, float& nS, bool g, float (&g_mean)[A], float (&g_next)[A],
                         float (&g_near)[A]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  static_assert(A >= 1 && A <= kCapsMaxAct, "act_dim");
  float dt[A], ds[A], da[A], db[A], dc[A];
  float sT = 0.0f, sS = 0.0f;
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < A; ++k) {
    float a, b, c;
    caps_pi(m[k], squash, a, da[k]);
    caps_pi(mn[k], squash, b, db[k]);
    caps_pi(mr[k], squash, c, dc[k]);
    dt[k] = a - b;
    ds[k] = a - c;
    sT = sT + dt[k] * dt[k];
    sS = sS + ds[k] * ds[k];
  }
  nT = sqrtf(sT);
  nS = sqrtf(sS);
  if (!g) return;
  const float wT = caps_unit_weight(lambda_t, nT, B), wS = caps_unit_weight(lambda_s, nS, B);
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 0; k < A; ++k) {
    const float eT = wT * dt[k], eS = wS * ds[k];
    const float gm = eT + eS;
    g_mean[k] = squash ? gm * da[k] : gm;
    g_next[k] = squash ? (-eT) * db[k] : -eT;
    g_near[k] = squash ? (-eS) * dc[k] : -eS;
  }
}

// (loss, temporal, spatial) from the two sums over rows.
USV_SAC_HD void caps_loss(float sumT, float sumS, float lambda_t, float lambda_s, int64_t B, float (&out)[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  out[1] = sac_mean(sumT, B);
  out[2] = sac_mean(sumS, B);
  out[0] = (lambda_t * out[1]) + (lambda_s * out[2]);
}

}  // namespace usv
