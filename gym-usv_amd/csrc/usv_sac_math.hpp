// usv_sac_math.hpp -- the arithmetic of the fused SAC update (usv_sac.hpp): SB3's SAC.train lines for the TD target,
// the twin-critic loss, the actor loss and the entropy-coefficient loss (sac/sac.py; TD3's target without the
// entropy term) and common/utils.py's polyak_update.  Plain C++ marked __host__ __device__, no HIP types: the
// kernels and a stand-alone host program (tests/test_sac_loss_math.py) run the same functions in the same order.
// All f32, every operation rounded on its own (contraction is off in every function here).
//
// Critic, per row i of B (sac_target, sac_critic_row):
//   qn   = min(q1t, q2t);  with an entropy term  qn = qn - ent logp_next
//   tgt  = r + ((1 - d) disc) qn                  Python's left-to-right order; disc the row's discount or gamma
//   d1   = q1 - tgt;  d2 = q2 - tgt
//   loss = 0.5 (S(d1 d1) / B + S(d2 d2) / B)      F.mse_loss twice; S the sum below, / B = / float(B)
//   g_q1 = d1 / B;  g_q2 = d2 / B                 the gradients at unit upstream; tgt carries none
// Policy, per row (sac_policy_row):
//   qmin          = min(q1p, q2p)
//   actor_loss    = S(ent logp - qmin) / B
//   ent_coef_loss = -(S(log_ent (logp + te)) / B)                te the target entropy
//   g_logp = ent / B;  g_q1p = -w / B;  g_q2p = -(1 - w) / B     w = 1, 0.5, 0 for q1p <, ==, > q2p (torch.min's ties
//                                                                under autograd; an unordered pair: w = 0)
//   g_log_ent     = -(S(logp + te) / B)
// ent is data (SB3 detaches it).  min propagates NaN as torch.min does (sac_min).
//
// The sum S over rows.  Rows are split into partials of kSacPartialRows = P = 1024 consecutive rows.  Within a
// partial, strand s of kSacStrands = 256 adds its rows s, s + 256, s + 512, s + 768 of the partial (those that
// exist) in ascending order from +0.0f; strands 64 w .. 64 w + 63 are added by sde_tree_sum (usv_sde_math.hpp: a
// balanced binary tree, neighbours first) into wave sum w, and the partial is (w0 + w1) + (w2 + w3).  The partials
// are added in ascending order from +0.0f (sac_sum).  Nothing in this depends on a grid size or on which block ends
// last.
//
// Polyak (polyak_coeffs, polyak_value):  t' = (t om) + (tau_f p) with tau_f = float(tau) and om = float(1.0 - tau),
// the subtraction in double as Python does it before torch casts the scalar: three roundings, torch's two-op
// t.mul_(1 - tau).add_(p, alpha=tau) without a fused multiply-add.  A tensor is cut into chunks of
// kPolyakChunk = C = 4096 elements, one block each (polyak_chunks).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "usv_sde_math.hpp"

#if defined(__HIP__) || defined(__CUDACC__)
#define USV_SAC_HD __host__ __device__ inline
#else
#define USV_SAC_HD inline
#endif

namespace usv {

constexpr int kSacStrands = 256;                   // strands of a partial = threads of a block
constexpr int kSacStrandRows = 4;                  // rows of a strand
constexpr int kSacPartialRows = kSacStrands * kSacStrandRows;   // P
constexpr int kSacWaves = kSacStrands / kSdeLanes;
constexpr int kSacScratchHead = 4;                 // floats in front of the partials: the ticket word, padded to 16 B
constexpr int kSacScratchSums = 3;                 // floats per partial (the policy's three sums; the critic uses two)
constexpr int kPolyakChunk = 4096;                 // C

USV_SAC_HD int64_t sac_partials(int64_t rows) { return (rows + kSacPartialRows - 1) / kSacPartialRows; }
USV_SAC_HD size_t sac_scratch_floats(int64_t rows) {
  return (size_t)kSacScratchHead + (size_t)kSacScratchSums * (size_t)sac_partials(rows);
}
USV_SAC_HD int64_t polyak_chunks(int64_t numel) { return (numel + kPolyakChunk - 1) / kPolyakChunk; }

// torch.min(a, b): a NaN in either operand gives NaN.
USV_SAC_HD float sac_min(float a, float b) { return (b < a || b != b) ? b : a; }

USV_SAC_HD float sac_mean(float sum, int64_t B) { return sum / (float)B; }

USV_SAC_HD float sac_target(float q1t, float q2t, bool with_ent, float ent, float logp_next, float r, float d,
                            float disc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float qn = sac_min(q1t, q2t);
  if (with_ent) qn = qn - ent * logp_next;
  return r + ((1.0f - d) * disc) * qn;
}

// One row of the critic: the differences, their squares (the terms of the two sums) and the unit gradients.
USV_SAC_HD void sac_critic_row(float q1, float q2, float tgt, int64_t B, float& t1, float& t2, float& g1, float& g2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float d1 = q1 - tgt, d2 = q2 - tgt;
  t1 = d1 * d1;
  t2 = d2 * d2;
  g1 = d1 / (float)B;
  g2 = d2 / (float)B;
}

USV_SAC_HD float sac_critic_loss(float s1, float s2, int64_t B) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return 0.5f * (sac_mean(s1, B) + sac_mean(s2, B));
}

// One row of the policy: the terms of the three sums (te, tg unused without a log_ent) and the q gradients.
USV_SAC_HD void sac_policy_row(float logp, float q1p, float q2p, float ent, float log_ent, float te, int64_t B,
                               float& ta, float& tl, float& tg, float& g1, float& g2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float qmin = sac_min(q1p, q2p);
  ta = ent * logp - qmin;
  tg = logp + te;
  tl = log_ent * tg;
  const float w = q1p < q2p ? 1.0f : (q1p == q2p ? 0.5f : 0.0f);
  g1 = -w / (float)B;
  g2 = -(1.0f - w) / (float)B;
}

USV_SAC_HD float sac_neg_mean(float sum, int64_t B) { return -sac_mean(sum, B); }

// The four wave sums of a partial.
USV_SAC_HD float sac_waves_sum(const float (&w)[kSacWaves]) {
  static_assert(kSacWaves == 4, "the partial is (w0 + w1) + (w2 + w3)");
  return (w[0] + w[1]) + (w[2] + w[3]);
}

// One partial of `count` <= P terms: strands, the tree over each wave's strands, the four wave sums.
USV_SAC_HD float sac_partial_sum(const float* term, int64_t count) {
  float w[kSacWaves];
  for (int v = 0; v < kSacWaves; ++v) {
    float s[kSdeLanes];
    for (int l = 0; l < kSdeLanes; ++l) {
      float acc = 0.0f;
      for (int64_t i = (int64_t)v * kSdeLanes + l; i < count; i += kSacStrands) acc = acc + term[i];
      s[l] = acc;
    }
    w[v] = sde_tree_sum(s);
  }
  return sac_waves_sum(w);
}

// The partials in ascending order from +0.0f.
USV_SAC_HD float sac_partials_sum(const float* part, size_t stride, int64_t partials) {
  float acc = 0.0f;
  for (int64_t p = 0; p < partials; ++p) acc = acc + part[(size_t)p * stride];
  return acc;
}

// S: the sum of B terms.
inline float sac_sum(const float* term, int64_t B) {
  float acc = 0.0f;
  for (int64_t at = 0; at < B; at += kSacPartialRows)
    acc = acc + sac_partial_sum(term + at, B - at < kSacPartialRows ? B - at : kSacPartialRows);
  return acc;
}

USV_SAC_HD bool polyak_tau_ok(double tau) { return tau >= 0.0 && tau <= 1.0; }
USV_SAC_HD void polyak_coeffs(double tau, float& tau_f, float& om) {
  tau_f = (float)tau;
  om = (float)(1.0 - tau);
}
USV_SAC_HD float polyak_value(float t, float p, float tau_f, float om) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (t * om) + (tau_f * p);
}

}  // namespace usv
