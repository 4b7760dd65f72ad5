// usv_ppo_math.hpp -- the arithmetic of the fused PPO loss (usv_ppo.hpp): the loss lines of SB3's PPO.train
// (ppo/ppo.py) for one minibatch of B rows, their statistics and common/utils.py's explained_variance.  Plain C++
// marked __host__ __device__, no HIP types: the kernels and a stand-alone host program
// (tests/test_ppo_loss_math.py) run the same functions in the same order.  All f32, every operation rounded on its
// own (contraction is off in every function here), / B = / float(B).
//
// The sum S over rows is usv_sac_math.hpp's: partials of 1024 rows, 256 strands, the tree over each wave's strands,
// (w0 + w1) + (w2 + w3), the partials in ascending order.  A partial carries kPpoSums = 5 sums here.
//
// Moments, with normalisation and B > 1 (SB3's len(advantages) > 1 guard), two passes (ppo_mean, ppo_sqdev, ppo_std):
//   mean = S(adv) / B;   d_i = adv_i - mean;   std = sqrtf(S(d_i d_i) / float(B - 1))         torch's unbiased std
// Per row (ppo_advantage, ppo_value_pred, ppo_row):
//   a     = (adv - mean) / (std + 1e-8f) with normalisation, adv without
//   ratio = expf(logp - old);  s1 = ratio a;  s2 = clamp(ratio, 1 - c, 1 + c) a;  sur = s2 < s1 ? s2 : s1
//                                                      (sde_ppo_surrogate: usv_sde_math.hpp's ratio, clamp, products)
//   vp    = v without a value clip;  dv = v - old_v;  vp = old_v + clamp(dv, -cv, cv) with one (a NaN stays)
//   e     = ret - vp;  the row's five terms:  sur,  e e,  the entropy (-logp without an entropy tensor),
//           (ratio - 1) - (logp - old),  |ratio - 1| > c ? 1 : 0  (a NaN ratio counts 0, as torch's comparison)
// The finish (ppo_finish), from the five sums:
//   policy_loss = -(S(sur) / B);  value_loss = S(e e) / B;  entropy_loss = -(S(entropy) / B)
//   loss = (policy_loss + ent_coef entropy_loss) + vf_coef value_loss                          SB3's order
//   approx_kl = S(..) / B;  clip_fraction = S(..) / B      (the count is exact in f32 below 2^24 rows)
// Gradients at unit upstream of loss:
//   g_logp    = gl + (s1 <= s2 ? gs s1 : 0)      sde_eval_row_grad with gs = -1 / B and gl = ent_coef / B without an
//                                                entropy tensor (d entropy_loss / d logp = 1 / B), 0 with one
//   g_values  = ((2 vf_coef) (vp - ret)) / B     where -cv <= dv <= cv (bounds inclusive, torch.clamp's backward) or
//                                                there is no value clip; 0 beyond, and for a NaN dv
//   g_entropy = -ent_coef / B
// adv, old, old_v and ret are data.
//
// Explained variance of (values, returns), y = ret, r = ret - v, population variances in the same two-pass form
// (ppo_mean, ppo_sqdev, ppo_explained):
//   my = S(y) / B;  mr = S(r) / B;  vy = S((y - my)^2) / B;  vr = S((r - mr)^2) / B;  ev = 1 - vr / vy, NaN if vy == 0
#pragma once

#include "usv_sac_math.hpp"

namespace usv {

constexpr int kPpoSums = 5;                        // floats per partial
constexpr int kPpoOuts = 6;                        // loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction
constexpr int kPpoScratchMeans = 2;                // the explained variance keeps its two means in the head's padding
constexpr float kPpoAdvEps = 1e-8f;
enum PpoSum { kPpoSur = 0, kPpoSq, kPpoEnt, kPpoKl, kPpoClipped };

static_assert(kPpoScratchMeans + 2 <= kSacScratchHead, "the two means fit behind the ticket word");

USV_SAC_HD size_t ppo_scratch_floats(int64_t rows) {
  return (size_t)kSacScratchHead + (size_t)kPpoSums * (size_t)sac_partials(rows);
}

// A clip range: finite and >= 0.
USV_SAC_HD bool ppo_range_ok(float c) { return c >= 0.0f && c <= 3.402823466e+38f; }

// What a call computes besides its rows: the switches and the four scalars.
struct PpoForm {
  bool normalize;                                  // and B > 1: the caller's test
  bool vclip;                                      // a value clip: old values and clip_vf
  bool with_entropy;                               // an entropy tensor
  float clip, clip_vf, ent_coef, vf_coef;
};

USV_SAC_HD float ppo_mean(float sum, int64_t B) { return sac_mean(sum, B); }

// One term of a second pass.
USV_SAC_HD float ppo_sqdev(float x, float mean) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float d = x - mean;
  return d * d;
}

USV_SAC_HD float ppo_std(float sqsum, int64_t B) { return sqrtf(sqsum / (float)(B - 1)); }

USV_SAC_HD float ppo_explained(float sq_y, float sq_r, int64_t B) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float vy = sac_mean(sq_y, B), vr = sac_mean(sq_r, B);
  return vy == 0.0f ? NAN : 1.0f - vr / vy;
}

USV_SAC_HD float ppo_advantage(float adv, bool normalize, float mean, float std) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return normalize ? (adv - mean) / (std + kPpoAdvEps) : adv;
}

// values_pred of one row; pass: whether the gradient reaches v.
USV_SAC_HD float ppo_value_pred(float v, float old_v, bool vclip, float cv, bool& pass) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  pass = true;
  if (!vclip) return v;
  const float dv = v - old_v;
  pass = dv >= -cv && dv <= cv;
  const float t = dv < -cv ? -cv : dv;             // torch.clamp: a NaN stays
  return old_v + (t > cv ? cv : t);
}

USV_SAC_HD float ppo_entropy_grad(float ent_coef, int64_t B) { return -ent_coef / (float)B; }

// One row: its five terms and the unit gradients of logp and v.  a: ppo_advantage's; entropy: unused without a
// tensor.
USV_SAC_HD void ppo_row(const PpoForm& f, float logp, float old, float a, float v, float old_v, float ret,
                        float entropy, int64_t B, float (&t)[kPpoSums], float& g_logp, float& g_v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float ratio;
  t[kPpoSur] = sde_ppo_surrogate(logp, old, a, f.clip, ratio);
  bool pass;
  const float vp = ppo_value_pred(v, old_v, f.vclip, f.clip_vf, pass);
  const float e = ret - vp;
  t[kPpoSq] = e * e;
  t[kPpoEnt] = f.with_entropy ? entropy : -logp;
  const float r1 = ratio - 1.0f;
  t[kPpoKl] = r1 - (logp - old);
  t[kPpoClipped] = fabsf(r1) > f.clip ? 1.0f : 0.0f;
  const float gl = f.with_entropy ? 0.0f : f.ent_coef / (float)B;
  g_logp = sde_eval_row_grad(gl, -1.0f / (float)B, ratio, a, f.clip);
  g_v = pass ? ((2.0f * f.vf_coef) * (vp - ret)) / (float)B : 0.0f;
}

// The six outputs from the five sums.
USV_SAC_HD void ppo_finish(const float (&s)[kPpoSums], float ent_coef, float vf_coef, int64_t B, float (&out)[kPpoOuts]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float pl = sac_neg_mean(s[kPpoSur], B), vl = sac_mean(s[kPpoSq], B), el = sac_neg_mean(s[kPpoEnt], B);
  out[0] = (pl + ent_coef * el) + vf_coef * vl;
  out[1] = pl;
  out[2] = vl;
  out[3] = el;
  out[4] = sac_mean(s[kPpoKl], B);
  out[5] = sac_mean(s[kPpoClipped], B);
}

}  // namespace usv
