// usv_sde_math.hpp -- the arithmetic of the fused gSDE action head (usv_sde.hpp): SB3's
// StateDependentNoiseDistribution (common/distributions.py: sample_weights, get_noise, log_prob) with the
// exploration matrix rebuilt from a counter-based generator in the step that uses it.  Plain C++ marked
// __host__ __device__, no HIP types: the kernels and a stand-alone host program (tests/test_sde_math.py)
// run the same functions in the same order.
//
// The matrix.  Element (j, k) of env e's [L][A] matrix (j the latent index, k the action index) has flat
// index i = j * A + k and is normal number i % 4 of Philox4x32-10 block b = i / 4 with
//   key     = (seed lo, seed hi)                the caller's 64-bit seed, unmodified
//   counter = (gid lo, gid hi, epoch, b)        gid = gid0 + e, the global env id; epoch the noise epoch
// (the multipliers and Weyl constants of Philox::block, usv_device.hpp).  A block's words (o0, o1, o2, o3)
// give four normals by two Box-Muller pairs:
//   u1 = ((o0 >> 8) + 1) * 2^-24  in (0, 1],   u2 = (o1 >> 8) * 2^-24  in [0, 1),   r = sqrt(-2 ln u1),
//   z0 = r cos(2 pi u2),  z1 = r sin(2 pi u2);   (o2, o3) give z2, z3 the same way.
// The numbering does not depend on how a kernel splits the work, and not on how envs are sharded.
//
// The head, all f32, every operation rounded on its own but the two accumulations, which are one fused
// multiply-add per term (explicit fmaf: contraction is off in every function here):
//   w_jk    = std_jk * z_jk
//   noise_k = sum_j lat_j * w_jk                 acc = fmaf(lat_j, w_jk, acc)
//   var_k   = sum_j (lat_j lat_j) (std_jk std_jk) acc = fmaf(lat_j * lat_j, std_jk * std_jk, acc)
//   a_k     = mean_k + noise_k                   the unclipped action (the rollout buffer's)
//   a_env_k = max(min(a_k, high_k), low_k)       a NaN action stays NaN, as torch.max(torch.min()) keeps it
//   s2_k    = var_k + 1e-6;  d_k = a_k - mean_k  (from the rounded a_k, as torch's log_prob(a) sees it)
//   logp    = sum_k ((-(d_k d_k) / (2 s2_k) - 0.5 ln s2_k) - 0.5 ln 2 pi),  k ascending from 0.0f
//
// Summation order over j.  Latent j belongs to lane (j / 4) % 64 of 64: a lane takes four consecutive
// latents of every 256 (sde_lane).  A lane accumulates its terms from +0.0f in ascending j; the 64 lane sums
// (+0.0f for a lane without latents) are added by a balanced binary tree over the lanes in lane order
// (sde_tree_sum: neighbours first).  Float addition is commutative, so a butterfly in which every lane adds
// its partner's value computes exactly this tree.
//
// The squashed, differentiable head (usv_sde_squash_forward / _backward: SAC's distribution, squash_output).
// noise_k and var_k as above, then per action, every operation rounded on its own:
//   u_k   = mean_k + noise_k                     the gaussian action (sde_action: bit-equal to the head above)
//   a_k   = tanhf(u_k)
//   t_k   = expf(-2 |u_k|);  q_k = 1 + t_k;  om_k = (4 t_k) / (q_k q_k)      1 - tanh^2 without a subtraction
//   c_k   = om_k + 1e-6
//   env_k = low_k + ((a_k + 1) * 0.5) * (high_k - low_k)
//   logp  = sum_k (sde_logp_term(u_k, mean_k, var_k) - ln c_k),  k ascending from 0.0f
// Two deviations from SB3: the log-probability is taken at u itself (SB3 goes through atanh(clamp(tanh(u))),
// which only adds rounding), and 1 - tanh^2 is the exp form (1 - a a loses all its digits once a rounds to 1).
// Backward, for upstream ga_k = dl/da_k and gl = dl/dlogp (sde_squash_grad_tail, wave-uniform per row):
//   G_k  = ga_k om_k + gl (((2 a_k) om_k) / c_k)         = g_mean_k
//   gn_k = G_k - (gl d_k) / s2_k                          the gradient of noise_k;  d_k = u_k - mean_k
//   gv_k = gl ((d_k d_k) / ((2 s2_k) s2_k) - 0.5 / s2_k)  the gradient of var_k
// and per matrix element (sde_grad_accum), two fused multiply-adds into each sum, in this order:
//   g_lat_j  = fmaf(gn_k, std_jk z_jk, .) then fmaf(gv_k, (2 lat_j)(std_jk std_jk), .)    k ascending from +0.0f
//   g_std_jk = fmaf(gn_k lat_j, z_jk, .)  then fmaf(gv_k, (2 (lat_j lat_j)) std_jk, .)    rows ascending
// The sum over rows of g_std.  R = ceil(n / 1024) rows per partial, P = ceil(n / R) <= 1024 partials; partial p
// adds rows [p R, min(n, (p + 1) R)) in ascending order from +0.0f.  The P partials of an element are added by
// 16 strands, strand s taking p = s, s + 16, .. in ascending order from +0.0f, and the 16 strand sums by a
// balanced binary tree in strand order, neighbours first (sde_partials_sum).
//
// The evaluation head (usv_sde_eval_forward / _backward: PPO's evaluate_actions, no noise).  For stored actions
// act_k, var_k as above (sde_var_accum, the variance line of sde_accum: sample's terms, lanes and tree), then
//   logp  = sum_k sde_logp_term(act_k, mean_k, var_k),  k ascending from 0.0f
// and, where old, adv and the clip range c are given (sde_ppo_surrogate),
//   ratio = expf(logp - old);  rc = min(max(ratio, 1 - c), 1 + c);  s1 = ratio adv;  s2 = rc adv
//   sur   = s2 < s1 ? s2 : s1
// Backward, for upstream gl (of logp) and gs (of sur), from the saved var and ratio:
//   t       = gl + (s1 <= s2 ? gs s1 : 0)                  torch.min / clamp under autograd, ties included
//   s2v_k   = var_k + 1e-6;  d_k = act_k - mean_k
//   g_mean_k = (t d_k) / s2v_k
//   gv_k    = t ((d_k d_k) / ((2 s2v_k) s2v_k) - 0.5 / s2v_k)
//   g_lat_j  = fmaf(gv_k, (2 lat_j)(std_jk std_jk), .)     k ascending from +0.0f
//   g_std_jk = fmaf(gv_k, (2 (lat_j lat_j)) std_jk, .)     rows ascending, partials and their sum as above
// (sde_eval_grad_accum alone).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__CUDACC__)
#define USV_SDE_HD __host__ __device__ inline
#else
#define USV_SDE_HD inline
#endif

namespace usv {

constexpr int kSdeLanes = 64;                      // partial sums per env = the lanes of a wave
constexpr int kSdePerLane = 4;                     // consecutive latents of a lane: one 16-B load
constexpr int kSdePass = kSdeLanes * kSdePerLane;  // latents per pass
constexpr int kSdeMaxLatent = 4096;
constexpr float kSdeEps = 1e-6f;                   // StateDependentNoiseDistribution.epsilon
constexpr float kSdeHalfLn2Pi = 0.91893853320467274178f;

USV_SDE_HD bool sde_latent_ok(int64_t L) { return L >= 4 && L <= kSdeMaxLatent && L % 4 == 0; }
USV_SDE_HD int sde_lane(int j) { return (j / kSdePerLane) % kSdeLanes; }
// the block and the normal within it of element (j, k) of an [L][A] matrix
USV_SDE_HD uint32_t sde_block_of(int j, int k, int A) { return (uint32_t)(j * A + k) / 4u; }
USV_SDE_HD int sde_slot_of(int j, int k, int A) { return (j * A + k) % 4; }

// Philox4x32-10 (Salmon et al., SC'11).
USV_SDE_HD void sde_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                           uint32_t (&o)[4]) {
  uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3, a = k0, b = k1;
  // Two rounds per trip, pinned: the sample kernel measured 6 % slower with one (same registers) and 1 % faster
  // fully unrolled for 10 more VGPRs and 18 more SGPRs (profiles/sde_ab_builds.json).
#if defined(__clang__)
#pragma unroll 2
#endif
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * x0, p1 = (uint64_t)0xCD9E8D57u * x2;
    const uint32_t lo0 = (uint32_t)p0, hi0 = (uint32_t)(p0 >> 32), lo1 = (uint32_t)p1, hi1 = (uint32_t)(p1 >> 32);
    x0 = hi1 ^ x1 ^ a; x1 = lo1; x2 = hi0 ^ x3 ^ b; x3 = lo0;
    a += 0x9E3779B9u; b += 0xBB67AE85u;
  }
  o[0] = x0; o[1] = x1; o[2] = x2; o[3] = x3;
}
// block b of global env gid in noise epoch `epoch`
USV_SDE_HD void sde_block(uint64_t seed, uint64_t gid, uint32_t epoch, uint32_t b, uint32_t (&o)[4]) {
  sde_philox((uint32_t)gid, (uint32_t)(gid >> 32), epoch, b, (uint32_t)seed, (uint32_t)(seed >> 32), o);
}

// Both are exact in f32: a 24-bit integer (2^24 itself for u1 = 1) times a power of two.
USV_SDE_HD float sde_u1(uint32_t o) { return (float)((o >> 8) + 1u) * 5.9604644775390625e-8f; }
USV_SDE_HD float sde_u2(uint32_t o) { return (float)(o >> 8) * 5.9604644775390625e-8f; }

// One Box-Muller pair.  Device: the hardware's log2, square root and its turn-based sine and cosine,
// which take u2 itself (v_sin_f32 / v_cos_f32 compute sin / cos of 2 pi x): the product 2 pi u2 is never
// formed, so it is never rounded, and u2 in [0, 1) is well inside their +-256-turn domain.  Host: libm.
USV_SDE_HD void sde_box_muller(float u1, float u2, float& zc, float& zs) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIP_DEVICE_COMPILE__)
  const float ln = __builtin_amdgcn_logf(u1) * 0.69314718055994530942f;
  const float r = __builtin_amdgcn_sqrtf(-2.0f * ln);
  zc = r * __builtin_amdgcn_cosf(u2);
  zs = r * __builtin_amdgcn_sinf(u2);
#else
  const float r = sqrtf(-2.0f * logf(u1));
  const float t = 6.28318530717958647692f * u2;
  zc = r * cosf(t);
  zs = r * sinf(t);
#endif
}
// the four normals of a block's words
USV_SDE_HD void sde_normals(const uint32_t (&o)[4], float (&z)[4]) {
  sde_box_muller(sde_u1(o[0]), sde_u2(o[1]), z[0], z[1]);
  sde_box_muller(sde_u1(o[2]), sde_u2(o[3]), z[2], z[3]);
}

USV_SDE_HD float sde_weight(float std, float z) { return std * z; }

// One term of a lane's variance sum.
USV_SDE_HD void sde_var_accum(float lat, float std, float& var) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float l2 = lat * lat, s2 = std * std;
  var = fmaf(l2, s2, var);
}

// One term of a lane's two accumulations.
USV_SDE_HD void sde_accum(float lat, float std, float w, float& noise, float& var) {
  noise = fmaf(lat, w, noise);
  sde_var_accum(lat, std, var);
}

// The 64 lane sums by the balanced tree; p is overwritten.
USV_SDE_HD float sde_tree_sum(float (&p)[kSdeLanes]) {
  for (int s = 1; s < kSdeLanes; s *= 2)
    for (int i = 0; i < kSdeLanes; i += 2 * s) p[i] = p[i] + p[i + s];
  return p[0];
}

USV_SDE_HD float sde_clip(float a, float low, float high) {
  const float t = high < a ? high : a;             // torch.min(a, high): NaN stays
  return t < low ? low : t;                        // torch.max(., low)
}

// a_k from the reduced sums.
USV_SDE_HD float sde_action(float mean, float noise) { return mean + noise; }

// One action's term of the log-probability, Normal(mean, sqrt(var + eps)).log_prob(a).
USV_SDE_HD float sde_logp_term(float a, float mean, float var) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float s2 = var + kSdeEps;
  const float d = a - mean;
  const float q = d * d;
  const float den = 2.0f * s2;
  const float t = q / den;
  const float lg = 0.5f * logf(s2);
  return (-t - lg) - kSdeHalfLn2Pi;
}

// ---- the squashed head
constexpr int kSdeMaxPartials = 1024;              // partial sums of g_std over rows
constexpr int kSdeStrands = 16;                    // strands that add the partials of one element

USV_SDE_HD int64_t sde_rows_per_partial(int64_t n) { return (n + kSdeMaxPartials - 1) / kSdeMaxPartials; }
USV_SDE_HD int64_t sde_partials(int64_t n) {
  const int64_t R = sde_rows_per_partial(n);
  return R > 0 ? (n + R - 1) / R : 0;
}

// a = tanh(u) and om = 1 - tanh(u)^2 = 4 t / (1 + t)^2 with t = exp(-2 |u|): no subtraction, no overflow.
USV_SDE_HD void sde_squash(float u, float& a, float& om) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  a = tanhf(u);
  const float t = expf(-2.0f * fabsf(u));
  const float q = 1.0f + t;
  om = (4.0f * t) / (q * q);
}

// SB3's unscale_action: [-1, 1] to the Box.
USV_SDE_HD float sde_unscale(float a, float low, float high) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return low + ((a + 1.0f) * 0.5f) * (high - low);
}

// One action's term of the squashed log-probability: the Gaussian term at u minus ln(1 - tanh^2 + eps).
USV_SDE_HD float sde_squash_logp_term(float u, float mean, float var, float om) {
  return sde_logp_term(u, mean, var) - logf(om + kSdeEps);
}

// The gradient of var_k for the row's upstream t of logp: t ((d d) / ((2 s2) s2) - 0.5 / s2).
USV_SDE_HD float sde_var_grad(float t, float d, float s2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return t * ((d * d) / ((2.0f * s2) * s2) - 0.5f / s2);
}

// One action's row gradients from the saved u and var: G (= g_mean), gn (of noise_k), gv (of var_k).
USV_SDE_HD void sde_squash_grad_tail(float u, float mean, float var, float ga, float gl, float& G, float& gn,
                                     float& gv) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float a, om;
  sde_squash(u, a, om);
  const float c = om + kSdeEps;
  const float s2 = var + kSdeEps;
  const float d = u - mean;
  const float lg = ((2.0f * a) * om) / c;
  G = ga * om + gl * lg;
  gn = G - (gl * d) / s2;
  gv = sde_var_grad(gl, d, s2);
}

// One matrix element's terms of g_lat_j and g_std_jk through the variance alone (the evaluation head's).
USV_SDE_HD void sde_eval_grad_accum(float lat, float std, float gv, float& g_lat, float& g_std) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float vl = (2.0f * lat) * (std * std);
  const float vs = (2.0f * (lat * lat)) * std;
  g_lat = fmaf(gv, vl, g_lat);
  g_std = fmaf(gv, vs, g_std);
}

// One matrix element's terms of g_lat_j and g_std_jk through the noise and the variance.  Its variance terms are
// sde_eval_grad_accum's, written out here: composed of a noise half and that function, the same arithmetic reaches
// the vectoriser in another order and sde_squash_backward_kernel<2> compiles to 614 instructions for 613, and the
// squashed update at 65 536 x 256 measured 0.5 % above the parent's slowest process (profiles/sde_refactor_ab.json,
// "composed_grad_accum").
USV_SDE_HD void sde_grad_accum(float lat, float std, float z, float gn, float gv, float& g_lat, float& g_std) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float w = sde_weight(std, z);
  const float vl = (2.0f * lat) * (std * std);
  const float nl = gn * lat;
  const float vs = (2.0f * (lat * lat)) * std;
  g_lat = fmaf(gn, w, g_lat);
  g_lat = fmaf(gv, vl, g_lat);
  g_std = fmaf(nl, z, g_std);
  g_std = fmaf(gv, vs, g_std);
}

// The P partials of one element (part[p * stride]) by strands and tree.
USV_SDE_HD float sde_partials_sum(const float* part, size_t stride, int P) {
  float s[kSdeStrands];
  for (int t = 0; t < kSdeStrands; ++t) {
    float acc = 0.0f;
    for (int p = t; p < P; p += kSdeStrands) acc = acc + part[(size_t)p * stride];
    s[t] = acc;
  }
  for (int h = 1; h < kSdeStrands; h *= 2)
    for (int i = 0; i < kSdeStrands; i += 2 * h) s[i] = s[i] + s[i + h];
  return s[0];
}

// ---- the evaluation head (PPO's evaluate_actions, usv_sde_eval_forward / _backward)
// torch.clamp(ratio, 1 - c, 1 + c): a NaN ratio stays NaN.
USV_SDE_HD float sde_ppo_clamp(float ratio, float clip) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float lo = 1.0f - clip, hi = 1.0f + clip;
  const float t = ratio < lo ? lo : ratio;
  return t > hi ? hi : t;
}

// The two products of PPO's surrogate from the ratio: s1 = ratio adv, s2 = clamp(ratio) adv.
USV_SDE_HD void sde_ppo_products(float ratio, float adv, float clip, float& s1, float& s2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  s1 = ratio * adv;
  s2 = sde_ppo_clamp(ratio, clip) * adv;
}

// ratio = exp(logp - old) and the clipped surrogate min(s1, s2) of one row.
USV_SDE_HD float sde_ppo_surrogate(float logp, float old, float adv, float clip, float& ratio) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  ratio = expf(logp - old);
  float s1, s2;
  sde_ppo_products(ratio, adv, clip, s1, s2);
  return s2 < s1 ? s2 : s1;
}

// The gradient of a row's logp for upstream gl (of logp) and gs (of the surrogate): torch.min and clamp under
// autograd.  s1 is chosen where s1 <= s2 and d s1 / d logp = s1; an unclipped row ties (s1 == s2), min halves the
// gradient between the two and clamp passes its half (bounds inclusive), which add to gs s1; a clipped row that
// ties has adv = 0 = s1.
USV_SDE_HD float sde_eval_row_grad(float gl, float gs, float ratio, float adv, float clip) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float s1, s2;
  sde_ppo_products(ratio, adv, clip, s1, s2);
  return gl + (s1 <= s2 ? gs * s1 : 0.0f);
}

// One action's gradients from the row's t (sde_eval_row_grad): g_mean_k and gv (of var_k).
USV_SDE_HD void sde_eval_grad_tail(float act, float mean, float var, float t, float& g_mean, float& gv) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float s2 = var + kSdeEps;
  const float d = act - mean;
  g_mean = (t * d) / s2;
  gv = sde_var_grad(t, d, s2);
}

}  // namespace usv
