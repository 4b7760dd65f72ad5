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

// One term of a lane's two accumulations.
USV_SDE_HD void sde_accum(float lat, float std, float w, float& noise, float& var) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float l2 = lat * lat, s2 = std * std;
  noise = fmaf(lat, w, noise);
  var = fmaf(l2, s2, var);
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

}  // namespace usv
