// usv_optim_math.hpp -- the arithmetic of the fused optimizer step (usv_optim.hpp): torch.nn.utils.clip_grad_norm_
// followed by torch.optim.Adam.step() (torch 2.x, amsgrad=False, weight_decay=0, maximize=False, the non-capturable
// path) over a list of tensors.  Plain C++ marked __host__ __device__, no HIP types: the kernels and a stand-alone
// host program (tests/test_optim_math.py) run the same functions in the same order.  All f32, every operation
// rounded on its own (contraction is off in every function here).
//
// Scalars (adam_scalars), in double from the step count t >= 1 and each cast once to f32:
//   bc1 = 1 - beta1^t;  step_size = lr / bc1;  bc2_sqrt = sqrt(1 - beta2^t);  1 - beta1, beta2, 1 - beta2, eps
// Clip, only with a max_norm (adam_clip_coef):
//   total = sqrtf(S)   S the sum of g g over every element of every tensor, below
//   coef  = min(1, max_norm / (total + 1e-6))      a NaN stays; an inf element gives coef = 0 and 0 inf = NaN there
//   g'    = g coef     always multiplied, as clip_grad_norm_ does when coef == 1; without a max_norm g' = g
// Per element (adam_value):
//   m' = m + (g' - m) (1 - beta1)
//   v' = v beta2 + ((1 - beta2) g') g'
//   p' = p - step_size (m' / (sqrtf(v') / bc2_sqrt + eps))
// The gradient is read and never written back: SB3 discards it at the next zero_grad.
//
// The sum S.  Each tensor is cut into chunks of kOptimChunk = C = 4096 elements (optim_chunks).  Within a chunk the
// elements form groups of four consecutive ones, 4 q .. 4 q + 3; strand s of kOptimStrands = 256 takes the groups
// s, s + 256, s + 512, s + 768 and adds the squares of their elements that exist in ascending element order from
// +0.0f (optim_strand_sqsum).  A group is one 16-B access where the tensor is 16-B aligned and four 4-B accesses
// where it is not: the assignment is the same either way.  Strands 64 w .. 64 w + 63 are added by sde_tree_sum
// (usv_sde_math.hpp) into wave sum w and the chunk's sum is (w0 + w1) + (w2 + w3) (sac_waves_sum).  The chunk sums
// are added in ascending order from +0.0f, tensors in list order and chunks in order within a tensor
// (optim_total_norm): a function of the list's numels alone, not of a grid, of which block ends last, of how the
// list is split over launches or of an alignment.
//
// State.  m and v live in two flat buffers; each tensor's segment is padded to a multiple of four floats
// (optim_state_floats), so a segment's offset follows from the numels before it and is 16-B aligned.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "usv_sac_math.hpp"

namespace usv {

constexpr int kOptimChunk = kPolyakChunk;          // C
constexpr int kOptimStrands = kSacStrands;         // strands of a chunk = threads of a block
constexpr int kOptimGroup = 4;                     // consecutive elements of a group: one 16-B access
constexpr int kOptimStrandGroups = kOptimChunk / (kOptimGroup * kOptimStrands);
constexpr int kOptimScratchHead = kSacScratchHead; // floats in front of the chunk sums: the ticket word, padded
constexpr float kOptimClipEps = 1e-6f;             // clip_grad_norm_'s
static_assert(kOptimStrandGroups * kOptimGroup * kOptimStrands == kOptimChunk, "a chunk is whole groups per strand");

USV_SAC_HD int64_t optim_chunks(int64_t numel) { return (numel + kOptimChunk - 1) / kOptimChunk; }
USV_SAC_HD int64_t optim_state_floats(int64_t numel) { return (numel + 3) / 4 * 4; }
USV_SAC_HD size_t optim_scratch_floats(int64_t chunks) { return (size_t)kOptimScratchHead + (size_t)chunks; }

struct AdamScalars {
  float om_b1, b2, om_b2, eps, step_size, bc2_sqrt;
};

// lr and eps finite and >= 0, the betas in [0, 1), t >= 1.
USV_SAC_HD bool adam_rate_ok(double x) { return x >= 0.0 && x <= 1.79769313486231570815e308; }
USV_SAC_HD bool adam_beta_ok(double b) { return b >= 0.0 && b < 1.0; }

inline AdamScalars adam_scalars(int64_t t, double lr, double beta1, double beta2, double eps) {
  const double bc1 = 1.0 - pow(beta1, (double)t);
  const double bc2 = 1.0 - pow(beta2, (double)t);
  AdamScalars s;
  s.om_b1 = (float)(1.0 - beta1);
  s.b2 = (float)beta2;
  s.om_b2 = (float)(1.0 - beta2);
  s.eps = (float)eps;
  s.step_size = (float)(lr / bc1);
  s.bc2_sqrt = (float)sqrt(bc2);
  return s;
}

// The clock block of usv_adam_step_dev: the step number and lr in device memory, and the two scalars that depend on
// them, derived on the device once per step (adam_clock_scalars) before any element is updated.  16-B aligned.
struct alignas(16) AdamClock {
  double lr;
  int64_t step;                                      // the number of the last step taken; 0 before the first
  float step_size, bc2_sqrt;                         // of that step
  uint32_t reserved[2];
};
static_assert(sizeof(AdamClock) == 32, "the clock block's layout (gym_usv_amd/optim.py reads it)");

// adam_scalars's two step-dependent scalars where the device derives them: the same doubles, each cast once.  The
// device's pow is another library than the host's: a pow off in its last place moves a cast by at most one f32 ulp.
USV_SAC_HD void adam_clock_scalars(int64_t t, double lr, double beta1, double beta2, float& step_size, float& bc2_sqrt) {
  const double bc1 = 1.0 - pow(beta1, (double)t);
  const double bc2 = 1.0 - pow(beta2, (double)t);
  step_size = (float)(lr / bc1);
  bc2_sqrt = (float)sqrt(bc2);
}

// A noise epoch moved on by inc: a uint32 that wraps, as the host's `epoch` does.
USV_SAC_HD uint32_t counter_added(uint32_t word, uint32_t inc) { return word + inc; }

USV_SAC_HD float optim_norm(float sqsum) { return sqrtf(sqsum); }

USV_SAC_HD float adam_clip_coef(float total, float max_norm) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float c = max_norm / (total + kOptimClipEps);
  return c > 1.0f ? 1.0f : c;                        // a NaN stays
}

USV_SAC_HD float adam_clipped(float g, float coef) { return g * coef; }

// One element; g is g'.
USV_SAC_HD void adam_value(float& p, float& m, float& v, float g, const AdamScalars& s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  m = m + (g - m) * s.om_b1;
  v = v * s.b2 + (s.om_b2 * g) * g;
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = p - s.step_size * (m / denom);
}

// acc + g g, the square rounded before the addition.
USV_SAC_HD float optim_sq_add(float acc, float g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float t = g * g;
  return acc + t;
}

// Strand s of a chunk of `count` <= C elements.
USV_SAC_HD float optim_strand_sqsum(const float* g, int count, int s) {
  float acc = 0.0f;
  for (int j = 0; j < kOptimStrandGroups; ++j) {
    const int at = kOptimGroup * (s + j * kOptimStrands);
    for (int k = 0; k < kOptimGroup; ++k)
      if (at + k < count) acc = optim_sq_add(acc, g[at + k]);
  }
  return acc;
}

// One chunk: strands, the tree over each wave's strands, the four wave sums.
inline float optim_chunk_sqsum(const float* g, int count) {
  float w[kSacWaves];
  for (int v = 0; v < kSacWaves; ++v) {
    float s[kSdeLanes];
    for (int l = 0; l < kSdeLanes; ++l) s[l] = optim_strand_sqsum(g, count, v * kSdeLanes + l);
    w[v] = sde_tree_sum(s);
  }
  return sac_waves_sum(w);
}

// acc + the chunk sums of one tensor in order; the list's total is this over its tensors from +0.0f.
inline float optim_tensor_sqsum(float acc, const float* g, int64_t numel) {
  for (int64_t at = 0; at < numel; at += kOptimChunk)
    acc = acc + optim_chunk_sqsum(g + at, numel - at < kOptimChunk ? (int)(numel - at) : kOptimChunk);
  return acc;
}

}  // namespace usv
