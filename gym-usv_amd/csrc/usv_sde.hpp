// usv_sde.hpp -- SB3's StateDependentNoiseDistribution (common/distributions.py: sample_weights, get_noise,
// log_prob) as HIP kernels: the rollout's sample, SAC's squashed head and PPO's evaluate_actions (include/usv_hip.h:
// usv_sde_sample / _weights / _squash_forward / _squash_backward / _eval_forward / _eval_backward).
// The arithmetic, the numbering of the matrix elements and the summation order are usv_sde_math.hpp's.
//
// One row loop, sde_row_sums<A, Noise>, serves the three forwards: a wave per row, a pass per 256 latents.  A lane
// takes four consecutive latents with one 16-B load and reads its 4 A std values; with Noise it rebuilds its 4 A
// matrix elements from the A Philox blocks that cover exactly them (block (j / 4) * A + m holds elements 4 m ..
// 4 m + 3 of the lane's 4 A) and accumulates its terms of noise_k and var_k, without it those of var_k alone.  The
// lane sums are reduced by the DPP butterfly (= sde_tree_sum).  The matrix never reaches memory.
//   sde_sample_kernel<A>, sde_squash_forward_kernel<A>, sde_eval_forward_kernel<A>
//                          wave and row set-up, sde_row_sums, lane 0's tail and stores.  The first two share noise_k
//                          and var_k, the third var_k, because they run the same code.
// The two backwards state their body each (pass-outer, row-inner; they differ in the row tail and in whether the
// normals are rebuilt): as one body templated on a row-tail policy, sde_squash_backward_kernel<2> compiled to 627
// instructions for 613 with four of its 32 accumulation fmas left scalar, and the squashed update at 65 536 x 256
// measured 2.0 % and 2.3 % above the parent's slowest process in two jobs (profiles/sde_refactor_ab.json,
// "shared_backward_body"); the eval kernel's code was the same either way.
//   sde_squash_backward_kernel<A>, sde_eval_backward_kernel<A>, sde_std_finalise_kernel (adds the partials)
//   sde_weights_kernel<A>  a lane per block of four elements: w[e][j][k], SB3's exploration_mat, for
//                          inspection, tests and checkpoints.
//   sde_sample_dev_kernel<A>, sde_squash_forward_dev_kernel<A>, sde_squash_backward_dev_kernel<A>,
//   sde_weights_dev_kernel<A>
//                          the four that draw noise, with the epoch read from a word in device memory instead of
//                          the arguments (usv_sde_*_dev): the same text (usv_sde_noise.inc), a scalar load per wave
//                          in front.
// The [L][A] std table is read once per wave, straight into registers: each element is used by one lane
// of the wave, once, so staging it in LDS would add a write, a barrier and a read without saving a load;
// the table (2 KiB at L = 256, A = 2) stays in L2 for the waves of the other envs.
// A lane whose four latents lie at or past L loads nothing (L % 4 == 0: a lane's four are in or out
// together) and contributes +0.0f; a wave whose env is at or past n returns before its first load.
#pragma once

#include "usv_sde_math.hpp"

namespace usv {

static_assert(kSdeLanes == kWave && kSdePerLane == 4, "usv_sde_math.hpp's lane split is this wave's");

struct SdeArgs {
  int n, L;
  uint32_t epoch;
  uint64_t seed, gid0;
  float low[2], high[2];
};

// sde_tree_sum over the wave's lanes, result wave-uniform.
__device__ __forceinline__ float sde_wave_sum(float v) {
  v = v + dpp<kDppXor1>(v);
  v = v + dpp<kDppXor2>(v);
  v = v + dpp<kDppHalfMirror>(v);
  v = v + dpp<kDppMirror>(v);
  return (bcast(v, 0) + bcast(v, 16)) + (bcast(v, 32) + bcast(v, 48));
}

// The row loop: lane l's passes over one row and the wave sums, wave-uniform.  Noise: noise_k and var_k with the
// normals of (seed, gid, epoch); without it var_k alone (noise stays +0.0f, the key is not read, nothing is reduced
// for it).
template <int A, bool Noise>
__device__ __forceinline__ void sde_row_sums(int L, int l, const float* __restrict__ row, const float* __restrict__ std,
                                             uint64_t seed, uint64_t gid, uint32_t epoch, float (&noise)[A],
                                             float (&var)[A]) {
#pragma unroll
  for (int k = 0; k < A; ++k) noise[k] = var[k] = 0.0f;
  for (int j0 = kSdePerLane * l; j0 < L; j0 += kSdePass) {
    const float4 lv = *reinterpret_cast<const float4*>(row + j0);     // row and stride are 16-B aligned
    const float x[4] = {lv.x, lv.y, lv.z, lv.w};
    float s[4 * A];
#pragma unroll
    for (int i = 0; i < 4 * A; ++i) s[i] = std[(size_t)j0 * A + i];
    if constexpr (Noise) {
#pragma unroll
      for (int m = 0; m < A; ++m) {
        uint32_t o[4];
        float z[4];
        sde_block(seed, gid, epoch, (uint32_t)(j0 / 4) * A + m, o);
        sde_normals(o, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = 4 * m + q;                      // element i of the lane's 4 A: latent i / A, action i % A
          sde_accum(x[i / A], s[i], sde_weight(s[i], z[q]), noise[i % A], var[i % A]);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4 * A; ++i) sde_var_accum(x[i / A], s[i], var[i % A]);
    }
  }
#pragma unroll
  for (int k = 0; k < A; ++k) {
    if constexpr (Noise) noise[k] = sde_wave_sum(noise[k]);
    var[k] = sde_wave_sum(var[k]);
  }
}

// The epoch of a _dev kernel: the word in device memory, read once by each wave (a scalar load: the address is
// wave-uniform and nothing in the kernel writes it).
__device__ __forceinline__ uint32_t sde_epoch_word(const uint32_t* __restrict__ epoch_dev) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)epoch_dev[0]);
}

// sde_sample_kernel<A>, sde_squash_forward_kernel<A>, sde_squash_backward_kernel<A>, sde_weights_kernel<A>: the epoch
// is SdeArgs's.
#define USV_NOISE_KERNEL(name) name##_kernel
#define USV_NOISE_EPOCH_PARAM
#define USV_NOISE_PROLOGUE
#include "usv_sde_noise.inc"
#undef USV_NOISE_KERNEL
#undef USV_NOISE_EPOCH_PARAM
#undef USV_NOISE_PROLOGUE

// ... and their _dev_kernel forms (usv_sde_*_dev): the epoch is the word epoch_dev points to.
#define USV_NOISE_KERNEL(name) name##_dev_kernel
#define USV_NOISE_EPOCH_PARAM const uint32_t* __restrict__ epoch_dev,
#define USV_NOISE_PROLOGUE a.epoch = sde_epoch_word(epoch_dev);
#include "usv_sde_noise.inc"
#undef USV_NOISE_KERNEL
#undef USV_NOISE_EPOCH_PARAM
#undef USV_NOISE_PROLOGUE

// PPO's evaluate_actions, forward: stored actions under the current policy, no noise.  Lane 0's tail: logp, and
// with old / adv the ratio and the clipped surrogate.  var_out (the backward's saved var) is NULL on a call that
// will not be differentiated; old, adv, sur and ratio are NULL together.
template <int A>
__global__ __launch_bounds__(kBlock) void sde_eval_forward_kernel(
    int n, int L, const float* __restrict__ mean, const float* __restrict__ lat, size_t stride,
    const float* __restrict__ std, const float* __restrict__ act, const float* __restrict__ old,
    const float* __restrict__ adv, float clip, float* __restrict__ logp, float* __restrict__ sur,
    float* __restrict__ ratio, float* __restrict__ var_out) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int64_t e = (int64_t)blockIdx.x * kWaves + wave;
  if (e >= n) return;                                   // wave-uniform
  float noise[A], var[A];
  sde_row_sums<A, false>(L, l, lat + (size_t)e * stride, std, 0, 0, 0, noise, var);
  if (l != 0) return;
  float lp = 0.0f;
#pragma unroll
  for (int k = 0; k < A; ++k) {
    const size_t at = (size_t)e * A + k;
    if (var_out) var_out[at] = var[k];
    lp = lp + sde_logp_term(act[at], mean[at], var[k]);
  }
  logp[e] = lp;
  if (old) {
    float r;
    sur[e] = sde_ppo_surrogate(lp, old[e], adv[e], clip, r);
    ratio[e] = r;
  }
}

// The backward: sde_squash_backward_kernel's shape without the normals.  A wave owns partial p of g_std, rows
// [p R, min(n, (p + 1) R)); pass-outer, row-inner, the 4 A std values and g_std accumulators of a lane's elements in
// registers.  The row tail (t, g_mean, gv: a few divisions, wave-uniform) is recomputed in every pass and lane 0
// stores g_mean in its first.  ratio and adv are NULL together (no surrogate: t = gl); g_logp and g_sur may each be
// NULL (zeros); g_lat is NULL where the latent needs no gradient, and then nothing of size [n][L] is written.
template <int A>
__global__ __launch_bounds__(kBlock) void sde_eval_backward_kernel(
    int n, int L, int R, const float* __restrict__ mean, const float* __restrict__ lat, size_t stride,
    const float* __restrict__ std, const float* __restrict__ act, const float* __restrict__ var,
    const float* __restrict__ ratio, const float* __restrict__ adv, float clip, const float* __restrict__ g_logp,
    const float* __restrict__ g_sur, float* __restrict__ g_mean, float* __restrict__ g_lat, size_t g_stride,
    float* __restrict__ part) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int64_t p = (int64_t)blockIdx.x * kWaves + wave;
  const int64_t e0 = p * R;
  if (e0 >= n) return;                                  // wave-uniform
  const int64_t e1 = e0 + R < n ? e0 + R : n;
  for (int j0 = kSdePerLane * l; j0 < L; j0 += kSdePass) {
    float s[4 * A], gs[4 * A];
#pragma unroll
    for (int i = 0; i < 4 * A; ++i) {
      s[i] = std[(size_t)j0 * A + i];
      gs[i] = 0.0f;
    }
    for (int64_t e = e0; e < e1; ++e) {
      const float gl = g_logp ? g_logp[e] : 0.0f;
      const float t = ratio ? sde_eval_row_grad(gl, g_sur ? g_sur[e] : 0.0f, ratio[e], adv[e], clip) : gl;
      float gv[A];
#pragma unroll
      for (int k = 0; k < A; ++k) {
        const size_t at = (size_t)e * A + k;
        float G;
        sde_eval_grad_tail(act[at], mean[at], var[at], t, G, gv[k]);
        if (j0 == 0) g_mean[at] = G;                    // lane 0, first pass
      }
      const float4 lv = *reinterpret_cast<const float4*>(lat + (size_t)e * stride + j0);
      const float x[4] = {lv.x, lv.y, lv.z, lv.w};
      float gx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int i = 0; i < 4 * A; ++i) sde_eval_grad_accum(x[i / A], s[i], gv[i % A], gx[i / A], gs[i]);
      if (g_lat)
        *reinterpret_cast<float4*>(g_lat + (size_t)e * g_stride + j0) = make_float4(gx[0], gx[1], gx[2], gx[3]);
    }
    float* const dst = part + ((size_t)p * L + j0) * A;       // 16-B aligned: scratch is, and (p L + j0) A % 4 == 0
#pragma unroll
    for (int m = 0; m < A; ++m)
      *reinterpret_cast<float4*>(dst + 4 * m) = make_float4(gs[4 * m], gs[4 * m + 1], gs[4 * m + 2], gs[4 * m + 3]);
  }
}

// g_std [L][A] from the P partials (sde_partials_sum's order).  A block takes 16 elements: wave w, lane
// 16 sl + ie is strand 4 w + sl of element ie; the strands of a wave meet by two lane exchanges, the waves in LDS.
static_assert(kSdeStrands == 4 * kWaves, "sde_std_finalise_kernel's strands are 4 per wave");
__global__ __launch_bounds__(kBlock) void sde_std_finalise_kernel(int P, int LA, const float* __restrict__ part,
                                                                 float* __restrict__ g_std) {
  __shared__ float sums[kWaves][16];
  const int w = threadIdx.x / kWave, l = lane_id();
  const int ie = l % 16, sl = l / 16;
  const int i = blockIdx.x * 16 + ie;
  float acc = 0.0f;
  if (i < LA)
    for (int p = 4 * w + sl; p < P; p += kSdeStrands) acc = acc + part[(size_t)p * LA + i];
  acc = acc + __shfl_xor(acc, 16);
  acc = acc + __shfl_xor(acc, 32);
  if (sl == 0) sums[w][ie] = acc;
  __syncthreads();
  if (threadIdx.x < 16 && i < LA) g_std[i] = (sums[0][ie] + sums[1][ie]) + (sums[2][ie] + sums[3][ie]);
}

}  // namespace usv
