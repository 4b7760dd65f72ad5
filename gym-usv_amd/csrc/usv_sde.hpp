// usv_sde.hpp -- SB3's StateDependentNoiseDistribution at rollout time (common/distributions.py:
// sample_weights, get_noise, log_prob) in one launch: usv_sde_sample / usv_sde_weights (include/usv_hip.h).
// The arithmetic, the numbering of the matrix elements and the summation order are usv_sde_math.hpp's.
//
//   sde_sample_kernel<A>   a wave per env, a pass per 256 latents.  A lane takes four consecutive latents
//                          with one 16-B load, rebuilds its 4 A matrix elements from the A Philox blocks
//                          that cover exactly them (block (j / 4) * A + m holds elements 4 m .. 4 m + 3 of
//                          the lane's 4 A), and accumulates its terms of noise_k and var_k.  The 2 A lane
//                          sums are reduced by the DPP butterfly (= sde_tree_sum), and lane 0 does the
//                          tail and the stores.  The matrix never reaches memory.
//   sde_weights_kernel<A>  a lane per block of four elements: w[e][j][k], SB3's exploration_mat, for
//                          inspection, tests and checkpoints.
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

template <int A>
__global__ __launch_bounds__(kBlock) void sde_sample_kernel(SdeArgs a, const float* __restrict__ mean,
                                                           const float* __restrict__ lat, size_t stride,
                                                           const float* __restrict__ std, float* __restrict__ act,
                                                           float* __restrict__ act_env, float* __restrict__ logp) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int64_t e = (int64_t)blockIdx.x * kWaves + wave;
  if (e >= a.n) return;                                 // wave-uniform
  const uint64_t gid = a.gid0 + (uint64_t)e;
  const float* const row = lat + (size_t)e * stride;
  float noise[A], var[A];
#pragma unroll
  for (int k = 0; k < A; ++k) noise[k] = var[k] = 0.0f;
  for (int j0 = kSdePerLane * l; j0 < a.L; j0 += kSdePass) {
    const float4 lv = *reinterpret_cast<const float4*>(row + j0);     // row and stride are 16-B aligned
    const float x[4] = {lv.x, lv.y, lv.z, lv.w};
    float s[4 * A];
#pragma unroll
    for (int i = 0; i < 4 * A; ++i) s[i] = std[(size_t)j0 * A + i];
#pragma unroll
    for (int m = 0; m < A; ++m) {
      uint32_t o[4];
      float z[4];
      sde_block(a.seed, gid, a.epoch, (uint32_t)(j0 / 4) * A + m, o);
      sde_normals(o, z);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 4 * m + q;                        // element i of the lane's 4 A: latent i / A, action i % A
        sde_accum(x[i / A], s[i], sde_weight(s[i], z[q]), noise[i % A], var[i % A]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < A; ++k) {
    noise[k] = sde_wave_sum(noise[k]);
    var[k] = sde_wave_sum(var[k]);
  }
  if (l != 0) return;
  float lp = 0.0f;
#pragma unroll
  for (int k = 0; k < A; ++k) {
    const float m = mean[(size_t)e * A + k];
    const float ak = sde_action(m, noise[k]);
    act[(size_t)e * A + k] = ak;
    act_env[(size_t)e * A + k] = sde_clip(ak, a.low[k], a.high[k]);
    lp = lp + sde_logp_term(ak, m, var[k]);
  }
  logp[e] = lp;
}

// blocks_per_env = L * A / 4; thread t of the grid owns block t % blocks_per_env of env t / blocks_per_env.
template <int A>
__global__ __launch_bounds__(kBlock) void sde_weights_kernel(SdeArgs a, const float* __restrict__ std,
                                                            float* __restrict__ w) {
  const int bpe = a.L * A / 4;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= (int64_t)a.n * bpe) return;
  const int64_t e = t / bpe;
  const uint32_t b = (uint32_t)(t - e * bpe);
  uint32_t o[4];
  float z[4];
  sde_block(a.seed, a.gid0 + (uint64_t)e, a.epoch, b, o);
  sde_normals(o, z);
  float* const dst = w + (size_t)e * a.L * A + 4 * (size_t)b;
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[q] = sde_weight(std[4 * (size_t)b + q], z[q]);
}

}  // namespace usv
