// usv_norm.hpp -- SB3's VecNormalize between the step and the frame stack, i.e.
// VecFrameStack(VecNormalize(venv)): running mean / variance of the observations and running variance of
// the discounted return (RunningMeanStd), clipped normalised observations pushed into the ring of
// usv_wrap.hpp, clipped normalised rewards.  usv_wrap_step_norm / usv_wrap_reset_norm (include/usv_hip.h)
// run behind usv_step on the same stream.  The arithmetic and the work split are usv_norm_math.hpp's.
//
// A training step is three launches, stream-ordered (a row can only be normalised once every row has
// been reduced); with training off it is the third alone:
//   1. norm_moments_kernel   one block per chunk of envs: reads obs [N][D] once (a wave load is 64
//      consecutive floats of one row), rew and returns; writes returns = returns * gamma + rew and, per
//      column and for the returns, one partial (mean, M2) to the caller's scratch.  The four wave
//      partials of a column meet in LDS and combine in wave order.  No atomics.
//   2. norm_finalise_kernel  one 64-lane block per column (D obs columns + the returns): combines the
//      column's partials in block-index order (the fixed tree of usv_norm_math.hpp) and merges the batch
//      into mean / var.  Every column reads the same old count, so no block of this launch writes it.
//   3. wrap_step_norm_kernel wrap_step_body (usv_wrap.hpp: wrap_step_kernel's code, so the same work
//      split and ordering argument) under the WrapNorm policy: the transform in the push and in the
//      terminal row, norm_rew, returns = 0 for done envs; before it norm_stage: the tables and -- thread 0
//      of block 0 -- the two counts, which launch 2 could not bump.
// No block waits for another anywhere; the order between launches is the stream's.
//
// Tables.  A lane normalising four floats needs four (mean, inv_std) pairs, 64 B.  Each block stages the
// D pairs in LDS (interleaved, 16 D bytes: 2.3 KB at D = 143) and computes inv_std = 1 / sqrt(var + eps)
// while doing so: one ds_read_b128 per pair instead of 36 more global loads per lane next to its 9 data
// loads, and the published inv_std (written by block 0) is by construction what every block used.
// LDS holds D <= kNormMaxDim.
#pragma once

#include "usv_norm_math.hpp"
#include "usv_wrap.hpp"

namespace usv {

static_assert(kNormWaves == kWaves && kNormLanes == kWave, "usv_norm_math.hpp's split is this block's");
constexpr int kNormMaxDim = 4096;      // 16 D bytes of LDS <= 64 KB
constexpr int kNormFinalRun = kNormMaxPartials / kNormLanes;   // partials a finalising lane folds at most
static_assert(kNormFinalRun * kNormLanes == kNormMaxPartials, "norm_final_run: per <= kNormFinalRun");

struct NormArgs {
  int n, D;
  int upd_obs, upd_ret;         // training && norm_obs, training && norm_reward (this call updates them)
  int norm_rew;                 // norm_reward
  double clip_obs, clip_rew, gamma, eps;
  double* obs_mean;             // [D]
  double* obs_var;
  double* obs_inv;
  double* obs_count;            // [1]
  double* ret_mean;
  double* ret_var;
  double* ret_inv;
  double* ret_count;
  double* returns;              // [n]
  double* scratch;              // [2][P][D + 1]: partial means, then partial M2s
};

// rew may be null with upd_ret == 0 (a reset).
template <typename RW>
__global__ __launch_bounds__(kBlock) void norm_moments_kernel(NormArgs a, const float* obs, const RW* rew) {
  __shared__ NormMoments sh[kNormWaves][kNormLanes];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int b = blockIdx.x, P = gridDim.x, D = a.D, C = D + 1;
  const int64_t N = a.n;
  const int groups = norm_chunk_groups(N);
  double* const pmean = a.scratch + (size_t)b * C;
  double* const pm2 = a.scratch + ((size_t)P + b) * C;
  if (a.upd_obs) {
    for (int c0 = 0; c0 < D; c0 += kNormLanes) {
      const int c = c0 + l;
      const bool act = c < D;
      NormMoments acc{0.0, 0.0, 0.0};
      for (int gi = w; gi < groups; gi += kNormWaves) {
        const int nr = norm_group_rows(N, b, gi);
        if (nr <= 0) break;
        // a lane past the last column reads column D - 1 again and drops its result: every load is
        // unconditional, so the sixteen of a group are in flight together
        const float* const src = obs + (size_t)norm_group_begin(N, b, gi) * D + (act ? c : D - 1);
        NormMoments g{0.0, 0.0, 0.0};
        if (nr == kNormGroupRows) {                     // all but the batch's last group
          float x[kNormGroupRows];
#pragma unroll
          for (int i = 0; i < kNormGroupRows; ++i) x[i] = src[i * D];
#pragma unroll
          for (int i = 0; i < kNormGroupRows; ++i) norm_group_add(g, (double)x[i], i);
        } else {
          for (int i = 0; i < nr; ++i) norm_group_add(g, (double)src[i * D], i);
        }
        acc = norm_combine(acc, g);
      }
      sh[w][l] = acc;
      __syncthreads();
      if (w == 0 && act) {
        NormMoments t = sh[0][l];
        for (int v = 1; v < kNormWaves; ++v) t = norm_combine(t, sh[v][l]);
        pmean[c] = t.mean;
        pm2[c] = t.m2;
      }
      __syncthreads();
    }
  }
  if (a.upd_ret) {
    NormMoments acc{0.0, 0.0, 0.0};
    for (int gi = w; gi < groups; gi += kNormWaves) {
      const int nr = norm_group_rows(N, b, gi);
      if (nr <= 0) break;
      const int64_t r0 = norm_group_begin(N, b, gi);
      double ret = 0.0;
      if (l < nr) {
        ret = norm_discount(a.returns[r0 + l], a.gamma, (double)rew[r0 + l]);
        a.returns[r0 + l] = ret;
      }
      NormMoments g{0.0, 0.0, 0.0};
      if (nr == kNormGroupRows) {
#pragma unroll
        for (int i = 0; i < kNormGroupRows; ++i) norm_group_add(g, __shfl(ret, i), i);
      } else {
        for (int i = 0; i < nr; ++i) norm_group_add(g, __shfl(ret, i), i);
      }
      acc = norm_combine(acc, g);
    }
    if (l == 0) sh[w][0] = acc;
    __syncthreads();
    if (w == 0 && l == 0) {
      NormMoments t = sh[0][0];
      for (int v = 1; v < kNormWaves; ++v) t = norm_combine(t, sh[v][0]);
      pmean[D] = t.mean;
      pm2[D] = t.m2;
    }
  }
}

// Block c < D: obs column c; block D: the returns.  P partials per column.
__global__ __launch_bounds__(kNormLanes) void norm_finalise_kernel(NormArgs a, int P) {
  __shared__ NormMoments sh[kNormLanes];
  const int c = blockIdx.x, l = threadIdx.x, D = a.D, C = D + 1;
  const bool is_ret = c == D;
  if (is_ret ? !a.upd_ret : !a.upd_obs) return;         // the whole block
  const int64_t N = a.n;
  const double* const pmean = a.scratch + c;
  const double* const pm2 = a.scratch + (size_t)P * C + c;
  int p0, p1;
  norm_final_run(P, l, &p0, &p1);
  // the lane's run is at most kNormFinalRun partials: all loaded first (a past-the-run index reads the
  // last partial again and is not combined), then folded in increasing order
  double qm[kNormFinalRun], q2[kNormFinalRun];
#pragma unroll
  for (int i = 0; i < kNormFinalRun; ++i) {
    const int p = min(p0 + i, P - 1);
    qm[i] = pmean[(size_t)p * C];
    q2[i] = pm2[(size_t)p * C];
  }
  NormMoments m{0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < kNormFinalRun; ++i) {
    const int p = p0 + i;
    if (p < p1) m = norm_combine(m, NormMoments{(double)(norm_chunk_end(N, p) - norm_chunk_begin(N, p)), qm[i], q2[i]});
  }
  sh[l] = m;
  __syncthreads();
  for (int s = 1; s < kNormLanes; s <<= 1) {
    if ((l & (2 * s - 1)) == 0) sh[l] = norm_combine(sh[l], sh[l + s]);
    __syncthreads();
  }
  if (l == 0) {
    double* const mean = is_ret ? a.ret_mean : a.obs_mean + c;
    double* const var = is_ret ? a.ret_var : a.obs_var + c;
    double mu = *mean, v = *var;
    norm_merge(mu, v, is_ret ? *a.ret_count : *a.obs_count, sh[0]);
    *mean = mu;
    *var = v;
  }
}

// The (mean, inv_std) pairs of the obs columns into LDS, the published reciprocals and the counts
// (block 0); returns the reward's inv_std.  Every thread of the block calls it (it has a barrier).
template <bool NORM_OBS>
__device__ __forceinline__ double norm_stage(const NormArgs& z, double* tab) {
  const int D = z.D;
  if (NORM_OBS) {
    for (int c = threadIdx.x; c < D; c += kBlock) {
      tab[2 * c] = z.obs_mean[c];
      tab[2 * c + 1] = norm_inv_std(z.obs_var[c], z.eps);
    }
    __syncthreads();
  }
  const double rinv = norm_inv_std(*z.ret_var, z.eps);
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < D; c += kBlock) z.obs_inv[c] = norm_inv_std(z.obs_var[c], z.eps);
    if (threadIdx.x == 0) {
      *z.ret_inv = rinv;
      if (z.upd_obs) *z.obs_count = norm_count_after(*z.obs_count, (double)z.n);
      if (z.upd_ret) *z.ret_count = norm_count_after(*z.ret_count, (double)z.n);
    }
  }
  return rinv;
}

// The wrappers' normalisation policy (usv_wrap.hpp).  NORM_OBS: every frame float is normalised on its
// way (column c of a piece: pairs c .. c + 3 of tab); the reward's switch is z.norm_rew.  norm_rew: the
// step's normalised-reward output (null in a reset).
template <bool NORM_OBS>
struct WrapNorm {
  const NormArgs& z;
  const double* tab;
  double rinv;
  float* norm_rew;
  template <typename RW>
  __device__ __forceinline__ void reward(int e, RW rw) const {
    norm_rew[e] = z.norm_rew ? norm_apply((double)rw, 0.0, rinv, z.clip_rew) : (float)rw;
  }
  __device__ __forceinline__ void restart(int e) const { z.returns[e] = 0.0; }
  __device__ __forceinline__ float one(float v, int c) const {
    return NORM_OBS ? norm_apply((double)v, tab[2 * c], tab[2 * c + 1], z.clip_obs) : v;
  }
  __device__ __forceinline__ WrapQuad4 quad(WrapQuad4 v, int c) const {
    if (!NORM_OBS) return v;
    const double* const t = tab + 2 * c;
    WrapQuad4 o;
    o.x = norm_apply((double)v.x, t[0], t[1], z.clip_obs);
    o.y = norm_apply((double)v.y, t[2], t[3], z.clip_obs);
    o.z = norm_apply((double)v.z, t[4], t[5], z.clip_obs);
    o.w = norm_apply((double)v.w, t[6], t[7], z.clip_obs);
    return o;
  }
};

template <typename RW, bool NORM_OBS>
__global__ __launch_bounds__(kBlock) void wrap_step_norm_kernel(WrapArgs a, NormArgs z, const float* obs, const RW* rew,
                                                               const uint8_t* done, const float* final_obs,
                                                               float* final_stack, float* norm_rew) {
  extern __shared__ double norm_tab[];
  const double rinv = norm_stage<NORM_OBS>(z, norm_tab);
  wrap_step_body(a, obs, rew, done, final_obs, final_stack, WrapNorm<NORM_OBS>{z, norm_tab, rinv, norm_rew});
}

template <bool MASKED, bool NORM_OBS>
__global__ __launch_bounds__(kBlock) void wrap_reset_norm_kernel(WrapArgs a, NormArgs z, const uint8_t* mask,
                                                                const float* obs) {
  extern __shared__ double norm_tab[];
  const double rinv = norm_stage<NORM_OBS>(z, norm_tab);
  wrap_reset_body<MASKED>(a, mask, obs, WrapNorm<NORM_OBS>{z, norm_tab, rinv, nullptr});
}

}  // namespace usv
