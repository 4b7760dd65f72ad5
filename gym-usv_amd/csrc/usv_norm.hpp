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
//   3. wrap_step_norm_kernel wrap_step_kernel's work (usv_wrap.hpp: same work split, same ordering
//      argument, rows 4-B aligned only) with the transform in the push and in the terminal row; also
//      norm_rew, returns = 0 for done envs, and -- thread 0 of block 0 -- the two counts, which launch 2
//      could not bump.
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

// wrap_push with every float normalised on its way (column c of a piece: pairs c .. c + 3 of tab).
__device__ __forceinline__ void wrap_push_norm(const WrapArgs& a, const double* tab, double clip, const float* src,
                                               int e0, int ne, int l) {
  const int D = a.D;
  float* const dst = a.ring + (size_t)e0 * a.stride + (size_t)a.p * D;
  const ptrdiff_t mir = a.m >= 0 ? (ptrdiff_t)(a.m - a.p) * D : 0;
  const float* const span = src + (size_t)e0 * D;
  if (D >= 4) {
    const int P = (D + 3) / 4, np = ne * P;
    const int dk = kWave / P, dr = kWave % P;
    int k = l / P, r = l - k * P;
    for (int q = l; q < np; q += 3 * kWave) {
      const float* sp[3];
      float* dp[3];
      int cc[3];
      WrapQuad4 v[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int c = min(4 * r, D - 4);
        cc[i] = c;
        sp[i] = span + k * D + c;
        dp[i] = dst + (size_t)k * a.stride + c;
        k += dk;
        r += dr;
        if (r >= P) { r -= P; ++k; }
      }
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (q + i * kWave < np) v[i] = *reinterpret_cast<const WrapQuad*>(sp[i]);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (q + i * kWave < np) {
          const double* const t = tab + 2 * cc[i];
          WrapQuad4 o;
          o.x = norm_apply((double)v[i].x, t[0], t[1], clip);
          o.y = norm_apply((double)v[i].y, t[2], t[3], clip);
          o.z = norm_apply((double)v[i].z, t[4], t[5], clip);
          o.w = norm_apply((double)v[i].w, t[6], t[7], clip);
          *reinterpret_cast<WrapQuad*>(dp[i]) = o;
          if (a.m >= 0) *reinterpret_cast<WrapQuad*>(dp[i] + mir) = o;
        }
    }
  } else {
    const int nd = ne * D;
    for (int q = l; q < nd; q += kWave) {
      const int k = q / D, c = q - k * D;
      const float v = norm_apply((double)span[q], tab[2 * c], tab[2 * c + 1], clip);
      float* const d = dst + (size_t)k * a.stride + c;
      d[0] = v;
      if (a.m >= 0) d[mir] = v;
    }
  }
}

// wrap_step_kernel with the normalisation (NORM_OBS: of the frames; the reward's by z.norm_rew).
template <typename RW, bool NORM_OBS>
__global__ __launch_bounds__(kBlock) void wrap_step_norm_kernel(WrapArgs a, NormArgs z, const float* obs, const RW* rew,
                                                               const uint8_t* done, const float* final_obs,
                                                               float* final_stack, float* norm_rew) {
  extern __shared__ double norm_tab[];
  const double rinv = norm_stage<NORM_OBS>(z, norm_tab);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int e0 = (blockIdx.x * kWaves + wave) * kWrapEnvs;
  const int ne = min(kWrapEnvs, a.n - e0);
  if (ne <= 0) return;
  // ---- stats (the raw reward: the Monitor sits inside VecNormalize), the normalised reward
  bool dn = false;
  if (l < ne) {
    const int e = e0 + l;
    const RW rw = rew[e];
    double ret = a.ep_ret[e] + (double)rw;
    int len = a.ep_len[e] + 1;
    dn = done[e] != 0;
    norm_rew[e] = z.norm_rew ? norm_apply((double)rw, 0.0, rinv, z.clip_rew) : (float)rw;
    if (dn) {
      if (a.episode) {
        a.episode[2 * (size_t)e] = ret;
        a.episode[2 * (size_t)e + 1] = (double)len;
      }
      if (a.cum_ret) {
        a.cum_ret[e] += ret;
        a.cum_len[e] += len;
        a.cum_eps[e] += 1;
      }
      ret = 0.0;
      len = 0;
      z.returns[e] = 0.0;
    }
    a.ep_ret[e] = ret;
    a.ep_len[e] = len;
  }
  // ---- rare: done envs (terminal stack with the normalised final obs last, then the clear)
  unsigned long long dm = ballot(dn);
  if (__builtin_expect(dm != 0ull, 0)) {
    const int D = a.D, older = (a.k - 1) * D;
    for (; dm; dm &= dm - 1) {
      const int e = e0 + __builtin_ctzll(dm);
      float* const row = a.ring + (size_t)e * a.stride;
      if (final_stack) {
        float* const f = final_stack + (size_t)e * a.k * D;
        const float* const t = row + (size_t)a.term * D;
        for (int c = l; c < older; c += kWave) f[c] = t[c];
        const float* const fo = final_obs + (size_t)e * D;
        for (int c = l; c < D; c += kWave)
          f[older + c] = NORM_OBS ? norm_apply((double)fo[c], norm_tab[2 * c], norm_tab[2 * c + 1], z.clip_obs) : fo[c];
        // the loads of the row have returned before the first zero below is issued
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      if (a.keep_sign) wrap_clear_row<true>(row, a, l); else wrap_clear_row<false>(row, a, l);
    }
  }
  // ---- push
  if (NORM_OBS) wrap_push_norm(a, norm_tab, z.clip_obs, obs, e0, ne, l);
  else wrap_push(a, obs, e0, ne, l);
}

// wrap_reset_kernel with returns = 0 for the restarted envs and the normalised push.
template <bool MASKED, bool NORM_OBS>
__global__ __launch_bounds__(kBlock) void wrap_reset_norm_kernel(WrapArgs a, NormArgs z, const uint8_t* mask,
                                                                const float* obs) {
  extern __shared__ double norm_tab[];
  norm_stage<NORM_OBS>(z, norm_tab);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int e0 = (blockIdx.x * kWaves + wave) * kWrapEnvs;
  const int ne = min(kWrapEnvs, a.n - e0);
  if (ne <= 0) return;
  bool on = false;
  if (l < ne) {
    on = !MASKED || mask[e0 + l] != 0;
    if (on) {
      a.ep_ret[e0 + l] = 0.0;
      a.ep_len[e0 + l] = 0;
      z.returns[e0 + l] = 0.0;
    }
  }
  const unsigned long long rm = ballot(on);
  if (rm == 0ull) return;
  for (unsigned long long b = rm; b; b &= b - 1)
    wrap_clear_row<false>(a.ring + (size_t)(e0 + __builtin_ctzll(b)) * a.stride, a, l);
  const bool all = rm == (ne == 64 ? ~0ull : (1ull << ne) - 1);
  for (unsigned long long b = all ? 1ull : rm; b; b &= b - 1) {
    const int f = all ? 0 : __builtin_ctzll(b), cnt = all ? ne : 1;   // every env of the wave, or one row at a time
    if (NORM_OBS) wrap_push_norm(a, norm_tab, z.clip_obs, obs, e0 + f, cnt, l);
    else wrap_push(a, obs, e0 + f, cnt, l);
  }
}

}  // namespace usv
