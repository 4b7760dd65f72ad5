// usv_rollout.hpp -- SB3's RolloutBuffer (common/buffers.py: add, compute_returns_and_advantage) and the
// truncation bootstrap of OnPolicyAlgorithm.collect_rollouts behind the fused wrappers, stream-ordered and
// without a host sync: usv_rollout_put_obs / _put_step / _gae (include/usv_hip.h).  The arithmetic and
// the slot numbering are usv_rollout_math.hpp's.
//
//   rollout_obs_kernel    row t of obs / act / val / logp (rollout_put_rows).  A wave owns kWrapEnvs = 16
//                         envs; their obs rows are copy_rows's (usv_row_copy.hpp) from a strided source,
//                         plain stores.
//   rollout_count_kernel  one block per chunk of envs: counts[b] = the chunk's bootstrapping envs.
//   rollout_step_kernel   one block per chunk: rew[t], start[t + 1], term_slot[t] and the rare W-float row
//                         copy into term_obs, by the whole wave.  Every block sums the <= 1024 chunk counts
//                         of the launch before it for its prefix; a wave ballot and the block's four wave
//                         counts (LDS) rank an env within its chunk.  The running total of the steps
//                         before t is read from totals[t & 1] and the new one written to totals[(t + 1) & 1]
//                         by block 0: no word is read and written in one launch.
//   rollout_gae_kernel    one lane per env, t = T - 1 .. 0; the loads of kRoGaeAhead steps are issued
//                         before their dependent chain runs.
// No atomics and no block waiting on another: the order between the count and the step is the stream's.
// Every output word has one writer and every sum is of integers, so a launch is bitwise reproducible.
#pragma once

#include "usv_rollout_math.hpp"
#include "usv_row_copy.hpp"

namespace usv {

static_assert(kRoBlock == kBlock, "usv_rollout_math.hpp's chunk pass is this block");

struct RoArgs {
  int n, T, W, A, cap;
  float* obs;
  float* act;
  float* rew;
  float* val;
  float* logp;
  float* adv;
  float* ret;
  uint8_t* start;               // [T + 1][n]
  int32_t* term_slot;           // [T][n]
  float* term_obs;              // [cap][W]
  int32_t* term_count;          // (stored, overflow)
  long long* totals;            // scratch: [2] running pair totals, then int32 counts[chunks]
  int32_t* counts;
};

// Row t of val / logp / act, and W floats of each env's src row (stride sstride) into dst + e * dstride:
// what the two put_obs kernels do for a wave.
__device__ __forceinline__ void rollout_put_rows(const RoArgs& a, int t, const float* src, size_t sstride, float* dst,
                                                 size_t dstride, int W, const float* act, const float* val,
                                                 const float* logp) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int e0 = (blockIdx.x * kWaves + wave) * kWrapEnvs;
  const int ne = min(kWrapEnvs, a.n - e0);
  if (ne <= 0) return;
  const size_t row0 = (size_t)t * a.n + e0;             // first of the wave's rows in a [T][n] buffer
  if (l < ne) {
    a.val[row0 + l] = val[e0 + l];
    a.logp[row0 + l] = logp[e0 + l];
  }
  for (int q = l; q < ne * a.A; q += kWave) a.act[row0 * a.A + q] = act[(size_t)e0 * a.A + q];
  copy_rows(src + (size_t)e0 * sstride, sstride, dst + (size_t)e0 * dstride, dstride, false, 0, W, ne, l,
            RowCopyPlain{});
}

__global__ __launch_bounds__(kBlock) void rollout_obs_kernel(RoArgs a, int t, const float* src, size_t sstride,
                                                            const float* act, const float* val, const float* logp) {
  rollout_put_rows(a, t, src, sstride, a.obs + (size_t)t * a.n * a.W, (size_t)a.W, a.W, act, val, logp);
}

__global__ __launch_bounds__(kBlock) void rollout_count_kernel(RoArgs a, const uint8_t* term, const uint8_t* trunc) {
  __shared__ int sh[kWaves];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int R = ro_chunk_envs(a.n);
  const int64_t e0 = (int64_t)blockIdx.x * R;
  int cnt = 0;                                          // wave-uniform
  for (int i = 0; i < R && e0 + i < a.n; i += kBlock) {
    const int64_t e = e0 + i + threadIdx.x;
    cnt += __builtin_popcountll(ballot(e < a.n && ro_bootstraps(term[e], trunc[e])));
  }
  if (lane_id() == 0) sh[w] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int v = 0; v < kWaves; ++v) c += sh[v];
    a.counts[blockIdx.x] = c;
  }
}

template <typename RW>
__global__ __launch_bounds__(kBlock) void rollout_step_kernel(RoArgs a, int t, const RW* rew, const uint8_t* term,
                                                             const uint8_t* trunc, const float* final_stack) {
  __shared__ long long sh_sum[2][kWaves];
  __shared__ int sh_cnt[kWaves];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int b = blockIdx.x, P = gridDim.x;
  // ---- pairs of this step in the chunks before this one, and in all of them
  long long before = 0, total = 0;
  for (int p = threadIdx.x; p < P; p += kBlock) {
    const int c = a.counts[p];
    total += c;
    before += p < b ? c : 0;
  }
  for (int s = kWave / 2; s; s >>= 1) {
    before += __shfl_xor(before, s);
    total += __shfl_xor(total, s);
  }
  if (l == 0) {
    sh_sum[0][w] = before;
    sh_sum[1][w] = total;
  }
  __syncthreads();
  before = total = 0;
  for (int v = 0; v < kWaves; ++v) {
    before += sh_sum[0][v];
    total += sh_sum[1][v];
  }
  const long long base = t == 0 ? 0 : a.totals[t & 1];
  if (b == 0 && threadIdx.x == 0) {
    a.totals[(t + 1) & 1] = base + total;
    a.term_count[0] = ro_stored(base + total, a.cap);
    a.term_count[1] = ro_overflow(base + total, a.cap);
  }
  // ---- the chunk, 256 envs per pass
  const int R = ro_chunk_envs(a.n), W = a.W;
  const int64_t e0 = (int64_t)b * R;
  const size_t row = (size_t)t * a.n;
  int run = 0;                                          // pairs of the chunk's earlier passes
  for (int i = 0; i < R && e0 + i < a.n; i += kBlock) { // block-uniform trip count
    const int64_t e = e0 + i + threadIdx.x;
    const bool in = e < a.n;
    bool bs = false;
    if (in) {
      const uint8_t tm = term[e], tr = trunc[e];
      bs = ro_bootstraps(tm, tr);
      a.rew[row + e] = (float)rew[e];
      a.start[row + a.n + e] = (tm | tr) != 0;
    }
    const unsigned long long bm = ballot(bs);
    if (l == 0) sh_cnt[w] = __builtin_popcountll(bm);
    __syncthreads();
    int wb = 0, all = 0;
    for (int v = 0; v < kWaves; ++v) {
      const int c = sh_cnt[v];
      all += c;
      wb += v < w ? c : 0;
    }
    __syncthreads();                                    // sh_cnt is rewritten by the next pass
    const int rank = run + wb + __builtin_popcountll(bm & ((1ull << l) - 1));
    const int32_t slot = bs ? ro_slot(base, before, rank, a.cap) : -1;
    if (in) a.term_slot[row + e] = slot;
    // rare: the terminal rows, one env at a time by the whole wave
    for (unsigned long long m = ballot(slot >= 0); m; m &= m - 1) {
      const int j = __builtin_ctzll(m);
      const int s = __shfl(slot, j);
      const float* const f = final_stack + (size_t)(e0 + i + w * kWave + j) * W;
      float* const d = a.term_obs + (size_t)s * W;
      for (int c = l; c < W; c += kWave) d[c] = f[c];
    }
    run += all;
  }
}

__global__ __launch_bounds__(kBlock) void rollout_gae_kernel(RoArgs a, const float* last_val, const float* term_val,
                                                            float g32, float gl32) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= a.n) return;
  const size_t n = a.n;
  float nv = last_val[e], gae = 0.0f;
  for (int t0 = a.T; t0 > 0; t0 -= kRoGaeAhead) {       // steps t0 - 1 .. t0 - kRoGaeAhead
    float r[kRoGaeAhead], v[kRoGaeAhead];
    uint8_t sn[kRoGaeAhead];
    int32_t ts[kRoGaeAhead];
#pragma unroll
    for (int i = 0; i < kRoGaeAhead; ++i) {             // a step before 0 reads step 0 again and is dropped
      const size_t at = (size_t)max(t0 - 1 - i, 0) * n + e;
      r[i] = a.rew[at];
      v[i] = a.val[at];
      sn[i] = a.start[at + n];
      ts[i] = a.term_slot[at];
    }
#pragma unroll
    for (int i = 0; i < kRoGaeAhead; ++i) {
      const int t = t0 - 1 - i;
      if (t < 0) break;
      float rr = r[i];
      if ((uint32_t)ts[i] < (uint32_t)a.cap) rr = ro_bootstrap(rr, g32, term_val[ts[i]]);
      const float ret = ro_gae_step(rr, v[i], nv, sn[i], g32, gl32, gae);
      a.adv[(size_t)t * n + e] = gae;
      a.ret[(size_t)t * n + e] = ret;
      nv = v[i];
    }
  }
  a.start[e] = a.start[(size_t)a.T * n + e];            // row T of this rollout is row 0 of the next
}

}  // namespace usv
