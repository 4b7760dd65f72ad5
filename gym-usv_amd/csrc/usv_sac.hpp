// usv_sac.hpp -- the fused SAC update as HIP kernels (include/usv_hip.h: usv_sac_critic_loss / _policy_loss /
// _loss_backward): SB3's SAC.train lines for the TD target, the twin-critic loss, the actor and
// entropy-coefficient losses with their gradients at unit upstream.  The arithmetic and the summation order are
// usv_sac_math.hpp's.  (polyak_update over a list of tensors is usv_optim.hpp's, next to the element loop it shares.)
//
// The reduction that these kernels, caps_loss_kernel (usv_caps.hpp), optim_sqsum_kernel (usv_optim.hpp) and the
// ppo kernels (usv_ppo.hpp, five floats per partial) share has two forms and no other: sac_for_rows, a thread's rows of its partial, and sac_finish, from the strands' sums to the
// one thread that holds the totals.
//
//   sac_critic_kernel, sac_policy_kernel
//       A block of 256 threads per partial of P = 1024 rows.  Thread t takes rows t, t + 256, t + 512, t + 768 of its
//       partial (sac_for_rows): every row stream is read with coalesced 4-B loads, the per-row outputs are written
//       the same way, and the thread's terms are its strand.  sac_finish: the strands are reduced by the DPP
//       butterfly (sde_wave_sum) and the four wave sums through LDS.  One partial: thread 0 has the sums.  More:
//       thread 0 stores the block's sums to the caller's scratch and draws a ticket; the block that draws the last
//       one adds all partials in ascending order (sac_combine_at).  No block waits for another.  The thread that
//       sac_finish names writes the loss.
//   sac_scale_kernel   the backward of either loss: the saved unit gradients times the upstream scalars, read on
//                      the device; a null upstream writes zeros.
#pragma once

#include "usv_sac_math.hpp"

namespace usv {

static_assert(kSacStrands == kBlock && kSacWaves == kWaves, "usv_sac_math.hpp's strands are this block's threads");

// The hand-off of the partials to the block that arrives last, called by every thread of a block that has more
// than one partial; s: the block's sums.  The scratch is [ticket, 3 pad][partials][3].  True in thread 0 of the last
// block alone, with the totals.  The counter form of the agent-scope release / acquire hand-off: thread 0's stores,
// every wave's vmcnt(0), the barrier, that lane's release fence and its own wait, a relaxed agent-scope ticket; the
// last arriver's wave 0 acquires once, and its own later plain loads then see every block's partial: a lane per
// partial, added in ascending order through readlane.  The ticket word is zero when the caller allocates the
// scratch, and the last arriver puts it back.  The block's partial is at `slot` of `partials`, `stride` floats per
// partial; the tickets may come from several stream-ordered launches that share the scratch (usv_optim.hpp).
// sac_finish is its only caller.
template <int NS>
__device__ __forceinline__ bool sac_combine_at(const float (&s)[NS], size_t slot, int partials, int stride,
                                               float* scratch, float (&total)[NS]) {
  unsigned* const ticket = reinterpret_cast<unsigned*>(scratch);
  float* const part = scratch + kSacScratchHead;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) part[slot * stride + k] = s[k];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x >= kWave) return false;
  unsigned drawn = 0;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  drawn = (unsigned)__builtin_amdgcn_readfirstlane((int)drawn);
  if (drawn != (unsigned)(partials - 1)) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int k = 0; k < NS; ++k) total[k] = 0.0f;
  for (int p0 = 0; p0 < partials; p0 += kWave) {
    const int p = p0 + (int)threadIdx.x;
    float v[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = p < partials ? part[(size_t)p * stride + k] : 0.0f;
    const int count = partials - p0 < kWave ? partials - p0 : kWave;
    for (int l = 0; l < count; ++l) {
#pragma unroll
      for (int k = 0; k < NS; ++k) total[k] = total[k] + bcast(v[k], l);
    }
  }
  if (threadIdx.x != 0) return false;
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// The block's sums of NS strands each: wave sums by the butterfly, the four of them through LDS.
template <int NS>
__device__ __forceinline__ void sac_block_sums(float (&s)[NS], float (&red)[NS][kSacWaves]) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const float w = sde_wave_sum(s[k]);
    if (lane == 0) red[k][wave] = w;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = sac_waves_sum(red[k]);
}

// The finish of a reduction, called by every thread of the block with its strand's sums s: the block's sums and,
// with more than one partial, the hand-off (the block's partial goes to `slot`).  True in the one thread of the grid
// that holds the totals, left in s.
template <int NS>
__device__ __forceinline__ bool sac_finish(float (&s)[NS], size_t slot, int partials, int stride, float* scratch) {
  __shared__ float red[NS][kSacWaves];
  sac_block_sums(s, red);
  if (partials > 1) {
    float total[NS];
    if (!sac_combine_at(s, slot, partials, stride, scratch, total)) return false;
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = total[k];
  }
  return threadIdx.x == 0;
}

// The row loop: row(i) for the thread's rows i < rows of the block's partial, strand t's rows t, t + 256, t + 512,
// t + 768 of it.
template <class F>
__device__ __forceinline__ void sac_for_rows(int rows, F&& row) {
  const int64_t base = (int64_t)blockIdx.x * kSacPartialRows;
#pragma unroll
  for (int j = 0; j < kSacStrandRows; ++j) {
    const int64_t i = base + threadIdx.x + j * kSacStrands;
    if (i < rows) row(i);
  }
}

struct SacCriticArgs {
  int rows;
  const float *q1, *q2, *q1t, *q2t, *rew, *done, *ent, *logp_next, *disc;
  float gamma;
  float *tgt, *loss, *g_q1, *g_q2, *scratch;
};

__global__ __launch_bounds__(kBlock) void sac_critic_kernel(SacCriticArgs a) {
  const bool with_ent = a.ent != nullptr;
  const float ent = with_ent ? a.ent[0] : 0.0f;
  float s[2] = {0.0f, 0.0f};
  sac_for_rows(a.rows, [&](int64_t i) {
    const float tgt = sac_target(a.q1t[i], a.q2t[i], with_ent, ent, with_ent ? a.logp_next[i] : 0.0f, a.rew[i],
                                 a.done[i], a.disc ? a.disc[i] : a.gamma);
    float t1, t2, g1, g2;
    sac_critic_row(a.q1[i], a.q2[i], tgt, a.rows, t1, t2, g1, g2);
    a.tgt[i] = tgt;
    if (a.g_q1) a.g_q1[i] = g1;
    if (a.g_q2) a.g_q2[i] = g2;
    s[0] = s[0] + t1;
    s[1] = s[1] + t2;
  });
  if (sac_finish(s, blockIdx.x, (int)gridDim.x, kSacScratchSums, a.scratch)) a.loss[0] = sac_critic_loss(s[0], s[1], a.rows);
}

struct SacPolicyArgs {
  int rows;
  const float *logp, *q1, *q2, *ent, *log_ent;
  float te;
  float *actor_loss, *ent_loss, *g_logp, *g_q1, *g_q2, *g_log_ent, *scratch;
};

__global__ __launch_bounds__(kBlock) void sac_policy_kernel(SacPolicyArgs a) {
  const float ent = a.ent[0];
  const bool with_le = a.log_ent != nullptr;
  const float le = with_le ? a.log_ent[0] : 0.0f;
  const float g_logp = sac_mean(ent, a.rows);
  float s[3] = {0.0f, 0.0f, 0.0f};
  sac_for_rows(a.rows, [&](int64_t i) {
    float ta, tl, tg, g1, g2;
    sac_policy_row(a.logp[i], a.q1[i], a.q2[i], ent, le, a.te, a.rows, ta, tl, tg, g1, g2);
    if (a.g_logp) a.g_logp[i] = g_logp;
    if (a.g_q1) a.g_q1[i] = g1;
    if (a.g_q2) a.g_q2[i] = g2;
    s[0] = s[0] + ta;
    s[1] = s[1] + tl;
    s[2] = s[2] + tg;
  });
  if (sac_finish(s, blockIdx.x, (int)gridDim.x, kSacScratchSums, a.scratch)) {
    a.actor_loss[0] = sac_mean(s[0], a.rows);
    if (with_le) {
      a.ent_loss[0] = sac_neg_mean(s[1], a.rows);
      if (a.g_log_ent) a.g_log_ent[0] = sac_neg_mean(s[2], a.rows);
    }
  }
}

struct SacScaleArgs {
  int rows;
  const float* up;                                   // the upstream of the row gradients, a device scalar or null
  const float* g[3];
  float* o[3];
  const float *up_s, *gs;                            // one more scalar gradient with its own upstream
  float* os;
};

__global__ __launch_bounds__(kBlock) void sac_scale_kernel(SacScaleArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const float up = a.up ? a.up[0] : 0.0f;
  if (i < a.rows) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (a.o[k]) a.o[k][i] = a.up ? a.g[k][i] * up : 0.0f;
  }
  if (i == 0 && a.os) a.os[0] = a.up_s ? a.gs[0] * a.up_s[0] : 0.0f;
}

}  // namespace usv
