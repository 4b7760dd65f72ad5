// usv_wrap.hpp -- the reference's two training wrappers behind the step, as one launch each:
// VecFrameStack(5) (train_test/sb3_train_vec.py:70; SB3 StackedObservations, channels-last) and
// RecordEpisodeStatistics (:43) / the Monitor of make_vec_env (:67).  usv_wrap_step runs after usv_step
// on the same stream and reads what it wrote (obs, reward, done mask, final obs); nothing is copied to
// the host.
//
// The stack is the mirrored ring of usv_wrap_layout.hpp: a step writes the new frame to its one or two
// slots and moves nothing else, and the stacked observation is a column window of the ring.
//
// Work split.  64-thread groups of a 256-thread block are waves; each wave owns kWrapEnvs = 16
// consecutive envs and shares nothing with any other wave (no LDS, no barrier, no atomics: every
// output word has one writer, so a launch is bitwise reproducible).
//   stats   lane l < 16 is env e0 + l: ep_ret += reward (f64), ep_len += 1; a done env emits its
//           episode row, adds it to its cumulative counters and restarts at 0.  Coalesced 4 / 8-B
//           accesses.
//   rare    a done env (about 1 in 216 per step): the whole wave copies its terminal stack and zeroes
//           its older frames (+0.0, or x * 0 with USV_WRAP_CLEAR_KEEPS_SIGN: wrap_clear_row).
//   push    the wave's 16 obs rows are one contiguous source span, copied into the ring slots of frame j
//           by copy_rows (usv_row_copy.hpp: 16-B pieces at declared 4-B alignment, three in flight).
//
// The step and the reset are one body each (wrap_step_body, wrap_reset_body) over a normalisation
// policy: WrapNoNorm here, WrapNorm of usv_norm.hpp for VecNormalize.  The policy is also the copy's
// transform.  The plain kernels' policy is empty: they take no NormArgs, no LDS and no barrier.
//
// Ordering within an env's ring row (the argument of usv_noscan_step.hpp for its obs span): all
// accesses to the row in a launch come from the wave that owns the env, and launches on a stream are
// ordered by their boundary.  Within the wave:
//   - the terminal read of the slots p+1 .. p+k-1 must see them before the clear zeroes them: the wave
//     waits for its loads (vmcnt(0)) before it issues the first zero;
//   - the clear and the push write disjoint slots (the clear spares exactly the slots of j), so their
//     order does not matter; nor does the order of the terminal read and the push.
#pragma once

#include "usv_wrap_layout.hpp"
#include "usv_row_copy.hpp"

namespace usv {

struct WrapArgs {
  int n, D, k, reward_bytes;
  int p, m, term;               // slots of frame j (mirror or -1), first slot of the terminal stack
  int keep_sign;                // USV_WRAP_CLEAR_KEEPS_SIGN: a done env's older frames are multiplied by zero
  size_t stride;                // floats per ring row
  float* ring;
  double* ep_ret;
  int32_t* ep_len;
  double* episode;              // [n][2] or null
  double* cum_ret;              // [n] or null (the three together)
  long long* cum_len;
  long long* cum_eps;
};

// No normalisation: nothing besides the wrappers' own work, and the frames are stored as they are.
struct WrapNoNorm : RowCopyPlain {
  template <typename RW>
  __device__ __forceinline__ void reward(int, RW) const {}   // env e's raw reward of this step
  __device__ __forceinline__ void restart(int) const {}      // env e starts an episode
};

// Zero every slot of a ring row but those of frame j (wrap_clears_slot), the whole wave.  KEEP_SIGN:
// x * 0 instead of +0.0, i.e. -0.0 where x was negative, as a stack cleared by a mask multiply holds
// (the default path of the SB3 adapter); each lane reads the words it then writes.
template <bool KEEP_SIGN>
__device__ __forceinline__ void wrap_clear_row(float* row, const WrapArgs& a, int l) {
  const int slots = wrap_ring_slots(a.k);
  for (int q = 0; q < slots; ++q) {
    if (q == a.p || q == a.m) continue;                 // = !wrap_clears_slot(j, k, q)
    float* const s = row + (size_t)q * a.D;
    for (int c = l; c < a.D; c += kWave) s[c] = KEEP_SIGN ? s[c] * 0.0f : 0.0f;
  }
}

// Frame j of the wave's `ne` envs from src rows (row stride D) into the ring slots p and m.
template <typename NORM>
__device__ __forceinline__ void wrap_push(const WrapArgs& a, const float* src, int e0, int ne, int l, const NORM& nz) {
  const int D = a.D;
  float* const dst = a.ring + (size_t)e0 * a.stride + (size_t)a.p * D;
  const ptrdiff_t mir = a.m >= 0 ? (ptrdiff_t)(a.m - a.p) * D : 0;
  copy_rows(src + (size_t)e0 * D, D, dst, a.stride, a.m >= 0, mir, D, ne, l, nz);
}

// The step of a wave.  obs / rew / done / final_obs: what usv_step wrote; final_stack [n][k D] or null.
// RW: the reward's type (reward_bytes).
template <typename RW, typename NORM>
__device__ __forceinline__ void wrap_step_body(const WrapArgs& a, const float* obs, const RW* rew, const uint8_t* done,
                                               const float* final_obs, float* final_stack, const NORM& nz) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int e0 = (blockIdx.x * kWaves + wave) * kWrapEnvs;   // this wave's envs: e0 .. e0 + ne - 1
  const int ne = min(kWrapEnvs, a.n - e0);
  if (ne <= 0) return;
  // ---- stats (of the raw reward: the Monitor sits inside VecNormalize)
  bool dn = false;
  if (l < ne) {
    const int e = e0 + l;
    const RW rw = rew[e];
    double ret = a.ep_ret[e] + (double)rw;
    int len = a.ep_len[e] + 1;
    dn = done[e] != 0;
    nz.reward(e, rw);
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
      nz.restart(e);
    }
    a.ep_ret[e] = ret;
    a.ep_len[e] = len;
  }
  // ---- rare: done envs (terminal stack with the final obs last, then the clear)
  unsigned long long dm = ballot(dn);
  if (__builtin_expect(dm != 0ull, 0)) {
    const int D = a.D, older = (a.k - 1) * D;
    for (; dm; dm &= dm - 1) {
      const int e = e0 + __builtin_ctzll(dm);
      float* const row = a.ring + (size_t)e * a.stride;
      if (final_stack) {
        float* const f = final_stack + (size_t)e * a.k * D;
        const float* const t = row + (size_t)a.term * D;   // frames j-k+1 .. j-1
        for (int c = l; c < older; c += kWave) f[c] = t[c];
        const float* const fo = final_obs + (size_t)e * D;
        for (int c = l; c < D; c += kWave) f[older + c] = nz.one(fo[c], c);
        // the loads of the row have returned before the first zero below is issued
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      if (a.keep_sign) wrap_clear_row<true>(row, a, l); else wrap_clear_row<false>(row, a, l);
    }
  }
  // ---- push
  wrap_push(a, obs, e0, ne, l, nz);
}

// The reset of a wave: envs whose mask byte is set (MASKED = false: mask is null, all) restart at frame
// j: older frames zero, obs as frame j, counters 0.  Same work split as the step.
template <bool MASKED, typename NORM>
__device__ __forceinline__ void wrap_reset_body(const WrapArgs& a, const uint8_t* mask, const float* obs, const NORM& nz) {
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
      nz.restart(e0 + l);
    }
  }
  const unsigned long long rm = ballot(on);
  if (rm == 0ull) return;
  for (unsigned long long b = rm; b; b &= b - 1)
    wrap_clear_row<false>(a.ring + (size_t)(e0 + __builtin_ctzll(b)) * a.stride, a, l);
  const bool all = rm == (ne == 64 ? ~0ull : (1ull << ne) - 1);
  for (unsigned long long b = all ? 1ull : rm; b; b &= b - 1) {
    const int f = all ? 0 : __builtin_ctzll(b), cnt = all ? ne : 1;   // every env of the wave, or one row at a time
    wrap_push(a, obs, e0 + f, cnt, l, nz);
  }
}

template <typename RW>
__global__ __launch_bounds__(kBlock) void wrap_step_kernel(WrapArgs a, const float* obs, const RW* rew,
                                                          const uint8_t* done, const float* final_obs,
                                                          float* final_stack) {
  wrap_step_body(a, obs, rew, done, final_obs, final_stack, WrapNoNorm{});
}

template <bool MASKED>
__global__ __launch_bounds__(kBlock) void wrap_reset_kernel(WrapArgs a, const uint8_t* mask, const float* obs) {
  wrap_reset_body<MASKED>(a, mask, obs, WrapNoNorm{});
}

}  // namespace usv
