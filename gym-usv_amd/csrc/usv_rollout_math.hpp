// usv_rollout_math.hpp -- the arithmetic and the work split of the device rollout buffer
// (usv_rollout.hpp): the truncation bootstrap, one step of the GAE recurrence, and how the terminal
// slots of a step are numbered.  Plain C++ marked __host__ __device__, no HIP types: the kernels and a
// stand-alone host program (tests/test_rollout_math.py) run the same functions in the same order.
//
// Rounding.  SB3's RolloutBuffer computes in float32 NumPy arrays: every operation is rounded to f32 on
// its own.  The lines below hold a * b + c shapes that clang contracts into an FMA by default, on the
// device and on the host; each function that has one switches contraction off for its body, so the
// result is the two-rounding one wherever this header is compiled.
//
// Slots.  A (t, env) pair bootstraps when the env was truncated and not terminated.  Its slot is the
// number of such pairs before it in (t, env) order within the rollout:
//   slot = base (pairs of the steps before t) + before (pairs of this step in the chunks before the
//          env's) + rank (pairs of this step earlier in the env's chunk),
// or -1 where that number is not below term_cap.  A chunk is ro_chunk_envs(N) consecutive envs: one
// block of kRoBlock = 256 up to 262 144 envs, then growing in steps of 256 so that there are never more
// than kRoMaxChunks = 1024 chunks (2^23 envs: 8 192 envs per chunk).  All three terms are sums of
// integers: they do not depend on the order in which anything ran.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__CUDACC__)
#define USV_RO_HD __host__ __device__ inline
#else
#define USV_RO_HD inline
#endif

namespace usv {

constexpr int kRoBlock = 256;          // envs a block ranks per pass = its threads
constexpr int kRoMaxChunks = 1024;
constexpr int kRoGaeAhead = 4;         // steps whose loads the GAE issues before it runs their chain

USV_RO_HD int ro_chunk_envs(int64_t N) {
  const int64_t per = (int64_t)kRoBlock * kRoMaxChunks;
  const int64_t m = (N + per - 1) / per;
  return (int)(kRoBlock * (m > 0 ? m : 1));
}
USV_RO_HD int ro_num_chunks(int64_t N) {
  const int64_t R = ro_chunk_envs(N);
  return (int)((N + R - 1) / R);
}

// collect_rollouts: `done and infos[idx].get("TimeLimit.truncated", False)`; the adapter sets
// TimeLimit.truncated = truncated and not terminated (gym_usv_amd/sb3.py).
USV_RO_HD bool ro_bootstraps(uint8_t terminated, uint8_t truncated) { return truncated != 0 && terminated == 0; }

USV_RO_HD int32_t ro_slot(int64_t base, int64_t before, int rank, int32_t cap) {
  const int64_t s = base + before + rank;
  return s < (int64_t)cap ? (int32_t)s : -1;
}
// (stored, overflow) of `total` pairs; the overflow saturates at INT32_MAX.
USV_RO_HD int32_t ro_stored(int64_t total, int32_t cap) { return total < (int64_t)cap ? (int32_t)total : cap; }
USV_RO_HD int32_t ro_overflow(int64_t total, int32_t cap) {
  const int64_t o = total - ro_stored(total, cap);
  return o > 2147483647 ? 2147483647 : (int32_t)o;
}

// float32(gamma) and float32(gamma * gae_lambda), the product taken in double as Python takes it.
USV_RO_HD float ro_g32(double gamma) { return (float)gamma; }
USV_RO_HD float ro_gl32(double gamma, double gae_lambda) { return (float)(gamma * gae_lambda); }

// collect_rollouts: rewards[idx] += self.gamma * terminal_value.
USV_RO_HD float ro_bootstrap(float rew, float g32, float terminal_value) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float p = g32 * terminal_value;
  return rew + p;
}

// compute_returns_and_advantage, one step: r the (bootstrapped) reward, val = values[t], nv =
// values[t + 1] (last_values at t = T - 1), start_next = episode_starts[t + 1] (dones at t = T - 1).
// Updates gae (= advantages[t]) and returns returns[t] = advantages[t] + values[t].
USV_RO_HD float ro_gae_step(float r, float val, float nv, uint8_t start_next, float g32, float gl32, float& gae) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float nnt = 1.0f - (float)start_next;
  const float a = g32 * nv;
  const float b = a * nnt;
  const float c = r + b;
  const float delta = c - val;
  const float d = gl32 * nnt;
  const float e = d * gae;
  gae = delta + e;
  return gae + val;
}

}  // namespace usv
