// usv_rollout_perm.hpp -- the minibatch gather that a HIP graph can replay: usv_rollout_gather_perm
// (include/usv_hip.h).  Which minibatch a call reads is not an argument: it is the two-word cursor in device memory,
// and the sample of each position is usv_rollout_perm_math.hpp's keyed bijection, computed here.
//
//   rollout_gather_perm_kernel   usv_rollout_gather.inc a second time.  A wave reads the cursor's (epoch, batch) once
//                                (scalar, as sde_epoch_word) and derives the six round keys from (seed, epoch): the
//                                same values in every lane, two Philox blocks.  Lane r < 4 then walks position
//                                batch B + b0 + r to its sample index, in place of reading idx[b0 + r], and writes
//                                it to idx_out if there is one.  The four indices are made wave-uniform by readlane
//                                before the action loop, which picks its row's among them: the walk is not redone per
//                                element.  An index is always in [0, T n), so bad_count stays as it is.
//   rollout_cursor_tick_kernel   one thread moves the cursor on (cursor_ticked), with plain stores.  It is launched
//                                behind the gather in the same call: stream order has the gather read the old words.
#pragma once

#include "usv_rollout_frames.hpp"
#include "usv_rollout_perm_math.hpp"
#include "usv_sde.hpp"             // sde_epoch_word

namespace usv {

// The wave-uniform index of row r < kRfRows among the four broadcast ones.
__device__ __forceinline__ int64_t rollout_perm_pick(const int64_t (&ri)[kRfRows], int r) {
  int64_t i = ri[0];
#pragma unroll
  for (int x = 1; x < kRfRows; ++x) i = r == x ? ri[x] : i;
  return i;
}

#define USV_GATHER_KERNEL rollout_gather_perm_kernel
#define USV_GATHER_INDEX_PARAM const RolloutCursor* __restrict__ cursor, uint64_t seed, uint32_t n_batches, \
                               int64_t* __restrict__ idx_out
#define USV_GATHER_PROLOGUE                                                                                     \
  const uint32_t epoch = sde_epoch_word(&cursor->epoch);                                                        \
  const uint32_t batch = cursor_batch(sde_epoch_word(&cursor->batch), n_batches);                               \
  const PermKeys keys = perm_keys(seed, epoch);                                                                 \
  int64_t mine = 0;
#define USV_GATHER_LANE_INDEX (mine = perm_index_keyed(keys, total, (int64_t)batch * B + b0 + l));              \
    if (idx_out) idx_out[b0 + l] = mine
#define USV_GATHER_BROADCAST                                                                                    \
  int64_t ri[kRfRows];                                                                                          \
  _Pragma("unroll") for (int x = 0; x < kRfRows; ++x)                                                           \
    ri[x] = (int64_t)(((unsigned long long)__builtin_amdgcn_readlane((uint32_t)((unsigned long long)mine >> 32), x) << 32) | \
                      __builtin_amdgcn_readlane((uint32_t)mine, x));
#define USV_GATHER_ROW_INDEX rollout_perm_pick(ri, r)
#include "usv_rollout_gather.inc"
#undef USV_GATHER_KERNEL
#undef USV_GATHER_INDEX_PARAM
#undef USV_GATHER_PROLOGUE
#undef USV_GATHER_LANE_INDEX
#undef USV_GATHER_BROADCAST
#undef USV_GATHER_ROW_INDEX

__global__ void rollout_cursor_tick_kernel(RolloutCursor* __restrict__ cursor, uint32_t n_batches) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t epoch = cursor->epoch, batch = cursor->batch;
  cursor_ticked(epoch, batch, n_batches);
  cursor->epoch = epoch;
  cursor->batch = batch;
}

}  // namespace usv
