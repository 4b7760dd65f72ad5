// usv_rollout_frames.hpp -- frame-deduplicated obs storage for the device rollout buffer and the
// minibatch gather (SB3's RolloutBuffer.get / _get_samples): usv_rollout_put_obs_frames and
// usv_rollout_gather (include/usv_hip.h).  The layout, the live mask and the clear rule are
// usv_rollout_frames_math.hpp's.
//
//   rollout_frames_obs_kernel  rollout_obs_kernel's work (rollout_put_rows, usv_rollout.hpp) with a
//                              destination row stride: row t of act / val / logp, and of each env's window
//                              the columns that are new -- all k D at t = 0 (frame rows 0 .. k - 1), the
//                              newest D afterwards (frame row t + k - 1).
//   rollout_gather_kernel      a wave owns kRfRows = 4 consecutive samples.  Lane r < 4 reads idx[b0 + r],
//                              checks it, splits it into (t, e), builds the live mask from at most k - 1
//                              start bytes and moves the four scalars; the offsets and masks are then
//                              broadcast (readlane: wave-uniform).  The obs rows are cut into 16-B pieces
//                              as above, on both sides; lane l takes pieces l, l + 64, .. of all four rows,
//                              so four loads are in flight per lane and the slot of each of a piece's four
//                              columns is worked out once for the four rows.  The mask is applied per
//                              element (a piece straddles frames when D is no multiple of 4) and only to
//                              rows that have a cleared slot.  Without frames (full storage) the source
//                              row is idx * W of obs and every slot is live.
//                              An index outside [0, T n) is never used as an address: its obs row, action
//                              and scalars are NaN and it is counted in bad_count (the kernel's only
//                              atomic, an integer add: the outputs are bitwise reproducible).
#pragma once

#include "usv_rollout_frames_math.hpp"
#include "usv_rollout.hpp"

namespace usv {

struct RfArgs {
  int k, D, keep_sign;
  float* frames;                // [n][T + k - 1][D], or null: full storage (gather only)
  int32_t* bad;                 // [1]
};

__global__ __launch_bounds__(kBlock) void rollout_frames_obs_kernel(RoArgs a, RfArgs f, int t, const float* src,
                                                                   size_t sstride, const float* act, const float* val,
                                                                   const float* logp) {
  rollout_put_rows(a, t, src + rf_put_col(t, f.k, f.D), sstride,
                   f.frames + rf_row_offset(0, rf_put_row(t, f.k), a.T, f.k, f.D), (size_t)rf_rows(a.T, f.k) * f.D,
                   rf_put_width(t, f.k, f.D), act, val, logp);
}

// rollout_gather_kernel: the body is usv_rollout_gather.inc's, which usv_rollout_perm.hpp includes again.
#define USV_GATHER_KERNEL rollout_gather_kernel
#define USV_GATHER_INDEX_PARAM const int64_t* idx
#define USV_GATHER_PROLOGUE
#define USV_GATHER_LANE_INDEX idx[b0 + l]
#define USV_GATHER_BROADCAST
#define USV_GATHER_ROW_INDEX idx[b0 + r]
#include "usv_rollout_gather.inc"
#undef USV_GATHER_KERNEL
#undef USV_GATHER_INDEX_PARAM
#undef USV_GATHER_PROLOGUE
#undef USV_GATHER_LANE_INDEX
#undef USV_GATHER_BROADCAST
#undef USV_GATHER_ROW_INDEX

}  // namespace usv
