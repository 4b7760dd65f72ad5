// usv_rollout_frames_math.hpp -- the index and liveness arithmetic of the frame-deduplicated rollout
// storage (usv_rollout_frames.hpp).  Plain C++ marked __host__ __device__, no HIP types, as
// usv_rollout_math.hpp: the kernels and a stand-alone host program (tests/test_rollout_frames_math.py)
// run the same functions.
//
// Layout.  frames [n][T + k - 1][D], env-major.  Row r of env e holds the frame pushed at time
// u = r - (k - 1): rows 0 .. k - 2 are the older frames of the window as it stood at put_obs(0), row
// t + k - 1 the newest frame of the window given to put_obs(t).  The k frames of sample (t, e) are rows
// t .. t + k - 1: one contiguous run of k D floats, slot j (0 = oldest) = row t + j = time t - (k - 1 - j).
//
// Liveness.  Slot j of sample (t, e) is cleared when an episode boundary lies between its frame and t:
// some s with max(u, 0) < s <= t and start[s][e] != 0 (start[t + 1] = term | trunc of step t, written by
// usv_rollout_put_step).  The slots with u < 0 were cleared by the ring itself for every boundary at or
// before step 0, so start[0] is never read.  The newest slot is always live.  At most k - 1 start bytes
// are read: s = t, t - 1 .. max(t - (k - 2), 1).
//
// Clear rule.  +0.0, or x * 0.0f with kRfKeepSign (-0.0 where x was negative, NaN where it was NaN or
// infinite): what DeviceWrappers(clear_keeps_sign=...) leaves in its ring.  x * 0 applied to a slot that
// the ring had cleared already gives the same bits again.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "usv_rollout_math.hpp"

namespace usv {

constexpr int kRfMaxStack = 32;        // k: the live mask is one 32-bit word
constexpr int kRfKeepSign = 1;         // usv_rollout_frames.flags: USV_ROLLOUT_FRAMES_CLEAR_KEEPS_SIGN
constexpr int kRfRows = 4;             // samples a wave of the gather keeps in flight

USV_RO_HD int64_t rf_rows(int32_t T, int32_t k) { return (int64_t)T + k - 1; }

// First float of frame row r of env e.
USV_RO_HD size_t rf_row_offset(int64_t e, int64_t r, int32_t T, int32_t k, int32_t D) {
  return ((size_t)e * (size_t)rf_rows(T, k) + (size_t)r) * (size_t)D;
}
// First float of the k D floats of sample (t, e).
USV_RO_HD size_t rf_sample_offset(int64_t e, int64_t t, int32_t T, int32_t k, int32_t D) {
  return rf_row_offset(e, t, T, k, D);
}

// What put_obs(t) copies from a [k D] window: columns [rf_put_col, rf_put_col + rf_put_width) into the
// frame rows from rf_put_row on.
USV_RO_HD int32_t rf_put_col(int32_t t, int32_t k, int32_t D) { return t == 0 ? 0 : (k - 1) * D; }
USV_RO_HD int32_t rf_put_width(int32_t t, int32_t k, int32_t D) { return t == 0 ? k * D : D; }
USV_RO_HD int64_t rf_put_row(int32_t t, int32_t k) { return t == 0 ? 0 : (int64_t)t + k - 1; }

USV_RO_HD bool rf_index_ok(int64_t idx, int64_t total) { return (uint64_t)idx < (uint64_t)total; }

USV_RO_HD uint32_t rf_all_live(int32_t k) { return k >= 32 ? 0xffffffffu : (1u << k) - 1u; }

// Bit j set: slot j of sample (t, e) is live.  start is [T + 1][n].
USV_RO_HD uint32_t rf_live_mask(const uint8_t* start, int64_t n, int64_t e, int32_t t, int32_t k) {
  uint32_t m = 1u << (k - 1);
  for (int j = k - 2; j >= 0; --j) {
    const int32_t s = t - (k - 2 - j);                  // the boundary between slot j and slot j + 1
    if (s >= 1 && start[(size_t)s * (size_t)n + (size_t)e] != 0) break;
    m |= 1u << j;
  }
  return m;
}

USV_RO_HD float rf_cleared(float x, bool keep_sign) { return keep_sign ? x * 0.0f : 0.0f; }

USV_RO_HD float rf_slot_value(float x, uint32_t live, int j, bool keep_sign) {
  return (live >> j) & 1u ? x : rf_cleared(x, keep_sign);
}

}  // namespace usv
