// usv_replay_math.hpp -- the index and liveness arithmetic of the device replay buffer (usv_replay.hpp):
// SB3's ReplayBuffer (common/buffers.py: add, sample, _get_samples; optimize_memory_usage=False,
// handle_timeout_termination=True) with one D-float frame per transition where SB3 keeps two k D stacks.
// Plain C++ marked __host__ __device__, no HIP types, as usv_rollout_frames_math.hpp (whose clear rule,
// rf_slot_value / rf_cleared, and index check this one uses): the kernels and a stand-alone host program
// (tests/test_replay_math.py) run the same functions.
//
// Steps and slots.  Env step c = 0, 1, .. counts the put_obs calls since construction or clear(); `count`
// is the number of completed transitions (put_step calls).  The ring has R rows: transition c lives in
// slot c mod R of act / rew / done / timeout / age / next_frame, all [R][n][..].  size = min(count, R)
// slots are valid; the step a valid slot holds is the largest c' < count with c' mod R == slot.  A flat
// index is i = slot * n + e.
//
// Frames.  frames [n][P][D], env-major, P = R + k - 1 rows per env: the frame of step c (the newest D
// columns of the window given to put_obs(c)) is row c mod P, and the k - 1 older frames of the first
// window are steps -(k - 1) .. -1, rows P - (k - 1) .. P - 1 (the mathematical modulus).  The window of
// transition c is frames c - k + 1 .. c: k rows from row (c - k + 1) mod P on, in at most two runs.  With
// P rows the window of the oldest valid transition, count - R, is still whole after put_obs(count - 1):
// frames count - R - k + 1 .. count - 1 are P rows.  put_obs(count) overwrites the oldest of them, so a
// gather between a put_obs and its put_step is refused.
// next_frame [R][n][D] holds the newest D columns of next_obs: of final_stack for a done env (SB3's
// terminal_observation), of the window after the step otherwise.  next_obs of transition c is frames
// c - k + 2 .. c followed by next_frame.
//
// Liveness.  age[slot][e] = a in [0, k - 1]: the newest 1 + a slots of the obs window are live, the older
// ones were cleared by the frame stack at an episode boundary.  The per-env counter starts at k - 1 (the
// first window is stored as the ring held it, cleared slots included, and counts as live); put_step makes
// it 0 for a done env and min(a + 1, k - 1) otherwise; put_obs copies it into age[slot].  The terminal
// stack is the one before the clear, so for done envs too the newest 1 + min(a + 1, k - 1) slots of
// next_obs are live: slot j of next_obs is live exactly when slot j + 1 of obs is, and its newest always.
// One mask therefore serves the k + 1 frames of a sample: frame j (0 .. k - 1 from the ring, k =
// next_frame) has the liveness of obs slot min(j, k - 1).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "usv_rollout_frames_math.hpp"

namespace usv {

constexpr int kRpKeepSign = 1;         // usv_replay.flags: USV_REPLAY_CLEAR_KEEPS_SIGN
constexpr int kRpRows = 4;             // samples a wave of the gather keeps in flight

USV_RO_HD int64_t rp_frame_rows(int32_t R, int32_t k) { return (int64_t)R + k - 1; }

USV_RO_HD int32_t rp_slot(int64_t c, int32_t R) { return (int32_t)(c % R); }
USV_RO_HD int64_t rp_size(int64_t count, int32_t R) { return count < (int64_t)R ? count : (int64_t)R; }
// The step held by a valid slot (slot < rp_size(count, R)).
USV_RO_HD int64_t rp_step_of_slot(int32_t slot, int64_t count, int32_t R) {
  return (int64_t)slot + (int64_t)R * ((count - 1 - slot) / R);
}
// The ring row of frame f >= -(k - 1).
USV_RO_HD int32_t rp_frame_row(int64_t f, int64_t P) {
  const int64_t m = f % P;
  return (int32_t)(m < 0 ? m + P : m);
}

// What the gather needs of `count`, as 32-bit numbers: a slot <= last holds a step of the newest lap, whose
// window begins at row (first[0] + slot) mod P; a later slot one of the lap before, from first[1].
struct RpLaps {
  int32_t last, first[2];
};
USV_RO_HD RpLaps rp_laps(int64_t count, int32_t R, int32_t k) {
  const int64_t P = rp_frame_rows(R, k), q = (count - 1) / R;
  RpLaps g;
  g.last = (int32_t)((count - 1) % R);
  g.first[0] = rp_frame_row(q * R - (k - 1), P);
  g.first[1] = rp_frame_row((q - 1) * R - (k - 1), P);   // (unused while count <= R: every slot <= last)
  return g;
}
// The first frame row of the window in `slot`; frame j of it is row rp_wrap(first + j, P).
USV_RO_HD int32_t rp_first_row(const RpLaps& g, int32_t slot, int32_t P) {
  const int32_t r = g.first[slot <= g.last ? 0 : 1] + slot;
  return r >= P ? r - P : r;
}
USV_RO_HD int32_t rp_wrap(int32_t row, int32_t P) { return row >= P ? row - P : row; }

// First float of frame row `row` of env e, and of the row of (slot, e) in a [R][n][w] buffer.
USV_RO_HD size_t rp_frame_offset(int64_t e, int64_t row, int64_t P, int32_t D) {
  return ((size_t)e * (size_t)P + (size_t)row) * (size_t)D;
}
USV_RO_HD size_t rp_slot_offset(int64_t slot, int64_t e, int64_t n, int32_t w) {
  return ((size_t)slot * (size_t)n + (size_t)e) * (size_t)w;
}

USV_RO_HD bool rp_index_ok(int64_t idx, int64_t size, int64_t n) { return rf_index_ok(idx, size * n); }

// Bit j set: slot j of the obs window is live.
USV_RO_HD uint32_t rp_live_mask(int32_t age, int32_t k) {
  const int32_t dead = k - 1 - age;                     // the oldest `dead` slots
  return rf_all_live(k) & ~(dead <= 0 ? 0u : (1u << dead) - 1u);
}
// ... of the next_obs window: (obs mask >> 1) and its newest slot.
USV_RO_HD uint32_t rp_next_live_mask(int32_t age, int32_t k) { return (rp_live_mask(age, k) >> 1) | (1u << (k - 1)); }
// Frame j of a sample's k + 1 (k: next_frame), as it appears in obs column block j and next_obs block j - 1.
USV_RO_HD float rp_frame_value(float x, uint32_t live, int j, int32_t k, bool keep_sign) {
  return rf_slot_value(x, live, j < k - 1 ? j : k - 1, keep_sign);
}

USV_RO_HD int32_t rp_age_start(int32_t k) { return k - 1; }
USV_RO_HD int32_t rp_age_next(int32_t age, bool done, int32_t k) {
  if (done) return 0;
  return age + 1 < k - 1 ? age + 1 : k - 1;
}

// OffPolicyAlgorithm / the adapter (gym_usv_amd/sb3.py): done = terminated | truncated,
// TimeLimit.truncated = truncated and not terminated.
USV_RO_HD uint8_t rp_done(uint8_t terminated, uint8_t truncated) { return (terminated | truncated) != 0; }
USV_RO_HD uint8_t rp_timeout(uint8_t terminated, uint8_t truncated) { return truncated != 0 && terminated == 0; }
// _get_samples: self.dones[i] * (1 - self.timeouts[i]), float32.
USV_RO_HD float rp_done_out(uint8_t done, uint8_t timeout) { return (float)done * (1.0f - (float)timeout); }

// A frame of D >= 4 floats is cut into rp_pieces(D) pieces of four, the last moved back to end with it.
USV_RO_HD int32_t rp_pieces(int32_t D) { return (D + 3) / 4; }
USV_RO_HD int32_t rp_piece_col(int32_t piece, int32_t D) { return 4 * piece < D - 4 ? 4 * piece : D - 4; }

// ---- n-step sampling (SB3 2.7's NStepReplayBuffer._get_samples; tests/replay_nstep_ref.py restates it)
// The run of sample (slot, e) walks s_j = (slot + j) mod R for j = 0 .. n_steps - 1 and ends at m, the first
// j with done[s_j], timeout[s_j] or s_j == last (SB3's temporary timeouts[pos - 1] |= ~dones[pos - 1]: a
// run never crosses the write position of a full ring, nor enters the unwritten rows of a partly filled
// one), else at n_steps - 1.  rewards = rew[s_0] for m == 0, else the float32 sum in the order j = 0 .. m of
// fl(rew[s_j] g[j]), every product and sum rounded on its own; discounts = g[m + 1]; dones and next_obs are
// those of transition (s_m, e).  g[j] = float32(double(gamma) ** j), j = 0 .. n_steps, is the caller's.
constexpr int kRpMaxNStep = 32;

USV_RO_HD int32_t rp_next_slot(int32_t s, int32_t R) { return s + 1 >= R ? 0 : s + 1; }
USV_RO_HD bool rp_run_ends(uint8_t done, uint8_t timeout, int32_t s, int32_t last) {
  return done != 0 || timeout != 0 || s == last;
}
// acc + fl(rew * g): two roundings, never one fused multiply-add.
USV_RO_HD float rp_return_add(float acc, float rew, float g) {
#pragma clang fp contract(off)
  const float term = rew * g;
  return acc + term;
}

struct RpRun {
  int32_t m, slot;                     // the stop index and s_m
  float ret;                           // the return so far
  uint8_t done, timeout, age;          // of (s_m, e)
  bool open;                           // no step has ended the run yet
};
USV_RO_HD RpRun rp_run_begin() { return RpRun{0, 0, 0.0f, 0, 0, 0, true}; }
// Step j of the walk, at slot s, with what transition (s, e) stores; a step behind the stop changes nothing,
// so the caller may load every step's values before it applies any.
USV_RO_HD void rp_run_step(RpRun& r, int32_t j, int32_t s, uint8_t done, uint8_t timeout, uint8_t age, float rew,
                           float gj, int32_t last) {
  if (!r.open) return;
  r.m = j;
  r.slot = s;
  r.done = done;
  r.timeout = timeout;
  r.age = age;
  r.ret = j == 0 ? rew : rp_return_add(r.ret, rew, gj);
  r.open = !rp_run_ends(done, timeout, s, last);
}
// Frame row j = 0 .. k - 2 of the next_obs window of transition c + m (steps c + m - k + 2 .. c + m), `first`
// being the first row of the obs window of c: first + m + 1 + j <= (P - 1) + (R - 1) + 1 + (k - 2) < 2 P.
// Slot k - 1 of that window is next_frame[s_m]; its liveness is rp_next_live_mask(age[s_m], k).
USV_RO_HD int32_t rp_nstep_row(int32_t first, int32_t m, int32_t j, int32_t P) { return rp_wrap(first + m + 1 + j, P); }

}  // namespace usv
