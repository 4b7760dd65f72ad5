// usv_replay.hpp -- SB3's ReplayBuffer (common/buffers.py: add, sample / _get_samples) and the
// terminal-observation substitution of OffPolicyAlgorithm._store_transition behind the fused wrappers,
// stream-ordered and without a host sync: usv_replay_put_obs / _put_step / _gather (include/usv_hip.h).
// The layout, the slot and row numbering, the live mask and the clear rule are usv_replay_math.hpp's.
//
//   replay_obs_kernel     a wave owns kWrapEnvs = 16 envs: act[slot], age[slot] (the per-env counter) and
//                         the newest D columns of each env's window into its frame row, by copy_rows
//                         (usv_row_copy.hpp) from a strided source; at step 0 the older (k - 1) D columns
//                         too, into the prologue rows (one contiguous run per env).
//   replay_step_kernel    the same split: rew / done / timeout[slot], the counter's update, and
//                         next_frame[slot]: the newest D columns of final_stack for a done env, of the
//                         window after the step otherwise.  The done bytes of the wave's envs are one
//                         ballot; a piece's source pointer is selected by its env's bit, so the 16-B loads
//                         stay unconditional.
//   replay_gather_kernel  a wave owns kRpRows = 4 consecutive samples.  Lane r < 4 reads idx[b0 + r],
//                         checks it, splits it into (slot, e), fetches age and moves the two scalars; the
//                         offsets, the first frame row and the mask are then broadcast (readlane:
//                         wave-uniform).  The k + 1 frames of a sample (k ring rows, taken mod P one by
//                         one: a window may wrap the ring end, and next_frame) are each cut into 16-B
//                         pieces at 4-B alignment; lane l takes pieces l, l + 64, .. of all four samples,
//                         so four loads are in flight per lane.  A piece lies in one frame: its liveness is
//                         one bit, and it is stored to observations (column block j) and to
//                         next_observations (block j - 1): (k + 1) D floats read, 2 k D written.
//                         An index outside [0, size n) is never used as an address: its outputs are NaN
//                         and it is counted in bad_count (the kernel's only atomic, an integer add: the
//                         outputs are bitwise reproducible).  A refused or absent sample loads row 0 of
//                         env 0 (always there) and drops it.
// D < 4 takes one float per piece.
//   replay_gather_nstep_kernel  (at the end of this file) the same split for SB3's n-step samples: lane r
//                         also walks its sample's run, and the two windows are 2 k frames.
#pragma once

#include "usv_replay_math.hpp"
#include "usv_row_copy.hpp"

namespace usv {

struct RpArgs {
  int n, R, W, A, k, D, keep_sign;
  int P;                        // rp_frame_rows(R, k)
  float* frames;                // [n][P][D]
  float* next_frame;            // [R][n][D]
  float* act;                   // [R][n][A]
  float* rew;                   // [R][n]
  uint8_t* done;                // [R][n]
  uint8_t* timeout;             // [R][n]
  uint8_t* age;                 // [R][n]
  uint8_t* age_now;             // [n]
  int32_t* bad;                 // [1]
};

// row: the frame row of this step; first: step 0, whose older frames go to the prologue rows.
__global__ __launch_bounds__(kBlock) void replay_obs_kernel(RpArgs a, int slot, int row, int first, const float* src,
                                                           size_t sstride, const float* act) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int e0 = (blockIdx.x * kWaves + wave) * kWrapEnvs;
  const int ne = min(kWrapEnvs, a.n - e0);
  if (ne <= 0) return;
  const size_t s0 = rp_slot_offset(slot, e0, a.n, 1);
  if (l < ne) a.age[s0 + l] = a.age_now[e0 + l];
  for (int q = l; q < ne * a.A; q += kWave) a.act[s0 * a.A + q] = act[(size_t)e0 * a.A + q];
  const size_t es = (size_t)a.P * a.D;                  // floats per env of the frame ring
  const float* const s = src + (size_t)e0 * sstride;
  float* const d = a.frames + (size_t)e0 * es;
  const int older = (a.k - 1) * a.D;
  if (first && older > 0)
    copy_rows(s, sstride, d + (size_t)rp_frame_row(-(int64_t)(a.k - 1), a.P) * a.D, es, false, 0, older, ne, l,
              RowCopyPlain{});
  copy_rows(s + older, sstride, d + (size_t)row * a.D, es, false, 0, a.D, ne, l, RowCopyPlain{});
}

template <typename RW>
__global__ __launch_bounds__(kBlock) void replay_step_kernel(RpArgs a, int slot, const RW* rew, const uint8_t* term,
                                                            const uint8_t* trunc, const float* next, size_t nstride,
                                                            const float* fin) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int e0 = (blockIdx.x * kWaves + wave) * kWrapEnvs;
  const int ne = min(kWrapEnvs, a.n - e0);
  if (ne <= 0) return;
  const size_t s0 = rp_slot_offset(slot, e0, a.n, 1);
  uint8_t dn = 0;
  if (l < ne) {
    const int e = e0 + l;
    const uint8_t tm = term[e], tr = trunc[e];
    dn = rp_done(tm, tr);
    a.rew[s0 + l] = (float)rew[e];
    a.done[s0 + l] = dn;
    a.timeout[s0 + l] = rp_timeout(tm, tr);
    a.age_now[e] = (uint8_t)rp_age_next(a.age_now[e], dn != 0, a.k);
  }
  const unsigned long long dm = ballot(dn != 0);        // bit i: env e0 + i is done
  const int D = a.D, col = (a.k - 1) * D;
  const float* const nx = next + (size_t)e0 * nstride + col;
  const float* const fs = fin + (size_t)e0 * a.W + col;
  float* const dst = a.next_frame + s0 * D;
  if (D >= 4) {
    const int Pf = rp_pieces(D), np = ne * Pf;
    for (int q = l; q < np; q += 2 * kWave) {
      const float* sp[2];
      float* dp[2];
      WrapQuad4 v[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int qq = min(q + i * kWave, np - 1);        // (a piece past the end repeats the last one's load)
        const int kk = qq / Pf, c = rp_piece_col(qq - kk * Pf, D);
        sp[i] = ((dm >> kk) & 1ull ? fs + (size_t)kk * a.W : nx + (size_t)kk * nstride) + c;
        dp[i] = dst + (size_t)kk * D + c;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) v[i] = *reinterpret_cast<const WrapQuad*>(sp[i]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (q + i * kWave < np) *reinterpret_cast<WrapQuad*>(dp[i]) = v[i];
    }
  } else {
    for (int q = l; q < ne * D; q += kWave) {
      const int kk = q / D, c = q - kk * D;
      dst[q] = ((dm >> kk) & 1ull ? fs + (size_t)kk * a.W : nx + (size_t)kk * nstride)[c];
    }
  }
}

__global__ __launch_bounds__(kBlock) void replay_gather_kernel(RpArgs a, RpLaps g, long long size, const int64_t* idx,
                                                              int B, float* obs_out, float* act_out, float* next_out,
                                                              float* done_out, float* rew_out) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int64_t b0 = ((int64_t)blockIdx.x * kWaves + wave) * kRpRows;
  if (b0 >= B) return;
  const int nb = (int)min((int64_t)kRpRows, B - b0);    // wave-uniform
  const int64_t total = (int64_t)size * a.n;
  const int W = a.W, D = a.D, k = a.k, P = a.P;
  const float nan = __builtin_nanf("");
  const bool keep = a.keep_sign != 0;
  const uint32_t all = rf_all_live(k);
  // ---- lane r < nb: sample b0 + r
  bool ok = false;
  uint32_t live = all;
  int first = 0;
  unsigned long long eoff = 0, noff = 0;                // the env's frame rows; the sample's next_frame row
  if (l < nb) {
    const int64_t i = idx[b0 + l];
    ok = rf_index_ok(i, total);
    float dv = nan, rw = nan;
    if (ok) {
      int64_t slot;
      if (total <= 0xffffffffll) slot = (int64_t)((uint32_t)i / (uint32_t)a.n);
      else slot = i / a.n;
      const int64_t e = i - slot * a.n;
      dv = rp_done_out(a.done[i], a.timeout[i]);
      rw = a.rew[i];
      live = rp_live_mask(a.age[i], k);
      first = rp_first_row(g, (int32_t)slot, P);
      eoff = rp_frame_offset(e, 0, P, D);
      noff = (unsigned long long)i * (unsigned long long)D;
    }
    done_out[b0 + l] = dv;
    rew_out[b0 + l] = rw;
  }
  const unsigned long long bad = ballot(l < nb && !ok);
  if (bad != 0ull && l == 0) atomicAdd(a.bad, (int)__builtin_popcountll(bad));
  // ---- actions
  for (int q = l; q < nb * a.A; q += kWave) {
    const int r = q / a.A, c = q - r * a.A;
    const int64_t i = idx[b0 + r];
    act_out[(size_t)(b0 + r) * a.A + c] = rf_index_ok(i, total) ? a.act[(size_t)i * a.A + c] : nan;
  }
  // ---- the k + 1 frames
  if (D >= 4) {
    size_t reoff[kRpRows], rnoff[kRpRows];
    int rfirst[kRpRows];
    uint32_t rlive[kRpRows];
    bool rok[kRpRows];
#pragma unroll
    for (int r = 0; r < kRpRows; ++r) {                 // wave-uniform copies of lane r's values
      const uint32_t elo = __builtin_amdgcn_readlane((uint32_t)eoff, r);
      const uint32_t ehi = __builtin_amdgcn_readlane((uint32_t)(eoff >> 32), r);
      const uint32_t nlo = __builtin_amdgcn_readlane((uint32_t)noff, r);
      const uint32_t nhi = __builtin_amdgcn_readlane((uint32_t)(noff >> 32), r);
      rlive[r] = __builtin_amdgcn_readlane(live, r);
      rok[r] = r < nb && __builtin_amdgcn_readlane((uint32_t)ok, r) != 0;
      // (a refused or absent sample carries offsets 0 and first row 0: the loads stay unconditional)
      rfirst[r] = (int)__builtin_amdgcn_readlane((uint32_t)first, r);
      reoff[r] = (size_t)(((unsigned long long)ehi << 32) | elo);
      rnoff[r] = (size_t)(((unsigned long long)nhi << 32) | nlo);
    }
    const int Pf = rp_pieces(D), np = (k + 1) * Pf;
    for (int p = l; p < np; p += kWave) {
      const int j = p / Pf, c = rp_piece_col(p - j * Pf, D);
      WrapQuad4 v[kRpRows];
#pragma unroll
      for (int r = 0; r < kRpRows; ++r) {
        const float* const sp = j == k ? a.next_frame + rnoff[r]
                                       : a.frames + reoff[r] + (size_t)rp_wrap(rfirst[r] + j, P) * D;
        v[r] = *reinterpret_cast<const WrapQuad*>(sp + c);
      }
#pragma unroll
      for (int r = 0; r < kRpRows; ++r) {
        if (r >= nb) continue;
        WrapQuad4 o = {nan, nan, nan, nan};
        if (rok[r]) {
          o = v[r];
          if (rlive[r] != all) {
#pragma unroll
            for (int x = 0; x < 4; ++x) o[x] = rp_frame_value(o[x], rlive[r], j, k, keep);
          }
        }
        const size_t ob = (size_t)(b0 + r) * W + c;
        if (j < k) *reinterpret_cast<WrapQuad*>(obs_out + ob + (size_t)j * D) = o;
        if (j >= 1) *reinterpret_cast<WrapQuad*>(next_out + ob + (size_t)(j - 1) * D) = o;
      }
    }
  } else {
    // D < 4: one float per lane; the trip count is wave-uniform, so every lane takes part in the shuffles
    const int F = (k + 1) * D;
    for (int q0 = 0; q0 < nb * F; q0 += kWave) {
      const int q = q0 + l;
      const int r = min(q / F, nb - 1), u = q - (q / F) * F, j = u / D, c = u - j * D;
      const int okr = __shfl((int)ok, r);
      const uint32_t lv = __shfl(live, r);
      const int fr = __shfl(first, r);
      const unsigned long long eo = __shfl(eoff, r), no = __shfl(noff, r);
      if (q >= nb * F) continue;
      float o = nan;
      if (okr) {
        const float* const sp = j == k ? a.next_frame + (size_t)no : a.frames + (size_t)eo + (size_t)rp_wrap(fr + j, P) * D;
        o = rp_frame_value(sp[c], lv, j, k, keep);
      }
      const size_t ob = (size_t)(b0 + r) * W + c;
      if (j < k) obs_out[ob + (size_t)j * D] = o;
      if (j >= 1) next_out[ob + (size_t)(j - 1) * D] = o;
    }
  }
}

// 1 (never the product; tools/replay_nstep_ab.py --libs compares builds): a ring row that both windows of a
// sample hold (m < k - 1) is loaded once, by the obs pass, and stored to both under their own masks.
#ifndef USV_RP_NSTEP_SHARE
#define USV_RP_NSTEP_SHARE 0
#endif

// g[j] = float32(gamma ** j), j = 0 .. n_steps: by value in the kernel's arguments
struct RpDiscounts {
  float g[kRpMaxNStep + 1];
};

// The n-step gather (usv_replay_math.hpp, "n-step sampling"): replay_gather_kernel's split.  Lane r < 4
// also walks its sample's run: the done / timeout / age bytes and the reward of four steps at a time, at
// stride n, loaded before any is applied (every slot of the ring is an address inside the buffers), until
// the run has ended.  obs is the window of (slot, e) under its own mask; next_obs the window of (s_m, e):
// k - 1 ring rows from rp_nstep_row on and next_frame[s_m], under the mask of age[s_m].  The two windows
// are 2 k separate frames to the piece loop, each piece loaded once and stored once: 2 k D floats read,
// 2 k D written (rows the windows share when m < k - 1 are read twice, by the same wave).
__global__ __launch_bounds__(kBlock) void replay_gather_nstep_kernel(RpArgs a, RpLaps g, long long size,
                                                                    const int64_t* idx, int B, int n_steps,
                                                                    RpDiscounts tab, float* obs_out, float* act_out,
                                                                    float* next_out, float* done_out, float* rew_out,
                                                                    float* disc_out) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int64_t b0 = ((int64_t)blockIdx.x * kWaves + wave) * kRpRows;
  if (b0 >= B) return;
  const int nb = (int)min((int64_t)kRpRows, B - b0);    // wave-uniform
  const int64_t total = (int64_t)size * a.n;
  const int W = a.W, D = a.D, k = a.k, P = a.P;
  const float nan = __builtin_nanf("");
  const bool keep = a.keep_sign != 0;
  const uint32_t all = rf_all_live(k);
  // ---- lane r < nb: sample b0 + r and its run
  bool ok = false;
  uint32_t live = all, nlive = all;                     // of the obs window; of the next_obs window
  int first = 0, m = 0;
  unsigned long long eoff = 0, noff = 0;                // the env's frame rows; next_frame[s_m]
  if (l < nb) {
    const int64_t i = idx[b0 + l];
    ok = rf_index_ok(i, total);
    float dv = nan, rw = nan, dc = nan;
    if (ok) {
      int64_t slot;
      if (total <= 0xffffffffll) slot = (int64_t)((uint32_t)i / (uint32_t)a.n);
      else slot = i / a.n;
      const int64_t e = i - slot * a.n;
      live = rp_live_mask(a.age[i], k);
      RpRun run = rp_run_begin();
      int s = (int)slot;
      for (int j0 = 0; j0 < n_steps && run.open; j0 += 4) {
        int sj[4];
        uint8_t dn[4], to[4], ag[4];
        float rv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const size_t at = rp_slot_offset(s, e, a.n, 1);
          sj[u] = s;
          dn[u] = a.done[at];
          to[u] = a.timeout[at];
          ag[u] = a.age[at];
          rv[u] = a.rew[at];
          s = rp_next_slot(s, a.R);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (j0 + u < n_steps) rp_run_step(run, j0 + u, sj[u], dn[u], to[u], ag[u], rv[u], tab.g[j0 + u], g.last);
      }
      m = run.m;
      dv = rp_done_out(run.done, run.timeout);
      rw = run.ret;
      dc = tab.g[m + 1];
      nlive = rp_next_live_mask(run.age, k);
      first = rp_first_row(g, (int32_t)slot, P);
      eoff = rp_frame_offset(e, 0, P, D);
      noff = (unsigned long long)rp_slot_offset(run.slot, e, a.n, D);
    }
    done_out[b0 + l] = dv;
    rew_out[b0 + l] = rw;
    disc_out[b0 + l] = dc;
  }
  const unsigned long long bad = ballot(l < nb && !ok);
  if (bad != 0ull && l == 0) atomicAdd(a.bad, (int)__builtin_popcountll(bad));
  // ---- actions
  for (int q = l; q < nb * a.A; q += kWave) {
    const int r = q / a.A, c = q - r * a.A;
    const int64_t i = idx[b0 + r];
    act_out[(size_t)(b0 + r) * a.A + c] = rf_index_ok(i, total) ? a.act[(size_t)i * a.A + c] : nan;
  }
  // ---- the 2 k frames: f < k is slot f of obs, f >= k slot f - k of next_obs
  if (D >= 4) {
    size_t reoff[kRpRows], rnoff[kRpRows];
    int rfirst[kRpRows], rm[kRpRows];
    uint32_t rlive[kRpRows], rnlive[kRpRows];
    bool rok[kRpRows];
#pragma unroll
    for (int r = 0; r < kRpRows; ++r) {                 // wave-uniform copies of lane r's values
      const uint32_t elo = __builtin_amdgcn_readlane((uint32_t)eoff, r);
      const uint32_t ehi = __builtin_amdgcn_readlane((uint32_t)(eoff >> 32), r);
      const uint32_t nlo = __builtin_amdgcn_readlane((uint32_t)noff, r);
      const uint32_t nhi = __builtin_amdgcn_readlane((uint32_t)(noff >> 32), r);
      rlive[r] = __builtin_amdgcn_readlane(live, r);
      rnlive[r] = __builtin_amdgcn_readlane(nlive, r);
      rok[r] = r < nb && __builtin_amdgcn_readlane((uint32_t)ok, r) != 0;
      // (a refused or absent sample carries offsets 0, first row 0 and m = 0: rows 0 .. k - 1 of env 0 and
      // next_frame[0], always there: the loads stay unconditional)
      rfirst[r] = (int)__builtin_amdgcn_readlane((uint32_t)first, r);
      rm[r] = (int)__builtin_amdgcn_readlane((uint32_t)m, r);
      reoff[r] = (size_t)(((unsigned long long)ehi << 32) | elo);
      rnoff[r] = (size_t)(((unsigned long long)nhi << 32) | nlo);
    }
    constexpr bool kShare = USV_RP_NSTEP_SHARE != 0;
    const int Pf = rp_pieces(D), np = 2 * k * Pf;
    for (int p = l; p < np; p += kWave) {
      const int f = p / Pf, c = rp_piece_col(p - f * Pf, D);
      const bool nx = f >= k;
      const int j = nx ? f - k : f;
      WrapQuad4 v[kRpRows] = {};
#pragma unroll
      for (int r = 0; r < kRpRows; ++r) {
        if (kShare && nx && j + rm[r] <= k - 2) continue;   // obs slot j + m + 1: loaded and stored there
        const int row = nx ? rp_nstep_row(rfirst[r], rm[r], min(j, k - 2), P) : rp_wrap(rfirst[r] + j, P);
        const float* const sp = nx && j == k - 1 ? a.next_frame + rnoff[r] : a.frames + reoff[r] + (size_t)row * D;
        v[r] = *reinterpret_cast<const WrapQuad*>(sp + c);
      }
      float* const out = nx ? next_out : obs_out;
#pragma unroll
      for (int r = 0; r < kRpRows; ++r) {
        if (r >= nb) continue;
        if (kShare && nx && j + rm[r] <= k - 2) continue;
        WrapQuad4 o = {nan, nan, nan, nan};
        if (rok[r]) {
          o = v[r];
          const uint32_t lv = nx ? rnlive[r] : rlive[r];
          if (lv != all) {
#pragma unroll
            for (int x = 0; x < 4; ++x) o[x] = rf_slot_value(o[x], lv, j, keep);
          }
        }
        *reinterpret_cast<WrapQuad*>(out + (size_t)(b0 + r) * W + (size_t)j * D + c) = o;
        if (kShare && !nx && j >= rm[r] + 1) {              // ... and slot j - m - 1 of next_obs, under its mask
          const int jn = j - rm[r] - 1;
          WrapQuad4 o2 = {nan, nan, nan, nan};
          if (rok[r]) {
            o2 = v[r];
#pragma unroll
            for (int x = 0; x < 4; ++x) o2[x] = rf_slot_value(o2[x], rnlive[r], jn, keep);
          }
          *reinterpret_cast<WrapQuad*>(next_out + (size_t)(b0 + r) * W + (size_t)jn * D + c) = o2;
        }
      }
    }
  } else {
    // D < 4: one float per lane; the trip count is wave-uniform, so every lane takes part in the shuffles
    const int F = 2 * k * D;
    for (int q0 = 0; q0 < nb * F; q0 += kWave) {
      const int q = q0 + l;
      const int r = min(q / F, nb - 1), u = q - (q / F) * F, f = u / D, c = u - f * D;
      const int okr = __shfl((int)ok, r);
      const uint32_t lv = __shfl(live, r), nlv = __shfl(nlive, r);
      const int fr = __shfl(first, r), mr = __shfl(m, r);
      const unsigned long long eo = __shfl(eoff, r), no = __shfl(noff, r);
      if (q >= nb * F) continue;
      const bool nx = f >= k;
      const int j = nx ? f - k : f;
      float o = nan;
      if (okr) {
        const int row = nx ? rp_nstep_row(fr, mr, min(j, k - 2), P) : rp_wrap(fr + j, P);
        const float* const sp = nx && j == k - 1 ? a.next_frame + (size_t)no : a.frames + (size_t)eo + (size_t)row * D;
        o = rf_slot_value(sp[c], nx ? nlv : lv, j, keep);
      }
      (nx ? next_out : obs_out)[(size_t)(b0 + r) * W + (size_t)j * D + c] = o;
    }
  }
}

}  // namespace usv
