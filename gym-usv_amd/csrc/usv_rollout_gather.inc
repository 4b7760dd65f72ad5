// The minibatch gather, stated once and included twice.  The including header defines
//   USV_GATHER_KERNEL        the kernel's name: rollout_gather_kernel (usv_rollout_frames.hpp), then
//                            rollout_gather_perm_kernel (usv_rollout_perm.hpp)
//   USV_GATHER_INDEX_PARAM   where the indices come from: `const int64_t* idx`, then the cursor block, the seed and
//                            an optional idx_out
//   USV_GATHER_PROLOGUE      nothing, then what a wave derives once (the cursor's words, the keys)
//   USV_GATHER_LANE_INDEX    lane l's own sample index: `idx[b0 + l]`, then the walk of its position
//   USV_GATHER_BROADCAST     nothing, then the lanes' indices made wave-uniform for the action loop
//   USV_GATHER_ROW_INDEX     the index of row r in the action loop: `idx[b0 + r]`, then a pick among the broadcast ones
// The first inclusion is token for token the kernel as it stood before the second existed, so its code is unchanged
// (tools/asm_same.py, DESIGN.md).
__global__ __launch_bounds__(kBlock) void USV_GATHER_KERNEL(RoArgs a, RfArgs f, USV_GATHER_INDEX_PARAM, int B,
                                                               float* obs_out, float* act_out, float* val_out,
                                                               float* logp_out, float* adv_out, float* ret_out) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int64_t b0 = ((int64_t)blockIdx.x * kWaves + wave) * kRfRows;
  if (b0 >= B) return;
  const int nb = (int)min((int64_t)kRfRows, B - b0);    // wave-uniform
  const int64_t total = (int64_t)a.T * a.n;
  const int W = a.W, D = f.D;
  const float nan = __builtin_nanf("");
  const bool keep = f.keep_sign != 0;
  const uint32_t all = rf_all_live(f.k);
  USV_GATHER_PROLOGUE
  // ---- lane r < nb: sample b0 + r
  bool ok = false;
  uint32_t live = all;
  unsigned long long off = 0;
  if (l < nb) {
    const int64_t i = USV_GATHER_LANE_INDEX;
    ok = rf_index_ok(i, total);
    float v = nan, lp = nan, ad = nan, rt = nan;
    if (ok) {
      v = a.val[i];
      lp = a.logp[i];
      ad = a.adv[i];
      rt = a.ret[i];
      if (f.frames) {
        int64_t t;
        if (total <= 0xffffffffll) t = (int64_t)((uint32_t)i / (uint32_t)a.n);
        else t = i / a.n;
        const int64_t e = i - t * a.n;
        live = rf_live_mask(a.start, a.n, e, (int32_t)t, f.k);
        off = rf_sample_offset(e, t, a.T, f.k, D);
      } else {
        off = (unsigned long long)i * (unsigned long long)W;
      }
    }
    val_out[b0 + l] = v;
    logp_out[b0 + l] = lp;
    adv_out[b0 + l] = ad;
    ret_out[b0 + l] = rt;
  }
  const unsigned long long bad = ballot(l < nb && !ok);
  if (bad != 0ull && l == 0) atomicAdd(f.bad, (int)__builtin_popcountll(bad));
  USV_GATHER_BROADCAST
  // ---- actions
  for (int q = l; q < nb * a.A; q += kWave) {
    const int r = q / a.A, c = q - r * a.A;
    const int64_t i = USV_GATHER_ROW_INDEX;
    act_out[(size_t)(b0 + r) * a.A + c] = rf_index_ok(i, total) ? a.act[(size_t)i * a.A + c] : nan;
  }
  // ---- obs rows
  const float* const src = f.frames ? f.frames : a.obs;
  if (W >= 4) {
    size_t roff[kRfRows];
    uint32_t rlive[kRfRows];
    bool rok[kRfRows];
#pragma unroll
    for (int r = 0; r < kRfRows; ++r) {                 // wave-uniform copies of lane r's values
      const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)off, r);
      const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(off >> 32), r);
      rlive[r] = __builtin_amdgcn_readlane(live, r);
      rok[r] = r < nb && __builtin_amdgcn_readlane((uint32_t)ok, r) != 0;
      // a refused or absent row loads row 0 instead (always there) and drops it: the four loads stay
      // unconditional, so nothing waits between them
      roff[r] = rok[r] ? (size_t)(((unsigned long long)hi << 32) | lo) : 0;
    }
    const int P = (W + 3) / 4;
    for (int p = l; p < P; p += kWave) {
      const int c = min(4 * p, W - 4);
      int sl[4];                                        // the slots of columns c .. c + 3
      {
        int j = c / D, rem = c - j * D;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          sl[x] = j;
          if (++rem == D) { rem = 0; ++j; }
        }
      }
      WrapQuad4 v[kRfRows];
#pragma unroll
      for (int r = 0; r < kRfRows; ++r) v[r] = *reinterpret_cast<const WrapQuad*>(src + roff[r] + c);
#pragma unroll
      for (int r = 0; r < kRfRows; ++r) {
        if (r >= nb) continue;
        WrapQuad4 o = {nan, nan, nan, nan};
        if (rok[r]) {
          o = v[r];
          if (rlive[r] != all) {
#pragma unroll
            for (int x = 0; x < 4; ++x) o[x] = rf_slot_value(o[x], rlive[r], sl[x], keep);
          }
        }
        *reinterpret_cast<WrapQuad*>(obs_out + (size_t)(b0 + r) * W + c) = o;
      }
    }
  } else {
    // W < 4: nb W <= 12 elements, one per lane; every lane takes part in the shuffles
    const int r = min(l / W, nb - 1), c = l - (l / W) * W;
    const int okr = __shfl((int)ok, r);
    const unsigned long long ro = __shfl(off, r);
    const uint32_t lv = __shfl(live, r);
    if (l < nb * W) {
      float o = nan;
      if (okr) o = rf_slot_value(src[(size_t)ro + c], lv, c / D, keep);
      obs_out[(size_t)(b0 + r) * W + c] = o;
    }
  }
}
