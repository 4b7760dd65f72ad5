// usv_reset_kernel.hpp -- the explicit (host-requested) reset of masked envs; it rescans, so it follows the lidar.
#pragma once

#include "usv_reset.hpp"
#include "usv_lidar.hpp"
#include "usv_scan_step.hpp"

namespace usv {

// --------------------------------------------------------------------------- reset kernel
// Explicit (host-requested) reset of masked envs.  Reset obs = new header + the stale
// sensor_data: the scan at the last stepped pose (recomputed when that pose is still the
// current one, else the stored one; zeros for a never-stepped env), simple_env.py:302.
// scan_valid == 2: the last step was a scan-free one (ignore_obstacles), its scan is all max range.
template <typename R, int MODE>
__global__ __launch_bounds__(kBlock) void reset_kernel(State<R> S, IO<R> io) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  auto* rayoff = reinterpret_cast<typename Vec2<R>::T*>(lds);
  auto* slots = reinterpret_cast<unsigned long long*>(lds + lds_rayoff_bytes<R>());
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);   // wave-uniform (SGPR)
  const int l = lane_id();
  const int e0 = blockIdx.x * kEPBReset;
  const int ne = S.N - e0 < kEPBReset ? S.N - e0 : kEPBReset;
  int* marks = reinterpret_cast<int*>(lds + lds_rayoff_bytes<R>() + kLdsSlotBytes);
  // one obstacle row per wave (SoA) in the obstacle area
  R* wx = reinterpret_cast<R*>(lds + lds_head_bytes<R>()) + wave * 3 * 64;
  R* wy = wx + 64;
  R* wr = wy + 64;
  lds_prologue(S, lds, tid);
  __syncthreads();
  for (int k = wave; k < ne; k += kWaves) {
    const int e = e0 + k;
    if (io.mask && !io.mask[e]) continue;
    R rd0, rd1;
    R* last = S.sensor_last + (size_t)e * kSensors;
    const int valid = uniform(S.I(I_SCAN)[e]);
    if (valid == 2) {
      // the last step ignored the obstacles (noscan_step_kernel): 128 readings of 100 (:222-224)
      rd0 = rd1 = R(kSensorMax);
      last[l] = rd0;
      last[64 + l] = rd1;
    } else if (valid) {
      R sp, cp;
      heading_sincos(S.F(F_PSI)[e], &sp, &cp);
      const int n = uniform(S.I(I_NOBS)[e]);
      if (l < S.cap) {
        const R* o = S.orow(e);
        wx[l] = o[l]; wy[l] = o[S.ostride + l]; wr[l] = o[2 * S.ostride + l];
      }
      Scan<R> sc;
      lidar_wave<R, kLidDefault>(RowSoA<R>{wx, wy, wr}, n, S.F(F_X)[e], S.F(F_Y)[e], sp, cp, rayoff,
                                 slots + wave * 128, marks + wave * 64, sc);
      rd0 = sc.rd0;
      rd1 = sc.rd1;
      last[l] = rd0;
      last[64 + l] = rd1;
    } else {
      rd0 = last[l];
      rd1 = last[64 + l];
    }
    float* row = io.obs + (size_t)e * kObsDim;
    row[kHdr + l] = (float)l_norm(rd0);
    row[kHdr + 64 + l] = (float)l_norm(rd1);
    R* info = io.info ? io.info + (size_t)e * USV_INFO_DIM : nullptr;
    if (S.np_reset) {
      if (l == 0) np_reset<R, MODE>(S, e, row, info, io.kpath);
    } else {
      const int ep = uniform(S.I(I_EPISODE)[e]);
      reset_wave<R, MODE>(S, e, row, info, io.kpath);
      if (S.exp) {
        __threadfence_block();                 // the wave's reset stores land before lane 0 rewrites
        if (l == 0) reset_experiment<R>(S, e, ep, row, info);
      }
    }
  }
}

}  // namespace usv
