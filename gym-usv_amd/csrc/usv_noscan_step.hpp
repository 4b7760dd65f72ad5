// usv_noscan_step.hpp -- the scan-free step of usv-simple / usv-asmc-simple with ignore_obstacles set
// (simple_env.py:49): every lidar reading is the maximum range (:222-224), the reward has no collision
// term (:155) and no env terminates on an obstacle (:334).  Launched instead of the installed step
// variant while the handle's switch is on (usv_set_ignore_obstacles).
#pragma once

#include "usv_reset.hpp"
#include "usv_dynamics.hpp"
#include "usv_queue_step.hpp"

namespace usv {

// Without the scan a step is the lane-per-env dynamics (~100 B of state traffic per env) and one
// 572-B obs row per env whose 128 sensor entries are the constant 100 / 100 = 1.0f: a streaming
// store.  256-thread blocks; each wave owns 64 consecutive envs and shares nothing with the other
// waves of its block (no block barrier).
//   phase A  lane l runs env_dynamics of env e0 + l (the code of the scanning kernels, unchanged) and
//            stores reward (= the partial reward), terminated (0), truncated and the done mask; its 15
//            header floats go to the wave's LDS slice.
//   phase B  the wave's 64 obs rows are one contiguous span of 64 x 572 = 36 608 B, a multiple of 16,
//            so the span starts 16-B aligned whenever obs_dev is: the wave streams it with full-width
//            write-through 16-B stores (36 instructions of 1 KiB), each dword the staged header value
//            or 1.0f by its index mod 143.  A base that is not 16-B aligned takes dword stores (256 B
//            per instruction); a ragged last wave (N not a multiple of 64) ends its span with up to
//            three dword stores.
//   rare     a truncated env's final_obs row, and with same-step autoreset its stale scan
//            (sensor_last = 100) and the reset, which writes the header of the returned row.
// Stale scan: the step leaves scan_valid (I_SCAN) = 2, "the stale scan is all max range", where the
// scanning step leaves 1; no sensor_last row is written per step.  reset_kernel turns 2 into 128
// readings of 100, so toggling the switch at run time is exact: the stale scan follows the mode of the
// last step taken.
//
// Store ordering.  Every store to env e's state, to its obs row and to its reset state is issued by
// one wave, the one that owns e: phase A (lane e - e0: the state, then I_SCAN = 2), phase B (the row),
// then the rare path (sensor_last, the reset's state, I_SCAN = 0 and the row's header).  A wave's
// stores to one address complete in the order it issued them, and no other wave of this launch writes
// those addresses (a wave's span holds its own 64 rows and nothing else, aligned or not), so the
// reset cannot be overtaken: neither its state by phase A's, nor its header by phase B's.  With
// CHAIN = false the ASMC chain's stores (asmc_chain_kernel) are ordered by the kernel boundary; the
// NumPy-exact and custom-experiment resets run in their own launches after this one.

typedef float NoscanQuad __attribute__((ext_vector_type(4)));

// 16-B obs store, write-through like st_obs (sc1).  The compiler has no atomic store of this width;
// the trailing nop covers the wait states between a store of more than 8 B and a VALU write of its
// data registers, which the hazard recognizer cannot see inside an asm.  No memory clobber: the data
// are register operands, volatile asms keep their order, and the kernel closes phase B with a
// compiler barrier.
__device__ __forceinline__ void st_obs4(float* p, NoscanQuad v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v));
}

// The kernel's arguments re-read from the kernarg segment where a rare path begins (q_cold_args, for
// either precision): what the rare path derives from them is then computed inside it.
template <typename R> struct NoscanColdArgs { State<R> S; IO<R> io; };
static_assert(sizeof(State<double>) % alignof(IO<double>) == 0, "IO follows State in the kernarg segment");
template <typename R>
__device__ __forceinline__ NoscanColdArgs<R> noscan_cold_args() {
  typedef const __attribute__((address_space(4))) NoscanColdArgs<R>* KArg;
  KArg ka = (KArg)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka));
  NoscanColdArgs<R> c;
  __builtin_memcpy(&c, ka, sizeof(c));
  return c;
}

// CHAIN = false (usv-asmc-simple): asmc_chain_kernel already ran the two UsvAsmc.compute calls.
// DONE / INFO: also write the done mask / the info rows (template switches, as in step_q_body).
template <typename R, int MODE, bool CHAIN, bool DONE, bool INFO>
__global__ __launch_bounds__(kBlock) void noscan_step_kernel(State<R> S, IO<R> io) {
  // per wave: 64 headers at stride 15 (odd: no bank conflict), and a tail that phase B's unused
  // reads may touch (value(), below)
  __shared__ float hdr_lds[kWaves][kWave * kHdr + 128];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int e0 = (blockIdx.x * kWaves + wave) * kWave;  // this wave's envs: e0 .. e0 + ne - 1
  const int ne = min(kWave, S.N - e0);
  if (ne <= 0) return;
  float* const hs = hdr_lds[wave];
  bool trunc = false;
  // ---- phase A
  if (l < ne) {
    const int e = e0 + l;
    const float2 a = reinterpret_cast<const float2*>(io.act)[e];
    float hdr[kHdr];
    R px, py, sp, cp, partial;
    env_dynamics<R, MODE, CHAIN>(S, e, a.x, a.y, hdr, px, py, sp, cp, partial, trunc,
                                 INFO ? io.info + (size_t)e * USV_INFO_DIM : nullptr);
    S.I(I_SCAN)[e] = 2;                                 // after env_dynamics' 1, same lane: the stale scan is all max range
#pragma unroll
    for (int i = 0; i < kHdr; ++i) hs[l * kHdr + i] = hdr[i];
    st_out(io.rew + e, partial);                        // :155 no collision term
    io.term[e] = 0;                                     // :334
    io.trunc[e] = trunc;
    if constexpr (DONE) io.done[e] = trunc;
  }
  // the wave's headers are in LDS (a wave's LDS operations execute in order; nothing is shared
  // with another wave)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // ---- phase B
  float* const span = io.obs + (size_t)e0 * kObsDim;
  const int nd = ne * kObsDim;                          // dwords of the span
  // Entry t of env k's row, for t up to 145, i.e. running on into the header of env k + 1: as
  // 143 = 128 + 15, header entry t (t < 15) of env k and entry t - 143 of env k + 1 are both
  // hs[15 k + (t & 127)].  The load is unconditional (a select, not a branch); for a sensor entry it
  // reads some word of the slice or of its 128-word tail, and the value is not used.
  auto value = [&](int k, int t) {
    const float h = hs[k * kHdr + (t & 127)];
    return (unsigned)(t - kHdr) >= 128u ? h : 1.0f;     // sensors: 100 / 100 (:222-224, :82-83)
  };
  if ((reinterpret_cast<uintptr_t>(io.obs) & 15) == 0) {
    // lane l's quads are the dwords d = 4 l + 256 i: their env k and row entry c advance by
    // 256 = 143 + 113 dwords per iteration, so one division per lane serves the whole span
    int d = 4 * l;
    int k = d / kObsDim, c = d - k * kObsDim;
    for (; d + 3 < nd; d += 4 * kWave) {
      NoscanQuad v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = value(k, c + j);
      st_obs4(span + d, v);
      c += 4 * kWave - kObsDim;
      ++k;
      if (c >= kObsDim) { c -= kObsDim; ++k; }
    }
    const int dt = (nd & ~3) + l;                       // ragged wave: the span's last nd mod 4 dwords
    if (dt < nd) st_obs(span + dt, value(dt / kObsDim, dt % kObsDim));
  } else {
    int k = 0, c = l;                                   // dwords d = l + 64 i (l < 143)
    for (int d = l; d < nd; d += kWave) {
      st_obs(span + d, value(k, c));
      c += kWave;
      if (c >= kObsDim) { c -= kObsDim; ++k; }
    }
  }
  asm volatile("" ::: "memory");                        // the rare path's stores stay behind phase B's
  // ---- rare: truncated envs (terminal obs, stale scan, same-step reset)
  unsigned long long dm = ballot(trunc);
  if (__builtin_expect_with_probability(dm != 0ull, 0, kQRare)) {
    const NoscanColdArgs<R> c = noscan_cold_args<R>();
    for (; dm; dm &= dm - 1) {
      const int k = __builtin_ctzll(dm);
      const int e = e0 + k;
      float* const row = c.io.obs + (size_t)e * kObsDim;
      if (c.io.fobs) {
        float* const f = c.io.fobs + (size_t)e * kObsDim;
        f[kHdr + l] = 1.0f;
        f[kHdr + 64 + l] = 1.0f;
        if (l < kHdr) f[l] = hs[k * kHdr + l];
      }
      if (c.S.autoreset == USV_AUTORESET_SAME_STEP) {
        // the returned row keeps its sensors (1.0): the stale scan of the new episode
        c.S.sensor_last[(size_t)e * kSensors + l] = R(kSensorMax);
        c.S.sensor_last[(size_t)e * kSensors + 64 + l] = R(kSensorMax);
        reset_wave<R, MODE>(c.S, e, row);               // Philox; the NumPy-exact reset follows in its own launch
      }
    }
  }
}

}  // namespace usv
