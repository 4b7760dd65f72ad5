// usv_variant.hpp -- the step-kernel variants of usv-simple / usv-asmc-simple in one place: their
// kinds, the block shapes and lidar bits the rules need, the default of a configuration
// (default_variant) and what usv_set_kernel_variant may select for it (variant_allowed).  All
// variants give bit-identical results.  Plain host C++17 (no HIP), so the rules are tested on
// their own (tests/test_step_variants.py); the device headers take the constants from here.
#pragma once

#include <stdint.h>

#include "usv_hip.h"

namespace usv {

// The values are those of usv_set_kernel_variant's `kind` and of the "epb,lid,kind" strings.
enum StepKind : int {
  kWaveFused = 1,    // step_kernel_wave: dynamics + wave-per-env scan in one launch
  kWaveSplit = 2,    // dyn_kernel, then scan_kernel
  kBlockDyn = 3,     // step_kernel_blockdyn: wave 0 runs the block's dynamics at full width (f64 usv-simple)
  kQueueSplit = 4,   // dyn_rec_kernel, then the block-queue step_q_kernel
  kQueueFused = 5,   // the block-queue step with the dynamics in its phase 1
  kQueueChain = 6,   // usv-asmc-simple: asmc_chain_kernel, then the fused block-queue step without the chain
};
// the block-queue step (f32, window lidar, cap <= 32); the others split the envs statically over waves
constexpr bool is_queue(int kind) { return kind == kQueueSplit || kind == kQueueFused || kind == kQueueChain; }

constexpr bool is_legacy(int mode) {   // lane-per-env legacy envs: obs 6, scalar action, no lidar, one kernel
  return mode == USV_MODE_ASMC_V0 || mode == USV_MODE_ASMC_YE_INT_V0 || mode == USV_MODE_PID_V0;
}

// Lidar variants (compile-time): bit 0 = drop obstacles wholly inside the rear blind sector
// before the ray loop, bit 1 = obstacle loop unrolled by two, bit 2 = angular-window pair
// expansion (f32: lidar_window / lidar_window2; f64: lidar_window_d).  The max-range test of :458 runs only in waves with an
// obstacle >= 99 m away (wave-uniform template switch).
constexpr int kLidSkip = 1, kLidUnroll2 = 2, kLidWindow = 4;
constexpr int kLidBrute = kLidSkip | kLidUnroll2, kLidFull = kLidBrute | kLidWindow;   // the two defaults
// usv_set_kernel_variant's lid carries the block-queue step's row-store override above the lidar bits
constexpr int kLidMask = 0xff, kLidSpanOn = 0x100, kLidSpanOff = 0x200, kLidSpanBits = kLidSpanOn | kLidSpanOff;

// Block shapes of the block-queue step: kQE = 128 envs on kQW = 16 waves (two blocks per CU), and
// kQE_S = 16 envs on kQW_S = 8 waves for small env counts, where 128-env blocks would leave most CUs
// idle (4 096 envs are 32 such blocks) -- each wave then owns about one pair, and up to four blocks
// share a CU.  The split kind has the large shape only.
constexpr int kQW = 16, kQE = 128;
constexpr int kQE_S = 16, kQW_S = 8;
constexpr int kQSmallBelow = 32768;   // env count below which the small blocks are the default (tools/nsweep.sh)
// f64 wave scans: 16 envs per wave from this env count up (one round of waves at 65 536 envs), else 8
constexpr int kF64WideFrom = 49152;

// Obs-row store layout of the block-queue step (State::rowspan; usv_set_kernel_variant lid bits 0x100 /
// 0x200 force it on / off; a template switch, SPAN, of the 128-env fused kernels without info rows, as
// the two layouts' code together in the pair loop spilled SGPRs; the others store pieces): an env pair's two rows as one span of 32-B-aligned 256-B stores (round 4),
// or each row in pieces (the sensor halves, then both headers in one store).  The span writes
// 1.05x the algorithmic bytes (pieces: 1.18x, sectors split between write-through stores) and wins
// where the rows go to DRAM (524 288 envs: 183.4 -> 161.4 us per step); with the working set in the
// 256 MB Infinity Cache the pieces are faster (65 536 envs: 19.2 vs 20.3 us), so the default switches
// at kRowSpanFrom envs.
constexpr int kRowSpanFrom = 196608;
// issue-priority mode of the static-split kinds (State::prio: 1 ramp, 2 last iteration first, 0 none);
// block dynamics, f64 at 65 536 envs, same box: 1 -> 40.5 us, 0 -> 43.2, 2 -> 43.2.  The ramp helps
// static splits only: the block queue runs without.
constexpr int kStaticPrio = 1;

// What a handle runs: Handle's kind / epb / lid and State's prio / rowspan (apply_variant).
struct Variant {
  int kind;      // StepKind
  int epb;       // envs per block
  int lid;       // lidar bits
  int prio;      // State::prio
  int rowspan;   // State::rowspan
};

constexpr int variant_prio(int kind) { return is_queue(kind) ? 0 : kStaticPrio; }

// Tuned defaults at 65 536 envs on MI355X (tools/sweep_variants.py, profiles/).  With the window lidar
// and cap <= 32:
//   f32  the fused block-queue step, small blocks below kQSmallBelow envs; usv-asmc-simple runs the
//        ASMC chain in its own launch first, and the queue then has usv-simple's phase 1 (ASMC's 20
//        substeps want full-width dynamics; 45.7 us vs 46.7 for the split wave scan);
//   f64  usv-simple: one launch, wave 0 of each block runs the block's dynamics at full width, then the
//        two-env wave scan, 16 envs/wave from kF64WideFrom envs up (40.3 us, against 47.7 for the split
//        dyn_kernel + scan), else 8; usv-asmc-simple: the split wave scan at the same widths (72.0 us
//        against 77.4 at 4 envs/wave; block-wide dynamics spill the f64 ASMC state at 4 waves per
//        SIMD, 94 us).
// Otherwise usv-simple runs the fused wave kernel at 16 envs/wave and usv-asmc-simple the split wave
// scan at 4.  The legacy ids have one kernel and never launch a step variant.
inline Variant default_variant(const usv_config& c) {
  const bool asmc = c.mode == USV_MODE_ASMC_SIMPLE;
  const bool window32 = !is_legacy(c.mode) && c.lidar_algo == USV_LIDAR_WINDOW && c.obstacle_cap <= 32;
  Variant v{};
  if (window32 && c.precision == USV_F32) {
    v.kind = asmc ? kQueueChain : kQueueFused;
    v.epb = c.num_envs < kQSmallBelow ? kQE_S : kQE;
  } else if (window32 && c.precision == USV_F64) {
    v.kind = asmc ? kWaveSplit : kBlockDyn;
    v.epb = c.num_envs >= kF64WideFrom ? 64 : 32;
  } else {
    v.kind = asmc ? kWaveSplit : kWaveFused;
    v.epb = asmc ? 16 : 64;
  }
  v.lid = c.lidar_algo == USV_LIDAR_BRUTE ? kLidBrute : kLidFull;
  v.prio = variant_prio(v.kind);
  v.rowspan = c.num_envs >= kRowSpanFrom;
  return v;
}

// usv_set_kernel_variant's rules: `refused` is null and `v` the variant to install (lid without the
// row-store bits, rowspan with their override), or `refused` says why not.  cfg.lidar_algo is not
// consulted: every lidar variant gives the same scan.
struct VariantCheck {
  const char* refused;
  Variant v;
};
inline VariantCheck variant_allowed(const usv_config& c, int kind, int epb, int lid) {
  if (is_legacy(c.mode)) return {"the legacy ids have one lane-per-env kernel", {}};
  const int rs = lid & kLidSpanBits;
  lid &= kLidMask;
  if (rs == kLidSpanBits || (rs && !is_queue(kind))) return {"bad row-store bits", {}};
  const bool f64 = c.precision == USV_F64;
  const bool lid_ok = lid == 0 || lid == kLidBrute || lid == kLidFull;
  bool ok = false;
  switch (kind) {
    case kWaveFused:
      ok = (epb == 16 || epb == 32 || epb == 64) && lid_ok;
      break;
    case kWaveSplit:
      ok = (epb == 8 || epb == 16 || epb == 32 || (epb == 64 && lid == kLidFull && f64)) && lid_ok;
      break;
    case kBlockDyn:
      ok = (epb == 32 || epb == 64) && lid == kLidFull && f64 && c.mode == USV_MODE_SIMPLE;
      break;
    case kQueueSplit:
    case kQueueFused:
    case kQueueChain:
      ok = (kind != kQueueChain || c.mode == USV_MODE_ASMC_SIMPLE) &&
           (epb == kQE || (kind != kQueueSplit && epb == kQE_S)) && lid == kLidFull &&
           c.precision == USV_F32 && c.obstacle_cap <= 32;
      break;
  }
  if (!ok) return {"kernel variant not available for this config", {}};
  return {nullptr, {kind, epb, lid, variant_prio(kind), rs ? rs == kLidSpanOn : c.num_envs >= kRowSpanFrom}};
}

}  // namespace usv
