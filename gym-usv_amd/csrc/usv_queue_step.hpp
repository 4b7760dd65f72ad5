// usv_queue_step.hpp -- the block-queue step (StepKind queue split / queue fused / queue after the ASMC chain of
// usv_variant.hpp) with dyn_rec_kernel and asmc_chain_kernel.
#pragma once

#include "usv_scan_step.hpp"

namespace usv {

// ---- block-queue step (f32 window lidar, cap <= 32): 1024-thread blocks of 16 waves own
// kQE = 128 envs each; the block's env pairs are pulled from an LDS counter.  VALU issue on a
// SIMD is arbitrated by priority, then age, so with a static split the oldest waves finish first
// and the youngest run alone at the end; with the queue the favoured waves simply take more pairs
// and all of them finish together.
//   fused (usv-simple): waves 0 and 1 run the block's dynamics lane-per-env (full width) and
//                       leave one 64-B record per env in LDS;
//   split (usv-asmc-simple): dyn_rec_kernel ran first and left the records in S.qrec; they are
//                       DMA'd into LDS.
// Record (16 f32): pose (x, y, ray-0 direction c0, s0) | partial reward, n_obs | truncated << 16
// (int bits), then the non-constant obs-header values h0, h2..h9, h11 (make_header).  The obs
// header is stored together with the sensors when the env's pair is scanned, so each obs row is
// written once, late, and as a whole (no early header stores to lines that would be evicted
// before the sensors reach them).
// Each wave's first pair is static (pair = wave); its rows and the next pair's are DMA'd while
// the current pair is scanned (one DMA instruction per pair: two 384-B SoA rows).
// kQE = 128 envs on kQW = 16 waves per block-queue block, compiled for 8 waves per SIMD (kQWPE) in
// kQSgpr = 80 SGPRs
constexpr int kQSgpr = 80, kQWPE = 8;
// Issue priority in the block queue (round 5).  VALU issue on a SIMD goes by priority, then age, so a
// CU's older block (the first one dispatched to it) wins every tie against the younger one: in the
// round-4 timeline the older block ended at ~11.7 us and the younger ran alone, at 4 waves per SIMD,
// for its last ~6 us.  (1) The dynamics waves run phase 1 at priority 3 (the younger block's 14 other
// waves wait at its barrier for them while the older block scans), back to 0 after the barrier;
// (2) in a one-round grid (<= 2 blocks per CU) the second block of each CU (block index >= the CU
// count: blocks are dispatched one per CU first) raises kQYoungWaves of its 16 waves to priority 1,
// so the two blocks progress at more even rates.  Both only in a one-round grid (State::qyoung set):
// with more rounds (524 288 envs) the phase-1 priority cost 0.9 us of 161.  Same-box A/Bs (gpurun_out
// r5b-r5e): -0.27 to -0.67 us per launch at 65 536 envs (usv-simple), -0.95 us (usv-asmc-simple, whose
// q kernel has the same phase 1).
constexpr int kQPrioDyn = 3, kQYoungWaves = 10;
// (the block shapes kQE / kQW, kQE_S / kQW_S: usv_variant.hpp; the record's size kQRec: usv_layout.hpp)
__host__ __device__ constexpr size_t q_slice_bytes() { return 256 * 8 + 64 * 4 + 2 * 1024; }

// One DMA instruction (<= 64 pieces of 16 B, i.e. <= 1 KiB): pieces c >= nchunk are not copied.
// src is wave-uniform: SGPR base + a 32-bit lane offset (the saddr form), so no per-lane 64-bit
// address is kept live across the pair loop.
__device__ __forceinline__ void dma_copy1(const void* src, void* dst, int bytes) {
  const int c = lane_id();
  const unsigned d = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)dst);
  const uint64_t a = (uint64_t)(uintptr_t)src;
  // (readfirstlane returns int: widen through unsigned, or the low half would sign-extend)
  const uint64_t sb = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) << 32) |
                      (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)a);
  if (c < bytes / 16) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(16 * c), "s"(sb), "s"(d) : "memory");
  }
}

// dma_copy1 from a loop-invariant wave-uniform base (SGPR pair) at a wave-uniform byte offset `off`
// carried in the lanes' 32-bit offsets: the pair loop then computes no 64-bit row address per pair.
__device__ __forceinline__ void dma_copy_at(const void* base, int off, void* dst, int bytes) {
  const int c = lane_id();
  const unsigned d = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)dst);
  const uint64_t a = (uint64_t)(uintptr_t)base;
  const uint64_t sb = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) << 32) |
                      (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)a);
  if (c < bytes / 16) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(16 * c + off), "s"(sb), "s"(d) : "memory");
  }
}

__device__ __forceinline__ void make_qrec(float* rec, float px, float py, float sp, float cp, float partial,
                                          int n, bool trunc, const float (&h)[kHdr]) {
  const float c0 = ray_c(cp, sp, (float)kStartC, (float)kStartS), s0 = ray_s(cp, sp, (float)kStartC, (float)kStartS);
  float4* r4 = reinterpret_cast<float4*>(rec);
  r4[0] = make_float4(px, py, c0, s0);
  r4[1] = make_float4(partial, __int_as_float(n | (trunc ? 1 << 16 : 0)), h[0], h[2]);
  r4[2] = make_float4(h[3], h[4], h[5], h[6]);
  r4[3] = make_float4(h[7], h[8], h[9], h[11]);
}
// obs-header value i (0..14) of the env whose record is `rec` (make_header's layout: entries 1, 10,
// 13 are 0, entries 12, 14 the max_acceleration constants)
__device__ __forceinline__ float qrec_hdr(const float* rec, int i) {
  const float v = rec[i == 0 ? 6 : (i <= 9 ? i + 5 : 15)];
  return (i == 1 || i == 10 || i == 13) ? 0.0f
       : i == 12 ? (float)(kMaxAccU / 10.0) : i == 14 ? (float)(kMaxAccR / 10.0) : v;
}

// Terminal obs and stale scan of a done env e (rare path; lane l holds its rays l, l + 64).
// `rot`: the scan is rotated across lanes (lane l holds rays (l - rot) & 63 and 64 + that).
__device__ __forceinline__ void q_emit_done(const State<float>& S, const IO<float>& io, int e,
                                            const Scan<float>& sc, const float* rec, int rot) {
  const int l = lane_id();
  const int ray = (l - rot) & (kWave - 1);
  if (io.fobs) {
    float* f = io.fobs + (size_t)e * kObsDim;
    f[kHdr + ray] = l_norm(sc.rd0);
    f[kHdr + 64 + ray] = l_norm(sc.rd1);
    const int hi = min(l, kHdr - 1);
    f[hi] = qrec_hdr(rec, hi);
  }
  if (S.autoreset == USV_AUTORESET_SAME_STEP) {
    S.sensor_last[(size_t)e * kSensors + ray] = sc.rd0;
    S.sensor_last[(size_t)e * kSensors + 64 + ray] = sc.rd1;
  }
}

// The kernel's arguments for its rare paths (a done env's terminal obs, a same-step reset), re-read
// from the kernarg segment where such a path begins.  The pointer passes through an empty asm, so
// the compiler cannot tell the copy from a fresh load: what the rare path derives from State / IO
// (the Philox key schedule, every field's base pointer, fobs, sensor_last) is then computed inside
// it, not hoisted ahead of the pair loop and carried through it in registers ("Cold
// paths").  Scalar loads: they count on lgkmcnt and wait for no store.  For kernels whose
// parameters are exactly (State<float>, IO<float>).
constexpr double kQRare = 1.0 - 1e-6;   // branch weight of the pair loop's rare paths
struct QColdArgs { State<float> S; IO<float> io; };
static_assert(sizeof(State<float>) % alignof(IO<float>) == 0, "IO follows State in the kernarg segment");
__device__ __forceinline__ QColdArgs q_cold_args() {
  typedef const __attribute__((address_space(4))) QColdArgs* KArg;   // (typed: 8-B aligned scalar loads)
  KArg ka = (KArg)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka));
  QColdArgs c;
  __builtin_memcpy(&c, ka, sizeof(c));
  return c;
}

template <int QE = kQE, int QW = kQW> __host__ __device__ constexpr size_t lds_q_bytes() {
  return wave_tab_bytes<float>() + QW * q_slice_bytes() + QE * kQRec * 4 + 16 + 2 * QE * 4;   // + n_obs[QE], episode[QE]
}
static_assert(2 * lds_q_bytes() <= 160 * 1024, "two blocks per CU");
static_assert(4 * lds_q_bytes<kQE_S, kQW_S>() <= 160 * 1024, "four small blocks per CU");

// DONE: also write the done mask (io.done, ABI v4).  A template switch rather than a runtime test:
// the raw step (usv_step, io.done null) then carries neither the pointer nor its branch in the pair
// loop, whose SGPR budget is at its limit (a runtime test cost 0.25 us per launch).
// CHAIN = false (usv-asmc-simple, FUSED): asmc_chain_kernel ran the ASMC chain, phase 1 the rest.
// INFO (fused): phase 1 writes the per-step info rows (usv_step_ex with info_dev); a template switch
// like DONE: the info path's registers would otherwise make phase 1 spill, and the spill's reload
// wait for every store the dynamics issued before the barrier.
template <int MODE, bool FUSED, bool DONE = false, int kQE = ::usv::kQE, int kQW = ::usv::kQW, bool CHAIN = true,
          bool INFO = false, bool SPAN = false>
__device__ __forceinline__ void step_q_body(const State<float>& S, const IO<float>& io) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  constexpr int os = 32, rowb = row_bytes<float>(32);  // cap in [29, 32]: plane stride 32, 384-B rows
  const int eb = blockIdx.x * kQE;                     // this block's envs: eb .. eb + nbe - 1
  const int nbe = min(kQE, S.N - eb);
  const int np = (nbe + 1) >> 1;                       // and pairs 0 .. np - 1 (block-local)
  char* const slice = lds + wave_tab_bytes<float>() + wave * q_slice_bytes();
  unsigned long long* const slot = reinterpret_cast<unsigned long long*>(slice);
  int* const mark = reinterpret_cast<int*>(slice + 256 * 8);
  float* const rowbuf0 = reinterpret_cast<float*>(slice + 256 * 8 + 64 * 4);
  float* const rowbuf1 = rowbuf0 + 256;
  float* const recs = reinterpret_cast<float*>(lds + wave_tab_bytes<float>() + kQW * q_slice_bytes());
  unsigned* const qctr = reinterpret_cast<unsigned*>(recs + kQE * kQRec);
  int* const qnob = reinterpret_cast<int*>(recs + kQE * kQRec) + 4;   // fused: the block's n_obs
  int* const qep = qnob + kQE;                                        // the block's episode counters
  const float2* const rayoff = reinterpret_cast<const float2*>(lds);
#ifdef USV_DIAG_QPROF
  QProf qprof;
  QProf* const qp = &qprof;
#else
  QProf* const qp = nullptr;
#endif
  // qctr[1 + w]: dynamics wave w's state stores are acknowledged (set after the barrier, below; a
  // wave that same-step-resets one of wave w's envs waits for it, so its reset stores cannot be
  // overtaken by them)
  unsigned* const qdyn = qctr + 1;
  if (threadIdx.x == 0) {
    qctr[0] = kQW;                                     // pairs 0 .. kQW-1 are the static first ones
    qdyn[0] = 0u;
    qdyn[1] = 0u;
  }

  // the ray table: by the last wave, so that the dynamics waves (fused) issue no DMA of their own
  if (wave == kQW - 1) dma_copy(S.ray_tab, lds, (int)wave_tab_bytes<float>());
#pragma unroll
  for (int i = 0; i < 4; ++i) slot[i * 64 + l] = kSlotArm;
  mark[l] = 0;                                         // lidar_window2 clears them after each call
  USV_STAMP_W(0);
  USV_STAMP_ID();
  int cur = wave < np ? wave : -1;
  // first (static) pairs: pair w's rows into wave w's buffer 0.  With the fused dynamics, waves 2 and 3
  // also issue those of waves 0 and 1, whose state loads would otherwise queue behind their own DMA
  // (a wave's loads return in issue order); the barrier below publishes them.
  constexpr int kDynWaves = FUSED ? (kQE + kWave - 1) / kWave : 0;
  static_assert(kQW >= 3 * kDynWaves + 1 && 2 * kQW <= kQE + 2 * kWave, "block shape");
  // the store flags qdyn[0..kDynWaves-1] live in the 16-B qctr words (lds_q_bytes), before qnob
  static_assert(kDynWaves <= 2, "qdyn holds two dynamics waves' flags");
  if (wave >= kDynWaves && cur >= 0) dma_copy1(S.orow(eb + 2 * cur), rowbuf0, min(2, nbe - 2 * cur) * rowb);
  if (FUSED && wave >= kDynWaves && wave < 2 * kDynWaves) {
    const int w = wave - kDynWaves;
    if (w < np)
      dma_copy1(S.orow(eb + 2 * w), lds + wave_tab_bytes<float>() + w * q_slice_bytes() + 256 * 8 + 64 * 4,
                min(2, nbe - 2 * w) * rowb);
  }
  {
    // the block's obstacle counts (fused) and episode counters into LDS, one env per lane.  Fused: by
    // waves 2 kDynWaves .. 3 kDynWaves - 1, so the dynamics waves load nothing after their stores: a
    // load issued after them would make the wave wait for every store's ack (one vmcnt counter)
    // before the barrier.  Split: by the waves below the ray table's, which copy no records.
    // The episode counters are for the same-step resets after the pair loop: an env is reset at most
    // once per launch, so the staged counter is its current one, and the reset starts with no load
    // queued behind its wave's stores.
    constexpr int kStageWaves = (kQE + kWave - 1) / kWave;
    constexpr int kStage0 = FUSED ? 2 * kDynWaves : kQW - 1 - kStageWaves;
    static_assert(kStage0 >= kDynWaves && kStage0 + kStageWaves <= kQW, "staging waves");
    if (wave >= kStage0 && wave < kStage0 + kStageWaves) {
      const int k = (wave - kStage0) * kWave + l;
      if (k < nbe) {
        if constexpr (FUSED) qnob[k] = S.I(I_NOBS)[eb + k];
        qep[k] = S.I(I_EPISODE)[eb + k];
      }
    }
  }
  if constexpr (FUSED) {
    // dynamics, one lane per env.  Lanes past the end repeat the wave's last env (same wave:
    // every lane loads the state before any lane stores it); a wave with no env of its own must
    // not run, or two waves would race on the same env's state
    if (wave < kDynWaves && wave * kWave < nbe) {
      if (S.qyoung != INT_MAX) __builtin_amdgcn_s_setprio(kQPrioDyn);
      const int k = min(wave * kWave + l, nbe - 1);
      const int e = eb + k;
      const float2 a = reinterpret_cast<const float2*>(io.act)[e];
      float hdr[kHdr];
      float px, py, sp, cp, partial;
      bool trunc;
      env_dynamics<float, MODE, CHAIN>(S, e, a.x, a.y, hdr, px, py, sp, cp, partial, trunc,
                                       INFO ? io.info + (size_t)e * USV_INFO_DIM : nullptr);
      io.trunc[e] = trunc;
      make_qrec(recs + k * kQRec, px, py, sp, cp, partial, 0, trunc, hdr);   // (n_obs: qnob)
    }
  } else {
    if (wave < kQE / 16 && wave * 16 < nbe)            // 16 records (1 KiB) per wave
      dma_copy1(S.qrec + (size_t)(eb + wave * 16) * kQRec, recs + wave * 16 * kQRec, min(16, nbe - wave * 16) * kQRec * 4);
  }
  // rows, ray table and records landed (the dynamics waves issued no DMA: their stores drain later,
  // ahead of their first pair's rows in the vmcnt order)
  // Per-lane and per-block invariants of the pair loop that do not depend on phase 1, computed (and
  // pinned: the compiler otherwise sinks them to the loop's preheader) ahead of the barrier by the
  // waves that only wait there; the dynamics waves, which the barrier waits for, do it after it.
  // hpk: the per-row layout's obs-header lanes (SPAN = false), loop-invariant, packed in one register
  // (a second one is one too many for the dynamics waves, which carry it through phase 1):
  // lanes 0..14 store env A's header value hi, 15..29 env B's, 30..63 repeat lane 29.  Bits 0..9: the
  // lane's byte offset from env A's obs row (value hi of its row, env B's lanes one row on); bits
  // 10..13: the record slot of value hi (qrec_hdr), bits 14 and 16: env B's lane (so bits 10..14 index
  // the value from env A's record, kQRec = 16 floats per record); bit 17: a constant entry (1, 10, 12-14).
  // oblk: this block's obstacle rows (pair p at 2 p rowb bytes).  ob: see pair_shift below.
  int hpk = 0;
  const float* oblk = nullptr;
  unsigned ob = 0;
  auto loop_setup = [&] {
    if constexpr (!SPAN) {
      const int hl = min(l, 2 * kHdr - 1);
      const int hi = hl >= kHdr ? hl - kHdr : hl;
      const int hrec = hi == 0 ? 6 : (hi <= 9 ? hi + 5 : 15);
      static_assert(kQRec == 16 && 4 * (kHdr + kObsDim) < 1024, "hpk fields");
      hpk = 4 * (hi + (hl >= kHdr ? kObsDim : 0)) | (hrec << 10) | ((hl >= kHdr) << 14) | ((hl >= kHdr) << 16) |
            ((hi == 1 || hi == 10 || hi >= 12) << 17);
      asm volatile("" : "+v"(hpk));
    }
    oblk = S.orow(eb);
    ob = (unsigned)(((uintptr_t)io.obs >> 2) & 7);
    asm volatile("" : "+s"(oblk), "+s"(ob));
  };
  if (wave >= kDynWaves) loop_setup();
  USV_STAMP_W(1);
  if (wave >= kDynWaves) vm_wait<0>();
  QMARK(10);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (FUSED && wave < kDynWaves) __builtin_amdgcn_s_setprio(0);
  if ((int)blockIdx.x >= S.qyoung && wave < kQYoungWaves) __builtin_amdgcn_s_setprio(1);
  // Same-step reset ordering: a dynamics wave stored its envs' state in phase 1, and
  // another wave may reset one of those envs later in this launch; two waves' stores to one address
  // are ordered only if the first is acknowledged before the second is issued.  So each dynamics
  // wave drains its stores here, after the barrier (its first pair's rows are already in LDS, and
  // env_dynamics issues the state stores as soon as the new state exists, so little is left to
  // wait for), and sets its flag; a reset of one of its envs waits for the flag.  Measured against
  // no ordering at all: +0.1 us at 65 536 envs, +0.15 us at 524 288 (a per-pair flag in the loop
  // cost 0.5 / 1.8 us, draining before the barrier 0.05 / 1.6 us; gpurun_out r5h, r5i).
  if (FUSED && wave < kDynWaves) {
    vm_wait<0>();
    __hip_atomic_store(qdyn + wave, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    loop_setup();
  }
  USV_STAMP_W(2);
  QMARK(0);
  unsigned tk = 0;
  if (l == 0) tk = atomicAdd(qctr, 1u);                 // LDS ticket of this wave's second pair
  // same-step autoresets of a pair run outside the pair loop (the loop is left and re-entered):
  // inside it their registers would spill the loop's to scratch
  int it = 0;
#ifdef USV_DIAG_STAMPS
  unsigned wsum = 0;                                   // (diagnostic: window sizes of this wave's pairs)
#endif
  const bool hb = l >= 32;
  // FULL (D): every pair of the block has its env B (nbe is even), so `hasB` is the constant true and
  // the lone-env selects fold away; the only block of a launch with an odd nbe runs the general body.
  auto pair_hasb = [&](auto full, int p) __attribute__((always_inline)) { return decltype(full)::value || 2 * p + 1 < nbe; };

  // An env pair's two obs rows are one 1144-B span, stored as five 256-B wave stores from the span's
  // first 32-B sector: every sector but the two at the span's ends is written whole by one write-through
  // store (the four sensor halves and the header store of round 3 split ~3 sectors per row between
  // instructions, 1.18x the algorithmic write bytes).  sh = the span's dword offset in its sector.
  auto pair_shift = [&](int p) { return (int)((ob + (unsigned)(eb + 2 * p) * (unsigned)kObsDim) & 7u); };
  // env record of pair c for this lane (lanes 0..31 env A, 32..63 env B; env A again when there is
  // no B): pose, meta and the obs-header value this lane stores (lanes sh..sh+14: env A's entries
  // 0..14, sh+15..sh+29: env B's; no env B: sh = 0 and lanes 15..29 repeat env A's).  Read one pair
  // ahead (after the current pair's scan), so the LDS latency overlaps the current pair's stores.
  auto rec_of = [&](auto full, int c, float4& P, float4& M, float& H) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full)::value;
    const int c0 = 2 * c;
    const bool cB = pair_hasb(full, c);
    const int kk = FULL ? c0 + (int)((unsigned)l >> 5) : ((hb && cB) ? c0 + 1 : c0);
    const float* const rk = recs + kk * kQRec;
    P = *reinterpret_cast<const float4*>(rk);
    M = *reinterpret_cast<const float4*>(rk + 4);
    if constexpr (FUSED) M.y = __int_as_float(__float_as_int(M.y) | qnob[kk]);   // n_obs | truncated << 16
    if constexpr (!SPAN) {                             // (the constant entries are selected at the store)
      // (FULL: bits 10..14 of hpk index env B's lanes' values one record on)
      H = FULL ? recs[c0 * kQRec + ((hpk >> 10) & 31)]
               : recs[((((hpk >> 16) & 1) && cB) ? c0 + 1 : c0) * kQRec + ((hpk >> 10) & 15)];
      return;
    }
    const int hl = min(max(l - ((SPAN && cB) ? pair_shift(c) : 0), 0), 2 * kHdr - 1);
    const int hi = hl >= kHdr ? hl - kHdr : hl;
    float v = recs[((hl >= kHdr && cB) ? c0 + 1 : c0) * kQRec + (hi == 0 ? 6 : (hi <= 9 ? hi + 5 : 15))];
    // make_header's constant entries 1, 10, 13 (0) and 12, 14 (max_acceleration / 10), as selects:
    // written as one conditional chain the compiler branches on exec around the record read
    const bool cst = ((0x7402 >> hi) & 1) != 0;
    const float hc = hi == 12 ? (float)(kMaxAccU / 10.0) : (hi == 14 ? (float)(kMaxAccR / 10.0) : 0.0f);
    asm volatile("" : "+v"(v));
    H = cst ? hc : v;
  };
  // The pair loop with its same-step resets, in two instantiations: the block runs one of them.
  // (One lambda around both loops rather than around the loop body alone: each copy then keeps the
  // original's shape, one flat loop, and only its own loop invariants live across the reset path.)
  auto run_pairs = [&](auto full) __attribute__((always_inline)) {
  // The block's first obs row, reward and flags.  Every store of the pair loop is one of these
  // wave-uniform bases plus a 32-bit lane offset that includes the pair's offset in the block
  // (at_bytes).  Computed here, not with loop_setup's values: ahead of phase 1 they cost it registers,
  // and a pointer pinned by an asm has lost its address space (its stores would be flat ones).
  float* const bobs = io.obs + (size_t)eb * kObsDim;
  float* const brew = io.rew + eb;
  uint8_t* const bterm = io.term + eb;
  [[maybe_unused]] uint8_t* const bdone = DONE ? io.done + eb : nullptr;
  for (;;) {
    unsigned done = 0;
    int de0 = 0;
    float4 pose = make_float4(0.f, 0.f, 0.f, 0.f), meta = pose;
    float hv = 0.0f;
    if (cur >= 0) rec_of(full, cur, pose, meta, hv);
    while (cur >= 0) {
      int nxt = (int)__builtin_amdgcn_readlane(tk, 0);
      QCOUNT(8, 1);
      const bool odd = (it & 1) != 0;
      float* const cbuf = odd ? rowbuf1 : rowbuf0;
      float* const nbuf = odd ? rowbuf0 : rowbuf1;
      const int k0 = 2 * cur;
      const int e0 = eb + k0;
      const bool hasB = pair_hasb(full, cur);
      if (nxt >= np) nxt = -1;
      if (nxt >= 0) {                                  // wave-uniform
        if (l == 0) tk = atomicAdd(qctr, 1u);
        dma_copy_at(oblk, 2 * rowb * nxt, nbuf, (pair_hasb(full, nxt) ? 2 : 1) * rowb);
      }
      // this lane's env in the block: lanes 0..31 env A, 32..63 env B (env A again when there is no B);
      // the element of the reward / flag stores (kept in 32 bits: a select would be widened into a
      // 64-bit address operand)
      const unsigned kl = (unsigned)k0 + (((unsigned)l >> 5) & (hasB ? 1u : 0u));
      const int nt = __float_as_int(meta.y);
      // the pair's span offset and the lane rotations of the two scans that put each reading in the
      // lane that stores it (no env B: the rows are stored as in round 3, unrotated)
      const bool span2 = SPAN && hasB;
      const int sh = span2 ? pair_shift(cur) : 0;
      const int rotA = span2 ? kHdr + sh : 0, rotB = span2 ? 2 * kHdr + sh : 0;
      Scan<float> sa, sb;
      QMARK(1);
#ifdef USV_DIAG_STAMPS
      int wq = 0;
      lidar_wave2(cbuf, os, (hb && !hasB) ? 0 : (nt & 0xffff), pose.x, pose.y, pose.z, pose.w, rayoff, slot,
                  mark, reinterpret_cast<int*>(nbuf) + 192, sa, sb, qp, rotA, rotB, &wq);
      wsum += (unsigned)wq;
#else
      lidar_wave2(cbuf, os, (hb && !hasB) ? 0 : (nt & 0xffff), pose.x, pose.y, pose.z, pose.w, rayoff, slot,
                  mark, reinterpret_cast<int*>(nbuf) + 192, sa, sb, qp, rotA, rotB);
#endif
      float4 pose_n = pose, meta_n = meta;
      float hv_n = hv;
      if (nxt >= 0) rec_of(full, nxt, pose_n, meta_n, hv_n);   // the next pair's record (wave-uniform)
      // collision (:153-156): two compares and ballots per env (a fminf of the two readings would
      // canonicalise both first); "any lane" is tested on the scalar unit (ballot_halves)
      const float kc = (float)kCollDist;
      const BallotHalves ca = ballot_halves(ballot(sa.rd0 < kc) | ballot(sa.rd1 < kc));
      const BallotHalves cb = ballot_halves(ballot(sb.rd0 < kc) | ballot(sb.rd1 < kc));
      const bool collA = (ca.lo | ca.hi) != 0u;
      const bool collB = hasB ? (cb.lo | cb.hi) != 0u : collA;
      const bool termB = hasB ? sb.term : sa.term;
      const unsigned po = (unsigned)k0 * (unsigned)(kObsDim * 4);   // env A's obs row in the block, bytes
      // the obs rows (header :91-96, sensors :82-83): five stores either way, so the loop's count of
      // memory instructions stays static (vm_wait below)
      if (span2) {
        // span dword 64 j + l - sh = lane l of store j: [header A | sensors A | header B | sensors B]
        float* const span = bobs + (unsigned)k0 * (unsigned)kObsDim - sh;   // (wave-uniform)
        const float a0 = l_norm(sa.rd0), a1 = l_norm(sa.rd1), b0 = l_norm(sb.rd0), b1 = l_norm(sb.rd1);
        const bool mA = l < kHdr + sh, mB = l < 2 * kHdr + sh;
        if (l >= sh) st_obs(span + l, mA ? hv : a0);   // (lanes < sh: the previous pair's dwords)
        st_obs(span + 64 + l, mA ? a0 : a1);
        st_obs(span + 128 + l, mA ? a1 : (mB ? hv : b0));
        st_obs(span + 192 + l, mB ? b0 : b1);
        if (mB) st_obs(span + 256 + l, b1);             // (lanes >= 30 + sh: the next pair's)
      } else {
        // per-row pieces: each row's sensors in two 256-B stores and the two headers in one (a lone
        // env, odd env count: env A's row twice, identical values to identical addresses)
        {
        // dword l of env A's row.  Add, then shift: a `4 * l` here is merged with the one that phase 1's
        // LDS set-up computes, which then stays live across the dynamics and makes them spill
        const unsigned lo = ((unsigned)k0 * (unsigned)kObsDim + (unsigned)l) << 2;
        float* const rowA = at_bytes(bobs, lo);
        float* const rowB = decltype(full)::value ? rowA + kObsDim : at_bytes(bobs, lo + (hasB ? 4u * kObsDim : 0u));
        st_obs(rowA + kHdr, l_norm(sa.rd0));
        st_obs(rowA + kHdr + 64, l_norm(sa.rd1));
        st_obs(rowB + kHdr, l_norm(hasB ? sb.rd0 : sa.rd0));
        st_obs(rowB + kHdr + 64, l_norm(hasB ? sb.rd1 : sa.rd1));
        if constexpr (SPAN) {
          // (a SPAN kernel gets here with a lone env only: lanes 0..14 its header, 15..29 the same again)
          const int hl = min(l, 2 * kHdr - 1);
          st_obs(at_bytes(bobs, po + 4u * (unsigned)(hl >= kHdr ? hl - kHdr : hl)), hv);
        } else {
          const int hl = min(l, 2 * kHdr - 1), hi = hl >= kHdr ? hl - kHdr : hl;   // (as in loop_setup)
          const float hc = hi == 12 ? (float)(kMaxAccU / 10.0) : hi == 14 ? (float)(kMaxAccR / 10.0) : 0.0f;
          // (no env B: env A's value again, to env A's row)
          const unsigned ho = (unsigned)hpk & 0x3ffu;
          const unsigned hoA = ho - (((unsigned)hpk >> 16) & 1u) * (unsigned)(4 * kObsDim);
          st_obs(at_bytes(bobs, po + (hasB ? ho : hoA)), ((hpk >> 17) & 1) ? hc : hv);
        }
        }
      }
      // reward, terminated: lanes 0..31 env A, 32..63 env B; the two wave-uniform flags become a lane
      // mask on the scalar unit (a per-lane select of them is three VALU instructions each)
      const bool term_l = half_lanes(sa.term, termB);
      const bool coll_l = half_lanes(collA, collB);
      st_out(at_bytes(brew, 4u * kl), coll_l ? -20.0f + meta.x : meta.x);
      *at_bytes(bterm, kl) = term_l;
      const bool done_l = term_l | ((nt >> 16) & 1);
      if constexpr (DONE) *at_bytes(bdone, kl) = done_l;   // (>= 7 stores still follow the DMA)
      const BallotHalves dm = ballot_halves(ballot(done_l));
      const bool doneA = dm.lo != 0u, doneB = hasB && dm.hi != 0u;
      if (__builtin_expect_with_probability(doneA | doneB, 0, kQRare)) {
        const QColdArgs c = q_cold_args();
        if (doneA) q_emit_done(c.S, c.io, e0, sa, recs + k0 * kQRec, rotA);
        if (doneB) q_emit_done(c.S, c.io, e0 + 1, sb, recs + (k0 + 1) * kQRec, rotB);
      }
      // the next pair's rows landed: at least seven stores (four sensor halves, the headers, the
      // rewards and the terminated flags) were issued after their DMA
      QMARK(5);
      vm_wait<7>();
      QMARK(6);
      if (it == 0) USV_STAMP_W(5);                      // (diagnostic: first pair done)
      cur = nxt;
      pose = pose_n;
      meta = meta_n;
      hv = hv_n;
      ++it;
      if (__builtin_expect_with_probability(S.autoreset == USV_AUTORESET_SAME_STEP && (doneA | doneB), 0, kQRare)) {
        done = (doneA ? 1u : 0u) | (doneB ? 2u : 0u);
        de0 = e0;
        break;
      }
    }
    if (__builtin_expect(!done, 1)) break;
    QMARK(11);
    const QColdArgs c = q_cold_args();
    for (; done; done &= done - 1) {
      const int e = de0 + __builtin_ctz(done);
      if constexpr (FUSED) {
        // the env's phase-1 stores (by dynamics wave (e - eb) / 64) are acknowledged before its reset
        // stores are issued: two waves' stores to one address are otherwise unordered
        const unsigned* const f = qdyn + ((e - eb) >> 6);
        while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u)
          __builtin_amdgcn_s_sleep(2);
      }
      reset_wave_ep<float, MODE>(c.S, e, uniform(qep[e - eb]), c.io.obs + (size_t)e * kObsDim);
    }
    QMARK(7);
  }
  };
  if ((nbe & 1) == 0) run_pairs(std::true_type{}); else run_pairs(std::false_type{});   // (wave-uniform, per block)
  QMARK(11);
  qprof_flush(qp);
#ifdef USV_DIAG_STAMPS
  USV_STAMP_V(4, (unsigned long long)it | ((unsigned long long)wsum << 16));   // (pairs | window sizes << 16)
#endif
  USV_STAMP_W(3);
  USV_STAMP_W(6);
}

template <int MODE, bool FUSED, bool DONE, bool CHAIN = true, bool INFO = false, bool SPAN = false>
__global__ __launch_bounds__(kQW * kWave) __attribute__((amdgpu_num_sgpr(kQSgpr), amdgpu_waves_per_eu(kQWPE, kQWPE)))
void step_q_kernel(State<float> S, IO<float> io) { step_q_body<MODE, FUSED, DONE, kQE, kQW, CHAIN, INFO, SPAN>(S, io); }
template <int MODE, bool DONE, bool CHAIN = true, bool INFO = false>
__global__ __launch_bounds__(kQW_S * kWave) __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(8, 8)))
void step_qs_kernel(State<float> S, IO<float> io) { step_q_body<MODE, true, DONE, kQE_S, kQW_S, CHAIN, INFO>(S, io); }

// Split block-queue step, first half: full-width lane-per-env dynamics writing the env records
// (make_qrec) for step_q_kernel<MODE, false, DONE>, plus truncated and the info row.
template <int MODE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, 2))) void dyn_rec_kernel(State<float> S, IO<float> io) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= S.N) return;
  const float2 a = reinterpret_cast<const float2*>(io.act)[e];
  const int nob = S.I(I_NOBS)[e];                  // (ahead of the dynamics' stores)
  float hdr[kHdr];
  float px, py, sp, cp, partial;
  bool trunc;
  env_dynamics<float, MODE>(S, e, a.x, a.y, hdr, px, py, sp, cp, partial, trunc,
                            io.info ? io.info + (size_t)e * USV_INFO_DIM : nullptr);
  io.trunc[e] = trunc;
  make_qrec(S.qrec + (size_t)e * kQRec, px, py, sp, cp, partial, nob, trunc, hdr);
}

// usv-asmc-simple, split at the ASMC chain (kQueueChain): the two UsvAsmc.compute calls of every env,
// lane per env, pose and velocity stored back; step_q_kernel<ASMC_SIMPLE, true, DONE, false> then runs
// UsvSimpleEnv.step(zeros(2)) on them in its fused phase 1.  The chain is a long dependent VALU
// stream (one wave per SIMD at 65 536 envs); this kernel holds nothing else, so it carries no records,
// headers or rewards, and the q kernel's phase 1 does that part at full width.
template <typename R>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, 2))) void asmc_chain_kernel(State<R> S, IO<R> io) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= S.N) return;
  const float2 a = reinterpret_cast<const float2*>(io.act)[e];
  R x = S.F(F_X)[e], y = S.F(F_Y)[e], psi = S.F(F_PSI)[e];
  R u = S.F(F_U)[e], v = S.F(F_V)[e], r = S.F(F_R)[e];
  asmc_env_chain<R>(S, e, S.I(I_ELAPSED)[e], a.x, a.y, x, y, psi, u, v, r);
  S.F(F_X)[e] = x; S.F(F_Y)[e] = y; S.F(F_PSI)[e] = psi;
  S.F(F_U)[e] = u; S.F(F_V)[e] = v; S.F(F_R)[e] = r;
}

}  // namespace usv
