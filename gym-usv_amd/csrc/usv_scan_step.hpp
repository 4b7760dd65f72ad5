// usv_scan_step.hpp -- the wave-per-env step: fused wave kernel, split dynamics + scan, block-wide dynamics
// (StepKind wave fused / wave split / block dynamics of usv_variant.hpp).
#pragma once

#include "usv_reset.hpp"
#include "usv_dynamics.hpp"
#include "usv_lidar.hpp"

namespace usv {

// --------------------------------------------------------------------------- wave-per-env scan
// Shared by the two fast step kernels (step_kernel_wave: dynamics + scan in one launch;
// dyn_kernel + scan_kernel: split).  Each wave owns EPW consecutive envs and, after one block
// barrier that publishes the ray table, shares nothing with the other waves of its block: the
// wave-per-env lidar loop keeps the NEXT envs' obstacle rows in flight (LDS-DMA) while the
// current ones are scanned; on the f32 window path two envs share each iteration.
//
// LDS: [ray table 128 x Vec2, block-shared]
//      [per wave: pair slots 256 x u64 | owner marks 64 x i32 | row buffers 2 x (2 rows, >= 1 KiB)]
__host__ __device__ constexpr size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
template <typename R> __host__ __device__ constexpr int row_bytes(int cap) { return 3 * obst_stride(cap) * (int)sizeof(R); }
template <typename R> __host__ __device__ constexpr size_t wave_tab_bytes() { return kSensors * 2 * sizeof(R); }
// two rows, and at least the 64 per-obstacle records (a, b, r^2, key) lidar_window2 / lidar_wave2_d leave in it
template <typename R> __host__ __device__ constexpr size_t scan_rowbuf_bytes(int cap) {
  return align16(std::max((size_t)2 * row_bytes<R>(cap), (size_t)64 * 4 * sizeof(R)));
}
// lidar_wave2 keeps pass-1 owner marks (64 ints) in the tail of the row buffer the next two-env DMA
// fills (cap <= 32: two rows), in the wave-scan slices and in the block queue's 1 KiB row buffers
static_assert(2 * row_bytes<float>(32) + 64 * 4 <= (int)scan_rowbuf_bytes<float>(32), "f32 mark2 tail");
static_assert(2 * row_bytes<float>(32) + 64 * 4 <= 1024, "block-queue mark2 tail");
template <typename R> __host__ __device__ constexpr size_t lds_scan_slice(int cap) {
  return 256 * 8 + 64 * 4 + 2 * scan_rowbuf_bytes<R>(cap);
}
template <typename R> __host__ __device__ size_t lds_scan_bytes(int cap, int waves = kWaves) {
  return wave_tab_bytes<R>() + waves * lds_scan_slice<R>(cap);
}

// LDS-DMA copy of `bytes` (multiple of 16, <= 2 KiB) from global `src` into the wave-uniform
// LDS buffer `dst`: lane l moves 16-B piece l (and l + 64).  Inline asm so hipcc does not
// track it: the compiler would otherwise drain it with vmcnt(0) at the first LDS read it
// cannot prove disjoint, i.e. inside the scan it is meant to overlap.  Completion is counted
// by hand (vm_wait) before the buffer is read.
__device__ __forceinline__ void dma_copy(const void* src, void* dst, int bytes) {
  const int nchunk = bytes / 16;
  const char* g = reinterpret_cast<const char*>(src);
  const unsigned d = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)dst);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = i * kWave + lane_id();
    if (c < nchunk) {
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                   "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(g + 16 * (size_t)c), "s"(d + 16u * i * kWave) : "memory");
    }
  }
}
// Wait until at most N vector-memory operations are outstanding (gfx9 vmcnt counts loads,
// LDS-DMA and stores in issue order): everything older than the last N has completed.
// Hand-counted vmcnt waits around the untracked inline-asm LDS-DMA.  The USV_SAFE_VMCNT build
// (libusvhip_safe.so) turns every one into vmcnt(0); tests/test_gpu_r2.py checks it is bitwise
// identical to the product build, so a miscounted wait (a DMA still in flight when its rows are
// read) would show as a difference.
template <int N> __device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 16, "vmcnt field");
#ifdef USV_SAFE_VMCNT
  __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0)
#else
  __builtin_amdgcn_s_waitcnt(0x0F70 | N);     // expcnt 7, lgkmcnt 15: no wait on those
#endif
}

template <typename R> struct ScanLds {
  typename Vec2<R>::T* rayoff;
  unsigned long long* slot;
  int* mark;
  R* row0;
  R* row1;
};
template <typename R>
__device__ __forceinline__ ScanLds<R> scan_lds(char* lds, int wave, int cap) {
  char* w = lds + wave_tab_bytes<R>() + wave * lds_scan_slice<R>(cap);
  R* r0 = reinterpret_cast<R*>(w + 256 * 8 + 64 * 4);
  return ScanLds<R>{reinterpret_cast<typename Vec2<R>::T*>(lds), reinterpret_cast<unsigned long long*>(w),
                    reinterpret_cast<int*>(w + 256 * 8), r0,
                    reinterpret_cast<R*>(reinterpret_cast<char*>(r0) + scan_rowbuf_bytes<R>(cap))};
}
// envs per scan iteration: two on the f32 window path (<= 32 obstacle lanes per env)
template <typename R, int LID> __device__ __forceinline__ int scan_step(int cap) {
  return ((LID & kLidWindow) != 0 && cap <= 32) ? 2 : 1;     // lidar_wave2 / lidar_wave2_d
}
// Issue the prologue DMAs (ray table by wave 0, the first iteration's rows) and arm the slots.
template <typename R, int LID>
__device__ __forceinline__ void scan_prologue(const State<R>& S, const ScanLds<R>& L, int wave, int e0, int ne) {
  const int cap = S.cap;
  if (wave == 0) dma_copy(S.ray_tab, L.rayoff, (int)wave_tab_bytes<R>());
  if (ne > 0) dma_copy(S.orow(e0), L.row0, min(scan_step<R, LID>(cap), ne) * row_bytes<R>(cap));
#pragma unroll
  for (int i = 0; i < 4; ++i) L.slot[i * 64 + lane_id()] = kSlotArm;
  L.mark[lane_id()] = 0;                              // lidar_window2 clears them after each call
}

// VALU issue is arbitrated by priority, then age (MI355X_MICROARCH.md, Two waves per SIMD): with
// a static split the oldest waves of a SIMD finish first and the youngest run alone at the end.
// The scan loops lower a wave's priority as it progresses (3 at the start, 0 in its last
// quarter), so the waves of a SIMD advance together and finish together.
__device__ __forceinline__ void set_prio(int p) {   // p wave-uniform
  if (p >= 3) __builtin_amdgcn_s_setprio(3);
  else if (p == 2) __builtin_amdgcn_s_setprio(2);
  else if (p == 1) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}

// Outputs of one scanned env e (wave-wide, lane l holds rays l and l + 64): the sensor half of
// its obs row; for a done env the terminal obs and the stale scan; term / collision bit k.
template <typename R, int MODE>
__device__ __forceinline__ void emit_env(const State<R>& S, const IO<R>& io, int e, const Scan<R>& sc,
                                         unsigned trunc_bit, int k, unsigned& term_m, unsigned& coll_m) {
  const int l = lane_id();
  const bool done = sc.term || trunc_bit;
  const bool coll = ballot((sc.rd0 < R(kCollDist)) | (sc.rd1 < R(kCollDist))) != 0;  // :153-156
  term_m |= (unsigned)sc.term << k;
  coll_m |= (unsigned)coll << k;
  const float s0 = (float)l_norm(sc.rd0), s1 = (float)l_norm(sc.rd1);        // :82-83
  float* row = io.obs + (size_t)e * kObsDim;
  st_out(row + kHdr + l, s0);                                  // stale scan is kept by reset
  st_out(row + kHdr + 64 + l, s1);
  if (done) {
    if (io.fobs) {                                             // terminal obs
      float* f = io.fobs + (size_t)e * kObsDim;
      f[kHdr + l] = s0;
      f[kHdr + 64 + l] = s1;
      // header: written earlier by this wave (wave kernel), by dyn_kernel, or by wave 0 of this
      // block (kBlockDyn, released before the block barrier)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (l < kHdr) f[l] = row[l];
    }
    if (S.autoreset == USV_AUTORESET_SAME_STEP) {
      S.sensor_last[(size_t)e * kSensors + l] = sc.rd0;
      S.sensor_last[(size_t)e * kSensors + 64 + l] = sc.rd1;
    }
  }
}

// The scan loop over this wave's ne envs.  Inputs lane-per-env (lane k = env e0 + k): pose
// P = (x, y, sin psi, cos psi), obstacle count nl, truncation bits trunc_m.  Writes the sensor
// half of each obs row, final obs and stale scan of done envs; returns term / collision bits.
// Precondition: the prologue DMAs have landed and the ray table is published.
template <typename R, int MODE, int LID>
__device__ __forceinline__ void scan_envs(const State<R>& S, const IO<R>& io, const ScanLds<R>& L, int e0,
                                          int ne, const R4<R>& P, int nl, unsigned trunc_m,
                                          unsigned& term_m, unsigned& coll_m, Prof& prof) {
  const int cap = S.cap;
  const int rowb = row_bytes<R>(cap);
  const int step = scan_step<R, LID>(cap);
  term_m = 0; coll_m = 0;
  auto emit = [&](int k, const Scan<R>& sc) {               // outputs of env e0 + k
    emit_env<R, MODE>(S, io, e0 + k, sc, (trunc_m >> k) & 1, k, term_m, coll_m);
  };
  const int iters = (ne + step - 1) / step;
  for (int k = 0; k < ne; k += step) {
    R* cur = ((k / step) & 1) ? L.row1 : L.row0;
    if (S.prio == 1) set_prio(3 - (4 * (k / step)) / iters);
    else if (S.prio == 2) set_prio(k + step >= ne ? 3 : 0);   // a wave's last iteration first
    prof.mark(4);
    // rows of this iteration landed: every env of the previous iteration issued its two
    // sensor-row stores after their DMA (a full pair: four), so all older ops are done
    if (k > 0) {
      if (step == 2) vm_wait<4>(); else vm_wait<2>();
    }
    if (k + step < ne)
      dma_copy(S.orow(e0 + k + step), ((k / step) & 1) ? L.row0 : L.row1, min(step, ne - k - step) * rowb);
    prof.mark(1);
    prof.count(7);
    if constexpr (std::is_same<R, float>::value && (LID & kLidWindow) != 0) {
      if (step == 2) {
        const bool hasB = k + 1 < ne;
        const bool hb = lane_id() >= 32;
        const int kl = hb ? k + 1 : k;             // this lane's env (B half: k + 1 if it exists)
        const int kc = hasB ? kl : k;
        const float lpx = __shfl(P.x, kc, kWave), lpy = __shfl(P.y, kc, kWave);
        const float lsp = __shfl(P.z, kc, kWave), lcp = __shfl(P.w, kc, kWave);
        const int lnl = (hb && !hasB) ? 0 : __shfl(nl, kc, kWave);
        Scan<float> sa, sb;
        // (pass-1 marks: the tail of the other row buffer, past the <= 768 B the next DMA fills)
        float* const oth = ((k / step) & 1) ? L.row0 : L.row1;
        lidar_wave2(cur, obst_stride(cap), lnl, lpx, lpy, ray_c(lcp, lsp, (float)kStartC, (float)kStartS),
                    ray_s(lcp, lsp, (float)kStartC, (float)kStartS), L.rayoff, L.slot, L.mark,
                    reinterpret_cast<int*>(oth) + 192, sa, sb);
        prof.mark(2);
        emit(k, sa);
        if (hasB) emit(k + 1, sb);
        prof.mark(3);
        continue;
      }
    }
    if constexpr (std::is_same<R, double>::value && (LID & kLidWindow) != 0) {
      if (step == 2) {                             // as above, f64 arithmetic (lidar_wave2_d)
        const bool hasB = k + 1 < ne;
        const bool hb = lane_id() >= 32;
        const int kl = hb ? k + 1 : k;
        const int kc = hasB ? kl : k;
        const double lpx = __shfl(P.x, kc, kWave), lpy = __shfl(P.y, kc, kWave);
        const double lsp = __shfl(P.z, kc, kWave), lcp = __shfl(P.w, kc, kWave);
        const int lnl = (hb && !hasB) ? 0 : __shfl(nl, kc, kWave);
        Scan<double> sa, sb;
        // the records overwrite this iteration's rows once every lane has read them (in-order LDS)
        lidar_wave2_d(cur, obst_stride(cap), lnl, lpx, lpy, lsp, lcp, L.rayoff, L.slot, L.mark,
                      reinterpret_cast<double4*>(cur), sa, sb);
        prof.mark(2);
        emit(k, sa);
        if (hasB) emit(k + 1, sb);
        prof.mark(3);
        continue;
      }
    }
    Scan<R> sc;
    const int os = obst_stride(cap);
    lidar_wave<R, LID>(RowSoA<R>{cur, cur + os, cur + 2 * os}, __builtin_amdgcn_readlane(nl, k), bcast(P.x, k),
                       bcast(P.y, k), bcast(P.z, k), bcast(P.w, k), L.rayoff, L.slot, L.mark, sc);
    prof.mark(2);
    emit(k, sc);
    prof.mark(3);
  }
}

// Epilogue shared by both: terminated flag and collision term of the reward (lane-per-env),
// then same-step autoreset of the done envs.
template <typename R, int MODE>
__device__ __forceinline__ void scan_epilogue(const State<R>& S, const IO<R>& io, int e0, int ne,
                                              R partial, bool have_partial, unsigned term_m,
                                              unsigned coll_m, unsigned trunc_m) {
  const int l = lane_id();
  if (l < ne) {
    const int e = e0 + l;
    const bool coll = (coll_m >> l) & 1;                                     // simple_env.py:153-156
    if (have_partial) st_out(io.rew + e, coll ? R(-20) + partial : partial);
    else if (coll) io.rew[e] = R(-20) + io.rew[e];
    io.term[e] = (term_m >> l) & 1;
    if (have_partial) io.trunc[e] = (trunc_m >> l) & 1;
    if (io.done) io.done[e] = ((term_m | trunc_m) >> l) & 1;
  }
  if (S.autoreset == USV_AUTORESET_SAME_STEP) {
    for (int k = 0; k < ne; ++k)
      if (((term_m | trunc_m) >> k) & 1) reset_wave<R, MODE>(S, e0 + k, io.obs + (size_t)(e0 + k) * kObsDim);
  }
}

// ---- fused: lane-per-env dynamics of the wave's own envs, then the scan
template <typename R, int MODE, int EPW, int LID>
__device__ __forceinline__ void step_body_wave(const State<R>& S, const IO<R>& io) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);   // wave-uniform (SGPR)
  const int l = lane_id();
  const int e0 = (blockIdx.x * kWaves + wave) * EPW;        // this wave's envs: e0 .. e0+ne-1
  const int ne = min(EPW, S.N - e0);
  const ScanLds<R> L = scan_lds<R>(lds, wave, S.cap);
  Prof prof;
  USV_STAMP_W(0);
  USV_STAMP_ID();
  if (S.prio == 1) __builtin_amdgcn_s_setprio(3);
  scan_prologue<R, LID>(S, L, wave, e0, ne);
  // dynamics: lanes 0..ne-1; lanes >= ne recompute env ne-1 and store identical values to the
  // identical addresses (benign) -- no divergent memory operations, so hipcc's own vmcnt
  // bookkeeping stays exact around the untracked DMAs
  R px = R(0), py = R(0), sp = R(0), cp = R(1);
  R partial = R(0);
  int nl = 0;
  bool trunc = false;
  if (ne > 0) {
    const int e = e0 + min(l, ne - 1);
    const float2 a = reinterpret_cast<const float2*>(io.act)[e];
    nl = S.I(I_NOBS)[e];                              // (ahead of the dynamics' stores)
    float hdr[kHdr];
    env_dynamics<R, MODE>(S, e, a.x, a.y, hdr, px, py, sp, cp, partial, trunc,
                             io.info ? io.info + (size_t)e * USV_INFO_DIM : nullptr);
    float* row = io.obs + (size_t)e * kObsDim;
#pragma unroll
    for (int i = 0; i < kHdr; ++i) row[i] = hdr[i];   // lane-per-env rows: plain stores (L2 merges them)
  }
  const unsigned trunc_m = (unsigned)ballot(trunc);
  USV_STAMP_W(1);
  // prologue DMAs landed (the dynamics' loads and stores were issued after them), then the
  // barrier publishes wave 0's ray table
  vm_wait<2>();
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (ne <= 0) return;
  USV_STAMP_W(2);
  prof.mark(0);
  unsigned term_m, coll_m;
  scan_envs<R, MODE, LID>(S, io, L, e0, ne, R4<R>{px, py, sp, cp}, nl, trunc_m, term_m, coll_m, prof);
  USV_STAMP_W(3);
  scan_epilogue<R, MODE>(S, io, e0, ne, partial, true, term_m, coll_m, trunc_m);
  prof.mark(5);
  prof.flush(blockIdx.x * kWaves + wave);
  USV_STAMP_W(6);
}

template <typename R, int MODE, int EPW, int LID>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(80), amdgpu_num_vgpr(64)))
void step_kernel_wave_tight(State<R> S, IO<R> io) { step_body_wave<R, MODE, EPW, LID>(S, io); }

template <typename R, int MODE, int EPW, int LID>
__global__ __launch_bounds__(kBlock) void step_kernel_wave(State<R> S, IO<R> io) {
  step_body_wave<R, MODE, EPW, LID>(S, io);
}

// ---- split: dyn_kernel (full-width lane-per-env dynamics: state, obs header, partial reward
// into rew, truncation into trunc, pose record), then scan_kernel
template <typename R, int MODE>
__global__ __launch_bounds__(kBlock) void dyn_kernel(State<R> S, IO<R> io) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= S.N) return;
  const float2 a = reinterpret_cast<const float2*>(io.act)[e];
  const int nob = S.I(I_NOBS)[e];                    // (ahead of the dynamics' stores)
  float hdr[kHdr];
  R px, py, sp, cp, partial;
  bool trunc;
  env_dynamics<R, MODE>(S, e, a.x, a.y, hdr, px, py, sp, cp, partial, trunc,
                             io.info ? io.info + (size_t)e * USV_INFO_DIM : nullptr);
  float* row = io.obs + (size_t)e * kObsDim;
#pragma unroll
  for (int i = 0; i < kHdr; ++i) row[i] = hdr[i];     // lane-per-env rows: plain stores (L2 merges them)
  S.pose[2 * (size_t)e] = R4<R>{px, py, sp, cp};
  S.pose[2 * (size_t)e + 1] = R4<R>{partial, R(nob), R(trunc ? 1 : 0), R(0)};
  io.rew[e] = partial;
  io.trunc[e] = trunc;
}

// WPB waves per block: 4 (256 threads) or 1 (64 threads: many small blocks, so the hardware
// dispatcher refills a SIMD as soon as one wave finishes and the drain tail is one small block)
template <typename R, int MODE, int EPW, int LID, int WPB>
__device__ __forceinline__ void scan_body(const State<R>& S, const IO<R>& io) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int wave = WPB == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);   // SGPR
  const int l = lane_id();
  const int e0 = (blockIdx.x * WPB + wave) * EPW;
  const int ne = min(EPW, S.N - e0);
  const ScanLds<R> L = scan_lds<R>(lds, wave, S.cap);
  Prof prof;
  USV_STAMP_W(0);
  USV_STAMP_ID();
  scan_prologue<R, LID>(S, L, wave, e0, ne);
  // per-env inputs, lane-per-env (lanes >= ne repeat env ne-1), read once: the scan loop then
  // issues no vector loads and its counted vm_wait stays exact
  const int ec = max(0, min(e0 + min(l, ne - 1), S.N - 1));
  const R4<R> P = S.pose[2 * (size_t)ec];
  const int nl = S.I(I_NOBS)[ec];
  const unsigned trunc_m = (unsigned)ballot(io.trunc[ec] != 0);
  vm_wait<0>();
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (ne <= 0) return;
  USV_STAMP_W(1);
  prof.mark(0);
  unsigned term_m, coll_m;
  scan_envs<R, MODE, LID>(S, io, L, e0, ne, P, nl, trunc_m, term_m, coll_m, prof);
  USV_STAMP_W(3);
  scan_epilogue<R, MODE>(S, io, e0, ne, R(0), false, term_m, coll_m, trunc_m);
  prof.mark(5);
  prof.flush(blockIdx.x * WPB + wave);
  USV_STAMP_W(6);
}

template <typename R, int MODE, int EPW, int LID, int WPB>
__global__ __launch_bounds__(kWave * WPB) __attribute__((amdgpu_num_sgpr(80), amdgpu_num_vgpr(64)))
void scan_kernel_tight(State<R> S, IO<R> io) { scan_body<R, MODE, EPW, LID, WPB>(S, io); }

template <typename R, int MODE, int EPW, int LID, int WPB>
__global__ __launch_bounds__(kWave * WPB) void scan_kernel(State<R> S, IO<R> io) {
  scan_body<R, MODE, EPW, LID, WPB>(S, io);
}

// f64 scan compiled for more waves per SIMD (the uncapped f64 scan takes 141 VGPRs: 3 waves)
constexpr int kF64ScanWaves = 4;
template <typename R, int MODE, int EPW, int LID, int WPB>
__global__ __launch_bounds__(kWave * WPB) __attribute__((amdgpu_waves_per_eu(kF64ScanWaves, kF64ScanWaves)))
void scan_kernel_d(State<R> S, IO<R> io) { scan_body<R, MODE, EPW, LID, WPB>(S, io); }

// ---- fused with block-wide dynamics (kBlockDyn, f64 usv-simple): wave 0 of each 4-wave block runs
// the dynamics of the block's 4 * EPW <= 64 envs lane-per-env (full width at EPW = 16, as the split
// dyn_kernel does) and hands each env's pose, obstacle count, partial reward and truncation to its
// scanning wave through LDS; waves 1..3 meanwhile wait at the barrier with their first rows in
// flight.  Same per-env arithmetic as kWaveFused and kWaveSplit, one launch instead of two (no pose records
// through HBM, no second launch ramp).
template <typename R> __host__ __device__ constexpr size_t lds_blockdyn_bytes(int cap) {
  return (lds_scan_bytes<R>(cap) + 31) / 32 * 32 + 2 * kWave * sizeof(R4<R>);
}
template <typename R, int MODE, int EPW, int LID>
__device__ __forceinline__ void step_body_blockdyn(const State<R>& S, const IO<R>& io) {
  static_assert(kWaves * EPW <= kWave, "one dynamics lane per env of the block");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);   // wave-uniform (SGPR)
  const int l = lane_id();
  const int eb = blockIdx.x * kWaves * EPW;                 // the block's envs eb .. eb+nbe-1
  const int nbe = min(kWaves * EPW, S.N - eb);
  const int e0 = eb + wave * EPW;                           // this wave's envs e0 .. e0+ne-1
  const int ne = min(EPW, S.N - e0);
  const ScanLds<R> L = scan_lds<R>(lds, wave, S.cap);
  R4<R>* const rec = reinterpret_cast<R4<R>*>(lds + (lds_scan_bytes<R>(S.cap) + 31) / 32 * 32);
  Prof prof;
  USV_STAMP_W(0);
  USV_STAMP_ID();
  if (S.prio == 1) __builtin_amdgcn_s_setprio(3);
  scan_prologue<R, LID>(S, L, wave, e0, ne);
  if (wave == 0) {
    // lanes >= nbe recompute env nbe-1 and store identical values to identical addresses (no
    // divergent memory operations: hipcc's vmcnt bookkeeping stays exact around the DMAs)
    const int e = eb + min(l, nbe - 1);
    const float2 a = reinterpret_cast<const float2*>(io.act)[e];
    const int nob = S.I(I_NOBS)[e];                        // (ahead of the dynamics' stores)
    float hdr[kHdr];
    R px, py, sp, cp, partial;
    bool trunc;
    env_dynamics<R, MODE>(S, e, a.x, a.y, hdr, px, py, sp, cp, partial, trunc,
                          io.info ? io.info + (size_t)e * USV_INFO_DIM : nullptr);
    float* row = io.obs + (size_t)e * kObsDim;
#pragma unroll
    for (int i = 0; i < kHdr; ++i) row[i] = hdr[i];         // lane-per-env rows: plain stores
    rec[l] = R4<R>{px, py, sp, cp};
    rec[kWave + l] = R4<R>{partial, R(nob), R(trunc ? 1 : 0), R(0)};
    USV_STAMP_W(1);
    if (io.fobs || S.autoreset == USV_AUTORESET_SAME_STEP) {
      // waves 1-3 read these header rows back for their done envs' terminal obs (emit_env), and
      // reset their done envs, whose state this wave stored (same-step autoreset): every store
      // complete and released to the workgroup before the barrier, so no reset store of another
      // wave can be overtaken by one of these
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      vm_wait<0>();
    } else {
      vm_wait<2>();   // the prologue DMA landed: the header stores above were issued after it
    }
  } else {
    vm_wait<0>();
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // records + ray table published
  if (ne <= 0) return;
  USV_STAMP_W(2);
  prof.mark(0);
  const int k = wave * EPW + min(l, ne - 1);                // lane-per-env view of this wave's envs
  const R4<R> P = rec[k], M = rec[kWave + k];
  const unsigned trunc_m = (unsigned)ballot(M.z != R(0));
  unsigned term_m, coll_m;
  scan_envs<R, MODE, LID>(S, io, L, e0, ne, P, (int)M.y, trunc_m, term_m, coll_m, prof);
  USV_STAMP_W(3);
  scan_epilogue<R, MODE>(S, io, e0, ne, M.x, true, term_m, coll_m, trunc_m);
  prof.mark(5);
  prof.flush(blockIdx.x * kWaves + wave);
  USV_STAMP_W(6);
}

template <typename R, int MODE, int EPW, int LID>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kF64ScanWaves, kF64ScanWaves)))
void step_kernel_blockdyn(State<R> S, IO<R> io) { step_body_blockdyn<R, MODE, EPW, LID>(S, io); }

}  // namespace usv
