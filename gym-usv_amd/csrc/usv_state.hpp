// usv_state.hpp -- device state (State, IO; its rows and sizes: usv_layout.hpp), the f32 heading frame, output stores and the
// observation header shared by every kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "usv_device.hpp"
#include "usv_diag.hpp"
#include "usv_hip.h"
#include "usv_variant.hpp"

namespace usv {

// (x, y, r, r*r) of one obstacle as a native 4-vector (one 16-B / 32-B access, selectable in
// registers without a stack temporary)
template <typename R> struct V4;
template <> struct V4<float> { typedef float T __attribute__((ext_vector_type(4))); };
template <> struct V4<double> { typedef double T __attribute__((ext_vector_type(4))); };
template <typename R> using R4 = typename V4<R>::T;

// Device state.  All real SoA fields share one allocation (field i at freal + i*fstride) and
// the int fields another, so the kernel holds two base pointers instead of twenty (kernel
// arguments live in SGPRs; fewer of them keeps the kernel at <= 80 SGPRs = 8 blocks per CU).
// The row enums (RealField, IntField, kV0*), the sizes and the slab the pointers are carved from
// are in usv_layout.hpp.
template <typename R> struct State {
  R* freal;                // [F_NREAL][fstride]
  int32_t* fint;           // [I_NINT][fstride]
  R* obst;                 // [N][3][ostride]: per env the planes x[ostride], y[ostride], r[ostride]
                           //   (slots >= n_obs zero); one env's row is 3 * ostride * sizeof(R) bytes
  R* sensor_last;          // [N][128]
  R* asmc;                 // [16][N]
  R* v0;                   // [21][fstride] legacy envs: last[9], aux[3], target[6], action_last,
                           //   ye_int, ye_last (usv-asmc-ye-int-v0)
  const R* ray_tab;        // [128][2] (cos, sin)(start + i*res)
  R4<R>* pose;             // [N][2] pose record after the step's dynamics (split wave step):
                           //   (x, y, sin psi, cos psi), (partial reward, n_obs, truncated, 0)
  float* qrec;             // [N][kQRec] f32 env record of the split block-queue step (dyn_rec_kernel)
  uint32_t* nprng;         // [10][fstride] NumPy PCG64 per env (state hi/lo, inc hi/lo as 32-bit
                           //   words, has_uint32, uinteger) for the NumPy-exact reset
  uint32_t* npmt;          // [625][fstride] legacy envs: np.random.RandomState MT19937 key[624], pos
  int np_reset;            // 1: resets draw from NumPy's Generator(PCG64) (np_reset) -- legacy
                           //   envs: from np.random's MT19937 (NpMt) -- not Philox
  int perturb;             // usv-asmc-simple: do_perturb (USV_FLAG_PERTURB)
  const R* exp;            // custom experiment applied by every reset, or null (kExp* layout)
  int N, cap, limit, autoreset;
  int prio;                // scan loops: raise the issue priority of lagging waves (s_setprio)
  int rowspan;             // block-queue step: store an env pair's obs rows as one 32-B-aligned span
  int qyoung;              // block-queue step: blocks from this index raise kQYoungWaves waves' issue
                           //   priority (a CU's second block of a one-round grid; INT_MAX: none)
  int fstride;             // elements between fields (>= N, 256-B aligned)
  int ostride;             // obstacle plane stride: cap rounded up to a multiple of 4
  uint64_t seed, gid0;
  __host__ __device__ R* F(int i) const { return freal + (size_t)i * fstride; }
  __host__ __device__ int32_t* I(int i) const { return fint + (size_t)i * fstride; }
  __host__ __device__ R* V(int i) const { return v0 + (size_t)i * fstride; }
  __host__ __device__ R* orow(int e) const { return obst + (size_t)e * 3 * ostride; }
};

// Heading representation of the f32 usv-simple / usv-asmc-simple state.  The reference integrates the
// heading without wrapping (simple_env.py:323, usv_asmc.py:234), so it grows without bound, and a float
// of 400 rad holds it to only +-1.5e-5 rad: every step's rounding then moved the angle feature
// (obs[3] = angle / pi) by ~5e-6 and the pose by the heading error times the distance run.  The f32
// state keeps psi = phi + 2 pi k instead: phi (F_PSI, a float within about a turn of zero) and the
// whole turns k (I_TURNS, int), with UsvAsmc's psi_d_last in phi's frame; the host state interface
// returns phi + 2 pi k in float64.  Every use of the heading is through sin / cos, wrap(. - psi) or
// differences, which are 2 pi-periodic or frame-free.  The f64 build keeps the reference's absolute
// heading (k = 0 always) and its arithmetic order.
constexpr float kTwoPiHi = 6.28318548f, kTwoPiLo = 1.74845553e-07f;   // 2 pi = hi - lo (float split)
template <typename R> __device__ __forceinline__ R turns_of(R psi) { return rint(psi * R(0.15915494309189535)); }
// psi - 2 pi n in float, the high part exact by Sterbenz for |n| <= 1 and |psi| within a turn or two
__device__ __forceinline__ float sub_turns(float psi, float n) { return fmaf(n, kTwoPiLo, fmaf(-n, kTwoPiHi, psi)); }
// A reset's heading (drawn, or the custom experiment's), with its whole turns split off in the f32 build
template <typename R> __device__ __forceinline__ void store_heading(const State<R>& S, int e, R psi) {
  if constexpr (std::is_same<R, float>::value) {
    const float n = turns_of(psi);
    S.F(F_PSI)[e] = sub_turns(psi, n);
    S.I(I_TURNS)[e] = (int)n;
  } else {
    S.F(F_PSI)[e] = psi;
  }
}
// End of an f32 step (env_dynamics): once the heading phi has left [-pi, pi], its whole turns move
// into k, and (usv-asmc-simple) UsvAsmc's psi_d_last with it, so the stored phi is always within
// [-pi, pi] and the host's phi + 2 pi k splits back into the same (phi, k).  k and psi_d_last are
// loaded with the rest of the state and stored back plain: a load after the dynamics' stores would
// make the wave wait for their acks (one vmcnt counter), and atomic adds are wrong for the lanes that
// repeat a wave's last env (each would add the turns again), where plain stores of the same value
// are not.
// phi + 2 pi k (the reference's heading) in R: for the info row
template <typename R> __device__ __forceinline__ R heading_abs(R phi, int k) {
  if constexpr (std::is_same<R, float>::value) {
    const float kf = (float)k;
    return fmaf(-kf, kTwoPiLo, fmaf(kf, kTwoPiHi, phi));
  } else {
    return phi;
  }
}
template <typename R> struct IO {
  const float* act;        // [N][2]
  float* obs;              // [N][143]
  R* rew;                  // [N]
  uint8_t* term;           // [N]
  uint8_t* trunc;          // [N]
  float* fobs;             // [N][143] or null
  const uint8_t* mask;     // [N] or null (reset kernel)
  R* info;                 // [N][USV_INFO_DIM] in R (f32 / f64 build) or null: step info (step kernels) / reset info
  int kpath;               // reset kernel: options['place_obstacles_on_path'] (0 = none)
  uint8_t* done;           // [N] terminated | truncated (gymnasium's info['_final_obs']) or null
};

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kEPBReset = 64;   // envs per block of the reset kernel
constexpr int kLidDefault = kLidFull;  // lidar variant of the reset kernel (all variants give identical scans)

template <typename R> __device__ __forceinline__ R big() { return R(1e30); }

// Output rows (obs, reward) are stored write-through (sc1: the line leaves the XCD's L2 as it is
// written, instead of being written back at the kernel boundary) where a wave stores contiguous
// bytes (a row's sensors, consecutive envs' rewards); lane-per-env stores to 64 different rows stay
// plain, so that L2 merges them.  The next launch on the stream
// then starts without a write-back of ~40 MB of dirty obs lines: 20.9 -> 19.4 us per step at
// 65 536 envs (back-to-back launches, tools/exp_ab.sh); the same policy for the dynamics' state
// stores measured slower (19.8 us), non-temporal stores in between (20.1 us).
template <typename T> __device__ __forceinline__ void st_out(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // global_store ... sc1
}
// obs-row stores of the block-queue step: write-through like st_out
template <typename T> __device__ __forceinline__ void st_obs(T* p, T v) { st_out(p, v); }

// (the obs-row store layout of the block-queue step, State::rowspan, and the issue-priority mode,
// State::prio, are described with their defaults in usv_variant.hpp)

// Division and square root of the per-step dynamics: in the f32 build the hardware reciprocal and
// square root (1 ulp; the reference's float64 values are matched to SURVEY 8(c)'s tolerance), which
// shortens the dependent chain of the block queue's phase 1 (barrier exit 3.4 -> 2.6 us); IEEE in
// the f64 build.
template <typename R> __device__ __forceinline__ R dyn_div(R a, R b) { return a / b; }
template <typename R> __device__ __forceinline__ R dyn_sqrt(R x) { return m_sqrt(x); }
template <> __device__ __forceinline__ float dyn_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
template <> __device__ __forceinline__ float dyn_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

template <typename R> struct Vec2;
template <> struct Vec2<float> { using T = float2; };
template <> struct Vec2<double> { using T = double2; };

// obs[0:15] = [velocity/10, target_state(4), last_action[[0,2]]/max_action[[0,2]],
//              max_action/10, max_acceleration/10]   (simple_env.py:72-96)
// x / c for a compile-time constant c: correctly rounded in the f64 build (div_const), a multiply by the
// rounded reciprocal (<= 1 ulp) in the f32 build.
template <typename R> __device__ __forceinline__ R cdiv(R x, double c) { return div_const(x, c); }
template <> __device__ __forceinline__ float cdiv(float x, double c) { return x * (float)(1.0 / c); }

template <typename R>
__device__ __forceinline__ void make_header(float (&h)[kHdr], R u, R v, R r, R angle, R dist,
                                            R ye, R refv, R act_u, R act_r, R mu, R mr) {
  h[0] = (float)cdiv(u, 10); h[1] = (float)cdiv(v, 10); h[2] = (float)cdiv(r, 10);
  h[3] = (float)cdiv(angle, kPi); h[4] = (float)cdiv(dist, kDiag);
  h[5] = (float)cdiv(ye, 10); h[6] = (float)cdiv(refv, 10);
  h[7] = (float)dyn_div(act_u, mu); h[8] = (float)dyn_div(act_r, mr);
  h[9] = (float)cdiv(mu, 10); h[10] = 0.0f; h[11] = (float)cdiv(mr, 10);
  h[12] = (float)(kMaxAccU / 10.0); h[13] = 0.0f; h[14] = (float)(kMaxAccR / 10.0);
}

}  // namespace usv
