// usv_kernels.hip -- host side and C ABI (include/usv_hip.h) of the batched USV path-following
// environment for gfx950.  The single translation unit of the library; the device code lives in
// the headers it includes, in this order:
//   usv_variant.hpp       step-variant kinds, block shapes and rules (host C++, no HIP)
//   usv_layout.hpp        state layout: constants, the slab's regions, the field table (host C++, no HIP)
//   usv_device.hpp        constants, math shims, wave helpers, Philox, the ASMC substep
//   usv_diag.hpp          instrumentation of the diagnostic builds, no-ops in the product
//   usv_state.hpp         State / IO, fields, heading frame, output stores, obs header
//   usv_reset.hpp         Philox / experiment / NumPy-exact resets, autoreset kernels
//   usv_dynamics.hpp      asmc_compute_kernel, the ASMC chain, env_dynamics
//   usv_lidar.hpp         brute and window lidar, lidar_wave, LDS head
//   usv_scan_step.hpp     wave-per-env step (wave fused, wave split, block dynamics)
//   usv_queue_step.hpp    block-queue step (queue split, fused, after the ASMC chain)
//   usv_reset_kernel.hpp  explicit reset kernel
//   usv_legacy.hpp        usv-asmc-v0 and the legacy float64 family
//   usv_noscan_step.hpp   scan-free step (ignore_obstacles)
//   usv_wrap_layout.hpp   the fused wrappers' frame ring: slots, stride, window (host C++, no HIP)
//   usv_row_copy.hpp      the trainer kernels' row copy: 16-B pieces at 4-B alignment, optional transform
//   usv_wrap.hpp          frame stack + episode statistics behind the step (usv_wrap_step / _reset)
//   usv_norm_math.hpp     VecNormalize: moments arithmetic, work split, transform (host C++, no HIP)
//   usv_norm.hpp          VecNormalize in front of the frame stack (usv_wrap_step_norm / _reset_norm)
//   usv_rollout_math.hpp  rollout buffer: bootstrap, GAE step, terminal-slot numbering (host C++, no HIP)
//   usv_rollout.hpp       RolloutBuffer + truncation bootstrap + GAE (usv_rollout_put_obs / _put_step / _gae)
//   usv_rollout_frames_math.hpp  frame-deduplicated obs storage: rows, live mask, clear rule (host C++, no HIP)
//   usv_rollout_frames.hpp  frame store and minibatch gather (usv_rollout_put_obs_frames / usv_rollout_gather)
//   usv_sde_math.hpp      gSDE head: Philox numbering, Box-Muller, sums, clip, log-probability (host C++, no HIP)
//   usv_sde.hpp           gSDE heads: one row loop under the three forwards, the two backwards, weights
//                         (usv_sde_sample / usv_sde_weights / usv_sde_squash_forward / _backward / usv_sde_eval_forward /
//                         _backward)
//   usv_sde_noise.inc     the four gSDE kernels that draw noise, stated once and included twice by usv_sde.hpp: with
//                         the epoch in the arguments, and read from a device word (usv_sde_*_dev)
//   usv_replay_math.hpp   replay buffer: slots, frame rows, age and live masks, n-step runs (host C++, no HIP)
//   usv_replay.hpp        ReplayBuffer: frame-deduplicated ring and fused sampling (usv_replay_put_obs / _put_step / _gather /
//                         _gather_nstep)
//   usv_sac_math.hpp      SAC update: TD target, losses, unit gradients, the sums' order, Polyak (host C++, no HIP)
//   usv_sac.hpp           SAC update: fused critic and policy losses, their backward; the reduction's row loop and
//                         finish, which usv_caps.hpp and usv_optim.hpp use too
//                         (usv_sac_critic_loss / _policy_loss / _loss_backward)
//   usv_caps_math.hpp     CAPS regulariser: counter layout of the perturbation, distances, unit gradients (host C++, no HIP)
//   usv_caps.hpp          CAPS regulariser: perturbed observations, the fused loss (usv_caps_perturb / usv_caps_loss)
//   usv_caps_noise.inc    caps_perturb_kernel, stated once and included twice likewise (usv_caps_perturb_dev)
//   usv_optim_math.hpp    optimizer step: Adam's scalars and element update, the clip, the norm's order (host C++, no HIP)
//   usv_optim.hpp         kernels over a tensor list: clip_grad_norm_ and Adam (the list passed by value), Polyak (a
//                         device table), one element loop under both (usv_adam_step / usv_polyak_update); Adam with
//                         its step and lr in a device clock block, and the one-thread counter kernels
//                         (usv_adam_step_dev / usv_counter_add): what a captured graph can replay
//   usv_ppo_math.hpp      PPO loss: moments, the row's terms and unit gradients, the finish, explained variance
//                         (host C++, no HIP)
//   usv_ppo.hpp           PPO loss: two moment kernels and the fused loss on usv_sac.hpp's reduction
//                         (usv_ppo_loss / usv_ppo_explained_variance)
//   usv_rollout_gather.inc  the minibatch gather, stated once and included twice: by usv_rollout_frames.hpp with the
//                         indices in a tensor, by usv_rollout_perm.hpp with a cursor and a keyed permutation
//   usv_rollout_perm_math.hpp  the permutation (Feistel network, cycle walking, Philox keys) and the minibatch cursor
//                         (host C++, no HIP)
//   usv_rollout_perm.hpp  the gather a graph can replay and the cursor's tick (usv_rollout_gather_perm)
// Reference: see include/usv_hip.h for the file:line each entry point replaces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <cstdlib>
#include <cstring>
#include <string>
#include <variant>
#include <vector>

#include "usv_hip.h"
// (definition order, which is the order of the kernels in the code object)
#include "usv_state.hpp"
#include "usv_reset.hpp"
#include "usv_dynamics.hpp"
#include "usv_lidar.hpp"
#include "usv_scan_step.hpp"
#include "usv_queue_step.hpp"
#include "usv_reset_kernel.hpp"
#include "usv_legacy.hpp"
#include "usv_noscan_step.hpp"   // (after the others: the kernels before it keep their place in the code object)
#include "usv_wrap.hpp"
#include "usv_norm.hpp"
#include "usv_rollout.hpp"
#include "usv_rollout_frames.hpp"
#include "usv_sde.hpp"
#include "usv_replay.hpp"
#include "usv_sac.hpp"           // (after the others: every kernel before it keeps its place in the code object)
#include "usv_caps.hpp"          // (after usv_sac.hpp, for the same reason)
#include "usv_optim.hpp"         // (after usv_caps.hpp, for the same reason)
#include "usv_ppo.hpp"           // (after usv_optim.hpp, for the same reason)
#include "usv_rollout_perm.hpp"  // (last, for the same reason)

// ============================================================================= host side
using namespace usv;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                 \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess)                                                             \
      return fail(USV_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e));      \
  } while (0)

struct Handle {
  usv_config cfg;
  int device;
  // step-kernel variant: StepKind, envs per block, lidar bits (usv_variant.hpp; written by apply_variant)
  int kind = 0, epb = 0, lid = 0;
  int cus = 256;                       // compute units of the device (State::qyoung)
  bool ignore = false;                 // ignore_obstacles (simple_env.py:49): the scan-free step replaces the variant
  void* slab = nullptr;
  SlabLayout lay{};                    // the slab's regions and the public fields in them (usv_layout.hpp)
  FieldTable fields{};
  void* exp_buf = nullptr;             // device usv_experiment record (kExp* layout, in R)
  std::variant<State<float>, State<double>> st;   // by cfg.precision (usv_create)
};

// f(S) with the handle's state, State<float> or State<double>
template <typename F>
auto with_state(Handle* h, F&& f) { return std::visit(f, h->st); }

// Installs a step variant (default_variant / variant_allowed): the only writer of these members.
void apply_variant(Handle* h, const Variant& v) {
  h->kind = v.kind;
  h->epb = v.epb;
  h->lid = v.lid;
  with_state(h, [&](auto& S) { S.prio = v.prio; S.rowspan = v.rowspan; });
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

template <typename R>
int carve(Handle* h, State<R>& S) {
  const size_t N = (size_t)h->cfg.num_envs;
  const SlabLayout& L = h->lay = slab_layout(h->cfg, sizeof(R));
  h->fields = field_table(h->cfg, L);
  HIP_TRY(hipMalloc(&h->slab, L.total));
  HIP_TRY(hipMemset(h->slab, 0, L.total));
  auto at = [&](Region r) { return L.size[r] ? (void*)((char*)h->slab + L.off[r]) : nullptr; };
  S.freal = (R*)at(R_FREAL);
  S.fint = (int32_t*)at(R_FINT);
  S.fstride = (int)L.fstride;
  S.ostride = (int)L.ostride;
  S.obst = (R*)at(R_OBST);
  S.sensor_last = (R*)at(R_SENSOR_LAST);
  S.asmc = (R*)at(R_ASMC);
  S.v0 = (R*)at(R_V0);
  R* tab = (R*)at(R_RAY_TAB);
  S.ray_tab = tab;
  S.pose = (R4<R>*)at(R_POSE);
  S.qrec = (float*)at(R_QREC);
  S.nprng = (uint32_t*)at(R_NPRNG);
  h->exp_buf = at(R_EXP);
  S.exp = nullptr;                                       // usv_set_experiment installs it
  S.perturb = (h->cfg.flags & USV_FLAG_PERTURB) != 0;
  S.npmt = (uint32_t*)at(R_NPMT);                        // legacy ids only, else null
  S.np_reset = 0;
  S.N = h->cfg.num_envs;
  S.cap = h->cfg.obstacle_cap;
  S.limit = h->cfg.max_episode_steps;
  S.autoreset = h->cfg.autoreset;
  S.qyoung = INT_MAX;                                    // (set per launch: launch_step)
  S.seed = h->cfg.seed;
  S.gid0 = h->cfg.env_id_offset;
  // ray offsets start + i*res (usv_asmc_ca_env.py:420), cos/sin in float64 on the host
  std::vector<R> ht(2 * kSensors);
  const double span = (2.0 / 3.0) * (2.0 * kPi), res = span / kSensors;
  for (int i = 0; i < kSensors; ++i) {
    const double a = i * res;            // from ray 0 (heading - 120 deg): see to_ray0
    ht[2 * i] = (R)std::cos(a);          // interleaved (c, s): the LDS image, copied verbatim
    ht[2 * i + 1] = (R)std::sin(a);
  }
  HIP_TRY(hipMemcpy(tab, ht.data(), 2 * kSensors * sizeof(R), hipMemcpyHostToDevice));
  // reference __init__ defaults: max_action = [3, 0, 3] (simple_env.py:32)
  std::vector<R> three(N, (R)3);
  HIP_TRY(hipMemcpy(S.F(F_MAX_U), three.data(), N * sizeof(R), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(S.F(F_MAX_R), three.data(), N * sizeof(R), hipMemcpyHostToDevice));
  return USV_OK;
}

// Step-kernel variants (usv_variant.hpp): the kernel of each kind, by envs per wave and lidar bits.

template <typename R, int MODE, int EPW>
void* pick_wave_lid(int lid) {
  if constexpr (std::is_same<R, float>::value && MODE == USV_MODE_SIMPLE) {
    if (lid == 0) return (void*)&step_kernel_wave_tight<R, MODE, EPW, 0>;
    if (lid == 3) return (void*)&step_kernel_wave_tight<R, MODE, EPW, 3>;
    return (void*)&step_kernel_wave_tight<R, MODE, EPW, 7>;
  }
  if (lid == 0) return (void*)&step_kernel_wave<R, MODE, EPW, 0>;
  if (lid == 3) return (void*)&step_kernel_wave<R, MODE, EPW, 3>;
  return (void*)&step_kernel_wave<R, MODE, EPW, 7>;
}
template <typename R, int MODE>
void* pick_wave(int epw, int lid, size_t* lds, int cap) {
  *lds = lds_scan_bytes<R>(cap);
  if (epw == 4) return pick_wave_lid<R, MODE, 4>(lid);
  if (epw == 16) return pick_wave_lid<R, MODE, 16>(lid);
  return pick_wave_lid<R, MODE, 8>(lid);
}

template <typename R, int MODE, int EPW, int WPB>
void* pick_scan_lid(int lid) {
  if constexpr (std::is_same<R, float>::value && MODE == USV_MODE_SIMPLE) {
    if (lid == 0) return (void*)&scan_kernel_tight<R, MODE, EPW, 0, WPB>;
    if (lid == 3) return (void*)&scan_kernel_tight<R, MODE, EPW, 3, WPB>;
    return (void*)&scan_kernel_tight<R, MODE, EPW, 7, WPB>;
  }
  if constexpr (std::is_same<R, double>::value) {
    if (lid == 7) return (void*)&scan_kernel_d<R, MODE, EPW, 7, WPB>;
  }
  if (lid == 0) return (void*)&scan_kernel<R, MODE, EPW, 0, WPB>;
  if (lid == 3) return (void*)&scan_kernel<R, MODE, EPW, 3, WPB>;
  return (void*)&scan_kernel<R, MODE, EPW, 7, WPB>;
}
template <typename R, int MODE, int WPB>
void* pick_scan(int epw, int lid) {
  if (epw == 2) return pick_scan_lid<R, MODE, 2, WPB>(lid);
  if (epw == 8) return pick_scan_lid<R, MODE, 8, WPB>(lid);
  if constexpr (std::is_same<R, double>::value && WPB == 4)
    if (epw == 16) return pick_scan_lid<R, MODE, 16, WPB>(lid);   // f64: one round of waves at 65 536 envs
  return pick_scan_lid<R, MODE, 4, WPB>(lid);
}

// Which block-queue kernel a launch runs.  chain: the phase 1 of kQueueChain, usv-asmc-simple's fused
// kernel without the ASMC chain; info: the fused kernels' info-row instantiation (kQueueSplit writes
// info in dyn_rec_kernel); span: row-span stores (State::rowspan), an instantiation of the fused
// 128-env kernels without info rows only.
struct QPick {
  int mode;
  bool fused, small, done, chain, info, span;
};
template <bool DONE, bool INFO>
void* pick_q_done(const QPick& q) {
  const bool simple = q.mode == USV_MODE_SIMPLE;
  if constexpr (!INFO)
    if (q.span && q.fused && !q.small) {
      if (simple) return (void*)&step_q_kernel<USV_MODE_SIMPLE, true, DONE, true, false, true>;
      return q.chain ? (void*)&step_q_kernel<USV_MODE_ASMC_SIMPLE, true, DONE, false, false, true>
                     : (void*)&step_q_kernel<USV_MODE_ASMC_SIMPLE, true, DONE, true, false, true>;
    }
  if (!simple && q.chain)
    return q.small ? (void*)&step_qs_kernel<USV_MODE_ASMC_SIMPLE, DONE, false, INFO>
                   : (void*)&step_q_kernel<USV_MODE_ASMC_SIMPLE, true, DONE, false, INFO>;
  if (q.small) return simple ? (void*)&step_qs_kernel<USV_MODE_SIMPLE, DONE, true, INFO>
                             : (void*)&step_qs_kernel<USV_MODE_ASMC_SIMPLE, DONE, true, INFO>;
  if (q.fused) return simple ? (void*)&step_q_kernel<USV_MODE_SIMPLE, true, DONE, true, INFO>
                             : (void*)&step_q_kernel<USV_MODE_ASMC_SIMPLE, true, DONE, true, INFO>;
  return simple ? (void*)&step_q_kernel<USV_MODE_SIMPLE, false, DONE> : (void*)&step_q_kernel<USV_MODE_ASMC_SIMPLE, false, DONE>;
}
void* pick_q(const QPick& q) {
  if (q.info && q.fused) return q.done ? pick_q_done<true, true>(q) : pick_q_done<false, true>(q);
  return q.done ? pick_q_done<true, false>(q) : pick_q_done<false, false>(q);
}
size_t q_lds_bytes(const QPick& q) { return q.small ? lds_q_bytes<kQE_S, kQW_S>() : lds_q_bytes(); }

// The kernel choice of a block-queue variant: the small blocks exist for the fused kinds only.
QPick q_pick(int mode, int kind, int epb) {
  QPick q{};
  q.mode = mode;
  q.fused = kind != kQueueSplit;
  q.small = q.fused && epb == kQE_S;
  q.chain = kind == kQueueChain;
  return q;
}
// ... of one launch: the outputs the caller asked for, and the handle's row-store layout
template <typename R>
QPick q_pick(const Handle* h, const State<R>& S, const IO<R>& io) {
  QPick q = q_pick(h->cfg.mode, h->kind, h->epb);
  q.done = io.done != nullptr;
  q.info = io.info != nullptr;
  q.span = S.rowspan != 0;
  return q;
}
// ... and every choice a handle of this mode and kind can come to launch (usv_set_kernel_variant
// may change epb and the row-store layout; done and info are per call): f(q) for each, until one fails
template <typename F>
int for_each_q_pick(int mode, int kind, F f) {
  for (const int epb : {kQE, kQE_S})
    for (const bool done : {false, true})
      for (const bool info : {false, true})
        for (const bool span : {false, true}) {
          QPick q = q_pick(mode, kind, epb);
          q.done = done;
          q.info = info;
          q.span = span;
          if (const int rc = f(q); rc != USV_OK) return rc;
        }
  return USV_OK;
}

template <typename R>
int launch_step_kernels(Handle* h, State<R>& S, const float* act, float* obs, void* rew, uint8_t* term,
                        uint8_t* trunc, uint8_t* done, float* fobs, void* info, hipStream_t st);

// The step, then (NumPy-exact reset mode) the resets of the envs that ended in it.
template <typename R>
int launch_step(Handle* h, State<R>& S, const float* act, float* obs, void* rew, uint8_t* term,
                uint8_t* trunc, uint8_t* done, float* fobs, void* info, hipStream_t st) {
  const int rc = launch_step_kernels(h, S, act, obs, rew, term, trunc, done, fobs, info, st);
  // (the legacy kernels reset inline, from the MT19937 state, in the NumPy-exact mode too)
  if (rc != USV_OK || S.autoreset != USV_AUTORESET_SAME_STEP || is_legacy(h->cfg.mode)) return rc;
  IO<R> io{act, obs, (R*)rew, term, trunc, fobs, nullptr, nullptr, 0};
  const dim3 grid((S.N + kBlock - 1) / kBlock), block(kBlock);
  if (!S.np_reset) {
    if (S.exp) hipLaunchKernelGGL((exp_autoreset_kernel<R>), grid, block, 0, st, S, io);
    HIP_TRY(hipGetLastError());
    return USV_OK;
  }
  if (h->cfg.mode == USV_MODE_SIMPLE)
    hipLaunchKernelGGL((np_autoreset_kernel<R, USV_MODE_SIMPLE>), grid, block, 0, st, S, io);
  else
    hipLaunchKernelGGL((np_autoreset_kernel<R, USV_MODE_ASMC_SIMPLE>), grid, block, 0, st, S, io);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// The scan-free step (ignore_obstacles): defined after every other launch path, so that its kernels are
// instantiated last and the ones before them keep their place in the code object.
template <typename R>
int launch_noscan(Handle* h, State<R>& S, IO<R>& io, hipStream_t st);

template <typename R>
int launch_step_kernels(Handle* h, State<R>& S, const float* act, float* obs, void* rew, uint8_t* term,
                        uint8_t* trunc, uint8_t* done, float* fobs, void* info, hipStream_t st) {
  IO<R> io{act, obs, (R*)rew, term, trunc, fobs, nullptr, is_legacy(h->cfg.mode) ? nullptr : (R*)info, 0, done};
  if (is_legacy(h->cfg.mode)) {
    const dim3 grid((S.N + kBlock - 1) / kBlock), block(kBlock);
    if (h->cfg.mode == USV_MODE_ASMC_V0)
      hipLaunchKernelGGL((v0_step_kernel<R>), grid, block, 0, st, S, io);
    else if (h->cfg.mode == USV_MODE_ASMC_YE_INT_V0)
      hipLaunchKernelGGL((legacy_step_kernel<R, kFamYeInt>), grid, block, 0, st, S, io);
    else
      hipLaunchKernelGGL((legacy_step_kernel<R, kFamPid>), grid, block, 0, st, S, io);
    HIP_TRY(hipGetLastError());
    return USV_OK;
  }
  if (h->ignore) return launch_noscan(h, S, io, st);        // whatever variant is installed
  const int epb = h->epb, lid = h->lid;
  const bool simple = h->cfg.mode == USV_MODE_SIMPLE;
  void* args[] = {(void*)&S, (void*)&io};
  if constexpr (std::is_same<R, float>::value) {
    if (is_queue(h->kind)) {                                 // block-queue step
      if (h->kind == kQueueSplit) {
        void* dyn = simple ? (void*)&dyn_rec_kernel<USV_MODE_SIMPLE> : (void*)&dyn_rec_kernel<USV_MODE_ASMC_SIMPLE>;
        HIP_TRY(hipLaunchKernel(dyn, dim3((S.N + kBlock - 1) / kBlock), dim3(kBlock), args, 0, st));
      }
      if (h->kind == kQueueChain)                            // usv-asmc-simple: the ASMC chain first
        HIP_TRY(hipLaunchKernel((void*)&asmc_chain_kernel<float>, dim3((S.N + kBlock - 1) / kBlock), dim3(kBlock), args, 0, st));
      const QPick q = q_pick(h, S, io);
      const int qe = q.small ? kQE_S : kQE, qw = q.small ? kQW_S : kQW;
      // a one-round grid of the 128-env blocks: the second block of each CU raises priority
      const int nblk = (S.N + qe - 1) / qe;
      S.qyoung = (!q.small && nblk > h->cus && nblk <= 2 * h->cus) ? h->cus : INT_MAX;
      HIP_TRY(hipLaunchKernel(pick_q(q), dim3(nblk), dim3(qw * kWave), args, q_lds_bytes(q), st));
      return USV_OK;
    }
  }
  if constexpr (std::is_same<R, double>::value) {
    if (h->kind == kBlockDyn) {                             // fused, block-wide dynamics (f64 usv-simple)
      void* fn = epb == 64 ? (void*)&step_kernel_blockdyn<R, USV_MODE_SIMPLE, 16, 7>
                           : (void*)&step_kernel_blockdyn<R, USV_MODE_SIMPLE, 8, 7>;
      HIP_TRY(hipLaunchKernel(fn, dim3((S.N + epb - 1) / epb), dim3(kBlock), args, lds_blockdyn_bytes<R>(S.cap), st));
      return USV_OK;
    }
  }
  if (h->kind == kWaveSplit) {                              // split: dynamics, then the wave scan
    void* dyn = simple ? (void*)&dyn_kernel<R, USV_MODE_SIMPLE> : (void*)&dyn_kernel<R, USV_MODE_ASMC_SIMPLE>;
    HIP_TRY(hipLaunchKernel(dyn, dim3((S.N + kBlock - 1) / kBlock), dim3(kBlock), args, 0, st));
    void* fn = simple ? pick_scan<R, USV_MODE_SIMPLE, kWaves>(epb / kWaves, lid)
                      : pick_scan<R, USV_MODE_ASMC_SIMPLE, kWaves>(epb / kWaves, lid);
    HIP_TRY(hipLaunchKernel(fn, dim3((S.N + epb - 1) / epb), dim3(kBlock), args, lds_scan_bytes<R>(S.cap), st));
    return USV_OK;
  }
  size_t lds;                                               // kWaveFused: fused wave kernel
  void* fn = simple ? pick_wave<R, USV_MODE_SIMPLE>(epb / kWaves, lid, &lds, S.cap)
                    : pick_wave<R, USV_MODE_ASMC_SIMPLE>(epb / kWaves, lid, &lds, S.cap);
  HIP_TRY(hipLaunchKernel(fn, dim3((S.N + epb - 1) / epb), dim3(kBlock), args, lds, st));
  return USV_OK;
}

template <typename R>
int launch_reset(Handle* h, State<R>& S, const uint8_t* mask, float* obs, int kpath, void* info,
                 hipStream_t st) {
  IO<R> io{nullptr, obs, nullptr, nullptr, nullptr, nullptr, mask, is_legacy(h->cfg.mode) ? nullptr : (R*)info, kpath};
  const dim3 grid((S.N + kEPBReset - 1) / kEPBReset), block(kBlock);
  const dim3 lgrid((S.N + kBlock - 1) / kBlock);
  if (h->cfg.mode == USV_MODE_ASMC_V0)
    hipLaunchKernelGGL((v0_reset_kernel<R, kFamV0>), lgrid, block, 0, st, S, io);
  else if (h->cfg.mode == USV_MODE_ASMC_YE_INT_V0)
    hipLaunchKernelGGL((v0_reset_kernel<R, kFamYeInt>), lgrid, block, 0, st, S, io);
  else if (h->cfg.mode == USV_MODE_PID_V0)
    hipLaunchKernelGGL((v0_reset_kernel<R, kFamPid>), lgrid, block, 0, st, S, io);
  else if (h->cfg.mode == USV_MODE_SIMPLE)
    hipLaunchKernelGGL((reset_kernel<R, USV_MODE_SIMPLE>), grid, block, lds_head_bytes<R>() + kWaves * 3 * 64 * sizeof(R), st, S, io);
  else
    hipLaunchKernelGGL((reset_kernel<R, USV_MODE_ASMC_SIMPLE>), grid, block, lds_head_bytes<R>() + kWaves * 3 * 64 * sizeof(R), st, S, io);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// f32 usv-simple / usv-asmc-simple keep the heading as phi + 2 pi k (store_heading): the host sees
// and sets the reference's heading, and UsvAsmc's psi_d_last in the reference's frame.
template <typename R>
bool turn_frame(const Handle* h) {
  return std::is_same<R, float>::value && !is_legacy(h->cfg.mode);
}
template <typename R>
int heading_io(Handle* h, State<R>& S, int f, double* hd, bool to_host) {
  const size_t N = (size_t)S.N;
  constexpr double kTwoPi = 2.0 * kPi;
  std::vector<int32_t> k(N);
  HIP_TRY(hipMemcpy(k.data(), S.I(I_TURNS), N * 4, hipMemcpyDeviceToHost));
  std::vector<R> t(N);
  R* dev = f == USV_FIELD_PSI ? S.F(F_PSI) : S.asmc;          // ASMC row 0: psi_d_last
  if (to_host) {
    HIP_TRY(hipMemcpy(t.data(), dev, N * sizeof(R), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < N; ++e) {
      const double v = (double)t[e] + kTwoPi * k[e];
      if (f == USV_FIELD_PSI) hd[e] = v;
      else hd[e * kAsmcN] = v;
    }
    return USV_OK;
  }
  if (f == USV_FIELD_ASMC) {
    HIP_TRY(hipMemcpy(t.data(), dev, N * sizeof(R), hipMemcpyDeviceToHost));   // (rows 1.. already written)
    for (size_t e = 0; e < N; ++e) t[e] = (R)(hd[e * kAsmcN] - kTwoPi * k[e]);
    HIP_TRY(hipMemcpy(dev, t.data(), N * sizeof(R), hipMemcpyHostToDevice));
    return USV_OK;
  }
  // a new heading: new whole turns, and usv-asmc-simple's psi_d_last moved into the new frame.
  // The turn count is an int32: a non-finite heading, or one whose turns do not fit (|psi| beyond
  // about 1.3e10 rad), is refused before anything is written.
  for (size_t e = 0; e < N; ++e)
    if (!std::isfinite(hd[e]) || std::fabs(hd[e] / kTwoPi) > 2147483000.0)
      return fail(USV_ERR_ARG, "heading must be finite with |psi| / 2 pi < 2^31");
  std::vector<int32_t> kn(N);
  for (size_t e = 0; e < N; ++e) {
    const double n = std::nearbyint(hd[e] / kTwoPi);
    kn[e] = (int32_t)n;
    t[e] = (R)(hd[e] - kTwoPi * n);
  }
  HIP_TRY(hipMemcpy(dev, t.data(), N * sizeof(R), hipMemcpyHostToDevice));
  if (h->cfg.mode == USV_MODE_ASMC_SIMPLE) {
    std::vector<R> s0(N);
    HIP_TRY(hipMemcpy(s0.data(), S.asmc, N * sizeof(R), hipMemcpyDeviceToHost));
    for (size_t e = 0; e < N; ++e) s0[e] = (R)((double)s0[e] + kTwoPi * (k[e] - kn[e]));
    HIP_TRY(hipMemcpy(S.asmc, s0.data(), N * sizeof(R), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(S.I(I_TURNS), kn.data(), N * 4, hipMemcpyHostToDevice));
  return USV_OK;
}

// The one copy routine: gathers a field from its region (dev: the field's first element, T = R or
// int32) into host [N][per] (H = double or int32), or scatters host into it.  The field's span of
// the region is moved whole; where the span holds other data too (the obstacle planes, padded SoA
// rows), a set is a read-modify-write.
template <typename T, typename H>
int copy_field(T* dev, const Field& fd, size_t N, H* host, bool to_host) {
  const size_t per = (size_t)fd.per;
  if (!per) return USV_OK;
  const size_t span = (N - 1) * fd.env_stride + (per - 1) * fd.comp_stride + 1;
  std::vector<T> tmp(span);
  if (to_host || span != N * per) HIP_TRY(hipMemcpy(tmp.data(), dev, span * sizeof(T), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < N; ++e)
    for (size_t c = 0; c < per; ++c) {
      T& v = tmp[e * fd.env_stride + c * fd.comp_stride];
      if (to_host) host[e * per + c] = (H)v;
      else v = (T)host[e * per + c];
    }
  if (!to_host) HIP_TRY(hipMemcpy(dev, tmp.data(), span * sizeof(T), hipMemcpyHostToDevice));
  return USV_OK;
}

// host <-> device for one field; host side [N][per] float64 / int32
template <typename R>
int field_io_impl(Handle* h, State<R>& S, int f, void* host, bool to_host) {
  const size_t N = (size_t)S.N;
  if (f == USV_FIELD_PSI && turn_frame<R>(h)) return heading_io<R>(h, S, f, (double*)host, to_host);
  if (f == USV_FIELD_N_OBS && !to_host) {
    const int32_t* hv = (const int32_t*)host;
    for (size_t i = 0; i < N; ++i)
      if (hv[i] < 0 || hv[i] > S.cap) return fail(USV_ERR_ARG, "n_obs out of [0, obstacle_cap]");
  }
  const Field& fd = h->fields.row[f];
  char* const region = (char*)h->slab + h->lay.off[fd.region];
  const int rc = fd.is_int ? copy_field((int32_t*)region + fd.first, fd, N, (int32_t*)host, to_host)
                           : copy_field((R*)region + fd.first, fd, N, (double*)host, to_host);
  // psi_d_last (ASMC row 0) between the reference's frame (host) and the heading's (device, f32)
  if (rc == USV_OK && f == USV_FIELD_ASMC && turn_frame<R>(h)) return heading_io<R>(h, S, f, (double*)host, to_host);
  return rc;
}
// Writes complete before returning (hipMemcpy from pageable memory may return before the DMA
// lands), so a kernel the caller launches next on any stream sees them.
template <typename R>
int field_io(Handle* h, State<R>& S, int f, void* host, bool to_host) {
  HIP_TRY(hipDeviceSynchronize());
  const int rc = field_io_impl(h, S, f, host, to_host);
  if (rc == USV_OK && !to_host) HIP_TRY(hipDeviceSynchronize());
  return rc;
}

template <typename R>
int set_experiment(Handle* h, State<R>& S, const usv_experiment* x) {
  HIP_TRY(hipDeviceSynchronize());                       // in-flight resets may read the old one
  if (!x) {
    S.exp = nullptr;
    return USV_OK;
  }
  const int cap = h->cfg.obstacle_cap;
  std::vector<R> v((size_t)kExpObs + 3 * cap, R(0));
  v[kExpN] = (R)x->n_obs;
  v[kExpPS] = (R)x->path_start[0]; v[kExpPS + 1] = (R)x->path_start[1];
  v[kExpAngle] = (R)x->angle;
  for (int i = 0; i < 3; ++i) v[kExpPose + i] = (R)x->position[i];
  for (int j = 0; j < x->n_obs; ++j) {
    v[kExpObs + j] = (R)x->obstacle_x[j];
    v[kExpObs + cap + j] = (R)x->obstacle_y[j];
    v[kExpObs + 2 * cap + j] = (R)x->obstacle_r[j];
  }
  HIP_TRY(hipMemcpy(h->exp_buf, v.data(), v.size() * sizeof(R), hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  S.exp = (const R*)h->exp_buf;
  return USV_OK;
}

// The block-queue step's LDS exceeds the 64 KiB default: raise the dynamic-LDS limit of every kernel
// a handle of this mode and kind can launch.
int queue_lds_attr(int mode, int kind) {
  if (!is_queue(kind)) return USV_OK;
  return for_each_q_pick(mode, kind, [](const QPick& q) {
    HIP_TRY(hipFuncSetAttribute(pick_q(q), hipFuncAttributeMaxDynamicSharedMemorySize, (int)q_lds_bytes(q)));
    return (int)USV_OK;
  });
}

Handle* as_handle(void* p) { return static_cast<Handle*>(p); }

// The scan-free step (ignore_obstacles).  usv-asmc-simple f32 runs the ASMC chain in its own launch
// first, as the block-queue default does; f64 runs it inside the step (36.4 against 40.6 us split).
template <typename R, int MODE, bool CHAIN>
void* pick_noscan(bool done, bool info) {
  if (done) return info ? (void*)&noscan_step_kernel<R, MODE, CHAIN, true, true>
                        : (void*)&noscan_step_kernel<R, MODE, CHAIN, true, false>;
  return info ? (void*)&noscan_step_kernel<R, MODE, CHAIN, false, true>
              : (void*)&noscan_step_kernel<R, MODE, CHAIN, false, false>;
}
template <typename R>
int launch_noscan(Handle* h, State<R>& S, IO<R>& io, hipStream_t st) {
  // (-DUSV_NOSCAN_F64_SPLIT builds the f64 library with the chain split off too, for the A/B in DESIGN.md)
#ifdef USV_NOSCAN_F64_SPLIT
  constexpr bool kSplit = true;
#else
  constexpr bool kSplit = std::is_same<R, float>::value;
#endif
  const bool done = io.done != nullptr, info = io.info != nullptr;
  const dim3 grid((S.N + kBlock - 1) / kBlock), block(kBlock);
  void* args[] = {(void*)&S, (void*)&io};
  void* fn;
  if (h->cfg.mode == USV_MODE_SIMPLE) {
    fn = pick_noscan<R, USV_MODE_SIMPLE, true>(done, info);
  } else {
    if constexpr (kSplit) HIP_TRY(hipLaunchKernel((void*)&asmc_chain_kernel<R>, grid, block, args, 0, st));
    fn = pick_noscan<R, USV_MODE_ASMC_SIMPLE, !kSplit>(done, info);
  }
  HIP_TRY(hipLaunchKernel(fn, grid, block, args, 0, st));
  return USV_OK;
}

}  // namespace

extern "C" {

int usv_abi_version(void) { return USV_ABI_VERSION; }

#ifdef USV_DIAG_PROF
int usv_diag_prof(void* host, size_t bytes) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_prof), bytes < sizeof(g_prof) ? bytes : sizeof(g_prof)));
  return USV_OK;
}
#endif
#ifdef USV_DIAG_QPROF
int usv_diag_qprof(void* host, size_t bytes) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_qprof), bytes < sizeof(g_qprof) ? bytes : sizeof(g_qprof)));
  return USV_OK;
}
#endif
#ifdef USV_DIAG_STAMPS
int usv_diag_stamps(void* host, size_t bytes) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), bytes < sizeof(g_stamps) ? bytes : sizeof(g_stamps)));
  return USV_OK;
}
#endif

const char* usv_last_error(void) { return g_err.c_str(); }

size_t usv_config_size(void) { return sizeof(usv_config); }

int usv_asmc_compute(int32_t precision, int32_t n, const void* act, void* pos, void* vel, void* state,
                     int32_t* perturb_step, int32_t do_perturb, int32_t calls, void* stream) {
  if (precision != USV_F32 && precision != USV_F64) return fail(USV_ERR_ARG, "unknown precision");
  if (n < 0 || calls < 0) return fail(USV_ERR_ARG, "n and calls must be >= 0");
  if (n == 0 || calls == 0) return USV_OK;
  if (!act || !pos || !vel || !state) return fail(USV_ERR_ARG, "null argument");
  // launch on the device that holds the state, whatever the caller's current device is; every buffer
  // must be device-accessible memory of that device (a pageable host pointer would fault the kernel)
  auto device_of = [](const void* p) {
    hipPointerAttribute_t pa{};
    return hipPointerGetAttributes(&pa, p) == hipSuccess ? pa.device : -1;
  };
  const int dev = device_of(state);
  if (dev < 0) { (void)hipGetLastError(); return fail(USV_ERR_ARG, "state is not a device pointer"); }
  if (device_of(act) != dev || device_of(pos) != dev || device_of(vel) != dev ||
      (perturb_step && device_of(perturb_step) != dev)) {
    (void)hipGetLastError();
    return fail(USV_ERR_ARG, "act / pos / vel / perturb_step are not device pointers on the state's device");
  }
  DeviceGuard g(dev);
  const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  if (precision == USV_F32)
    hipLaunchKernelGGL(asmc_compute_kernel<float>, grid, block, 0, st, n, (const float*)act, (float*)pos,
                       (float*)vel, (float*)state, perturb_step, do_perturb, calls);
  else
    hipLaunchKernelGGL(asmc_compute_kernel<double>, grid, block, 0, st, n, (const double*)act, (double*)pos,
                       (double*)vel, (double*)state, perturb_step, do_perturb, calls);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

void usv_config_default(usv_config* cfg, int32_t mode, int32_t num_envs) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->abi_version = USV_ABI_VERSION;
  cfg->mode = mode;
  cfg->precision = USV_F32;
  cfg->num_envs = num_envs;
  cfg->obstacle_cap = 32;
  cfg->max_episode_steps = mode == USV_MODE_ASMC_SIMPLE ? 1000 : is_legacy(mode) ? 0 : 500;  // gym_usv/__init__.py
  cfg->autoreset = USV_AUTORESET_SAME_STEP;
  cfg->lidar_algo = USV_LIDAR_WINDOW;
  cfg->seed = 0;
  cfg->env_id_offset = 0;
}

int usv_create(const usv_config* cfg, int32_t device, void** out) {
  if (!cfg || !out) return fail(USV_ERR_ARG, "null argument");
  *out = nullptr;
  if (cfg->abi_version != USV_ABI_VERSION) return fail(USV_ERR_ABI, "abi_version mismatch");
  if (cfg->mode != USV_MODE_SIMPLE && cfg->mode != USV_MODE_ASMC_SIMPLE && !is_legacy(cfg->mode))
    return fail(USV_ERR_ARG, "unknown mode");
  if (cfg->precision != USV_F32 && cfg->precision != USV_F64)
    return fail(USV_ERR_ARG, "unknown precision");
  if (cfg->num_envs <= 0) return fail(USV_ERR_ARG, "num_envs must be > 0");
  if (cfg->obstacle_cap < 29 || cfg->obstacle_cap > 64)
    return fail(USV_ERR_ARG, "obstacle_cap must be in [29, 64] (reference draws up to 29)");
  if (cfg->autoreset != USV_AUTORESET_SAME_STEP && cfg->autoreset != USV_AUTORESET_DISABLED)
    return fail(USV_ERR_ARG, "unknown autoreset mode");
  if (cfg->lidar_algo != USV_LIDAR_BRUTE && cfg->lidar_algo != USV_LIDAR_WINDOW)
    return fail(USV_ERR_ARG, "unknown lidar algorithm");
  if ((cfg->flags & ~(USV_FLAG_PERTURB | USV_FLAG_IGNORE_OBSTACLES)) != 0 || cfg->reserved != 0)
    return fail(USV_ERR_ARG, "unknown flags");
  if ((cfg->flags & USV_FLAG_PERTURB) && cfg->mode != USV_MODE_ASMC_SIMPLE)
    return fail(USV_ERR_ARG, "USV_FLAG_PERTURB applies to usv-asmc-simple only");
  if ((cfg->flags & USV_FLAG_IGNORE_OBSTACLES) && is_legacy(cfg->mode))
    return fail(USV_ERR_ARG, "USV_FLAG_IGNORE_OBSTACLES applies to usv-simple / usv-asmc-simple only");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(USV_ERR_ARG, "bad device index");
  DeviceGuard g(device);
  Handle* h = new Handle();
  h->cfg = *cfg;
  h->device = device;
  h->ignore = (cfg->flags & USV_FLAG_IGNORE_OBSTACLES) != 0;
  if (cfg->precision == USV_F64) h->st = State<double>{};   // (else the zeroed State<float> it starts as)
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
      h->cus = cus;
  }
  apply_variant(h, default_variant(*cfg));
  if (const int rc = queue_lds_attr(cfg->mode, h->kind); rc != USV_OK) { delete h; return rc; }
  const int rc = with_state(h, [&](auto& S) { return carve(h, S); });
  if (rc != USV_OK) {
    if (h->slab) (void)hipFree(h->slab);
    delete h;
    return rc;
  }
  *out = h;
  return USV_OK;
}

int usv_set_kernel_variant(void* hp, int32_t kind, int32_t epb, int32_t lid) {
  Handle* h = as_handle(hp);
  if (!h) return fail(USV_ERR_ARG, "null handle");
  const VariantCheck c = variant_allowed(h->cfg, kind, epb, lid);
  if (c.refused) return fail(USV_ERR_ARG, c.refused);
  DeviceGuard g(h->device);
  HIP_TRY(hipDeviceSynchronize());                 // launches in flight keep the variant they took
  // raise the new variant's LDS limit first, and commit it to the handle only if that worked
  if (const int rc = queue_lds_attr(h->cfg.mode, kind); rc != USV_OK) return rc;
  apply_variant(h, c.v);
  return USV_OK;
}

int usv_set_ignore_obstacles(void* hp, int32_t on) {
  Handle* h = as_handle(hp);
  if (!h) return fail(USV_ERR_ARG, "null handle");
  if (is_legacy(h->cfg.mode))
    return fail(USV_ERR_ARG, "ignore_obstacles applies to usv-simple / usv-asmc-simple only");
  DeviceGuard g(h->device);
  HIP_TRY(hipDeviceSynchronize());                 // launches in flight keep the step they took
  h->ignore = on != 0;                             // (the installed variant stays, for the toggle back)
  return USV_OK;
}

int usv_get_ignore_obstacles(void* hp) {
  Handle* h = as_handle(hp);
  if (!h) return fail(USV_ERR_ARG, "null handle");
  return h->ignore ? 1 : 0;
}

void usv_destroy(void* hp) {
  Handle* h = as_handle(hp);
  if (!h) return;
  DeviceGuard g(h->device);
  (void)hipDeviceSynchronize();
  if (h->slab) (void)hipFree(h->slab);
  delete h;
}

int usv_num_envs(void* hp) { return hp ? as_handle(hp)->cfg.num_envs : fail(USV_ERR_ARG, "null handle"); }
int usv_obs_dim(void* hp) {
  return hp ? (is_legacy(as_handle(hp)->cfg.mode) ? 6 : kObsDim) : fail(USV_ERR_ARG, "null handle");
}
int usv_act_dim(void* hp) {
  return hp ? (is_legacy(as_handle(hp)->cfg.mode) ? 1 : 2) : fail(USV_ERR_ARG, "null handle");
}
int usv_reward_bytes(void* hp) {
  return hp ? (as_handle(hp)->cfg.precision == USV_F64 ? 8 : 4) : fail(USV_ERR_ARG, "null handle");
}

int usv_set_reset_rng(void* hp, int32_t kind) {
  Handle* h = as_handle(hp);
  if (!h) return fail(USV_ERR_ARG, "null handle");
  if (kind != USV_RESET_PHILOX && kind != USV_RESET_NUMPY_PCG64) return fail(USV_ERR_ARG, "unknown reset rng");
  with_state(h, [&](auto& S) { S.np_reset = kind == USV_RESET_NUMPY_PCG64; });
  return USV_OK;
}

int usv_seed(void* hp, uint64_t seed) {
  Handle* h = as_handle(hp);
  if (!h) return fail(USV_ERR_ARG, "null handle");
  DeviceGuard g(h->device);
  h->cfg.seed = seed;
  int32_t* ep = with_state(h, [&](auto& S) {
    S.seed = seed;
    return S.I(I_EPISODE);
  });
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(ep, 0, (size_t)h->cfg.num_envs * 4));
  HIP_TRY(hipDeviceSynchronize());     // ordered before launches on any (non-blocking) stream
  return USV_OK;
}

int usv_reset_ex(void* hp, const uint8_t* mask, float* obs, const usv_reset_options* opt, void* info,
                 void* stream) {
  Handle* h = as_handle(hp);
  if (!h || !obs) return fail(USV_ERR_ARG, "null argument");
  const int kpath = opt ? opt->place_obstacles_on_path : 0;
  if (kpath < 0) return fail(USV_ERR_ARG, "place_obstacles_on_path must be >= 0");
  if (kpath > 0 && is_legacy(h->cfg.mode))
    return fail(USV_ERR_ARG, "place_obstacles_on_path applies to usv-simple / usv-asmc-simple only");
  if (kpath > 0 && 29 + kpath > h->cfg.obstacle_cap)
    return fail(USV_ERR_ARG, "place_obstacles_on_path needs obstacle_cap >= 29 + k (reference draws up to 29)");
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  return with_state(h, [&](auto& S) { return launch_reset(h, S, mask, obs, kpath, info, st); });
}

int usv_reset(void* hp, const uint8_t* mask, float* obs, void* stream) {
  return usv_reset_ex(hp, mask, obs, nullptr, nullptr, stream);
}

int usv_step_ex(void* hp, const float* act, float* obs, void* rew, uint8_t* term, uint8_t* trunc,
                uint8_t* done, float* fobs, void* info, void* stream) {
  Handle* h = as_handle(hp);
  if (!h || !act || !obs || !rew || !term || !trunc) return fail(USV_ERR_ARG, "null argument");
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  return with_state(h, [&](auto& S) { return launch_step(h, S, act, obs, rew, term, trunc, done, fobs, info, st); });
}

int usv_step(void* hp, const float* act, float* obs, void* rew, uint8_t* term, uint8_t* trunc,
             float* fobs, void* stream) {
  return usv_step_ex(hp, act, obs, rew, term, trunc, nullptr, fobs, nullptr, stream);
}

int usv_set_experiment(void* hp, const usv_experiment* x) {
  Handle* h = as_handle(hp);
  if (!h) return fail(USV_ERR_ARG, "null handle");
  if (is_legacy(h->cfg.mode)) return fail(USV_ERR_ARG, "custom experiments apply to usv-simple / usv-asmc-simple only");
  if (x && (x->n_obs < 1 || x->n_obs > h->cfg.obstacle_cap || x->n_obs > 64))
    return fail(USV_ERR_ARG, "experiment n_obs must be in [1, obstacle_cap]");
  DeviceGuard g(h->device);
  return with_state(h, [&](auto& S) { return set_experiment(h, S, x); });
}

int usv_field_info(void* hp, int32_t f, int32_t* per_env, int32_t* is_int, const char** name) {
  Handle* h = as_handle(hp);
  if (!h || f < 0 || f >= USV_FIELD_COUNT) return fail(USV_ERR_ARG, "bad handle or field");
  const Field& fd = h->fields.row[f];
  if (per_env) *per_env = fd.per;
  if (is_int) *is_int = fd.is_int;
  if (name) *name = fd.name;
  return USV_OK;
}

static int field_call(void* hp, int32_t f, void* host, size_t bytes, bool to_host) {
  Handle* h = as_handle(hp);
  if (!h || !host || f < 0 || f >= USV_FIELD_COUNT) return fail(USV_ERR_ARG, "bad argument");
  if (bytes != field_bytes(h->cfg, h->fields.row[f])) return fail(USV_ERR_ARG, "byte count mismatch");
  DeviceGuard g(h->device);
  return with_state(h, [&](auto& S) { return field_io(h, S, f, host, to_host); });
}
int usv_get_field(void* hp, int32_t f, void* host, size_t bytes) { return field_call(hp, f, host, bytes, true); }
int usv_set_field(void* hp, int32_t f, const void* host, size_t bytes) {
  return field_call(hp, f, (void*)host, bytes, false);
}

size_t usv_state_bytes(void* hp) {
  Handle* h = as_handle(hp);
  if (!h) return 0;
  size_t b = 0;
  for (const Field& fd : h->fields.row) b += field_bytes(h->cfg, fd);
  return b;
}

// the blob: every field's host image, in table order
static int state_call(void* hp, void* host, size_t bytes, bool to_host) {
  Handle* h = as_handle(hp);
  if (!h || !host) return fail(USV_ERR_ARG, "bad argument");
  if (bytes != usv_state_bytes(hp)) return fail(USV_ERR_ARG, "byte count mismatch");
  char* p = (char*)host;
  for (int f = 0; f < USV_FIELD_COUNT; ++f) {
    const size_t fb = field_bytes(h->cfg, h->fields.row[f]);
    const int rc = field_call(hp, f, p, fb, to_host);
    if (rc != USV_OK) return rc;
    p += fb;
  }
  return USV_OK;
}
int usv_get_state(void* hp, void* host, size_t bytes) { return state_call(hp, host, bytes, true); }
int usv_set_state(void* hp, const void* host, size_t bytes) { return state_call(hp, (void*)host, bytes, false); }

// ---- fused wrappers (usv_wrap.hpp): handle-free, stream-ordered, like usv_asmc_compute
size_t usv_wrap_ring_stride(int32_t obs_dim, int32_t n_stack) {
  return obs_dim > 0 && n_stack >= 1 ? wrap_ring_stride(obs_dim, n_stack) : 0;
}

size_t usv_wrap_window_offset(int32_t obs_dim, int32_t n_stack, int64_t j) {
  return obs_dim > 0 && n_stack >= 1 && j >= 0 ? wrap_window_offset(obs_dim, n_stack, j) : 0;
}

// One buffer of a trainer entry.  al: its alignment, a power of two; opt: it may be null.
struct Buf {
  const void* p;
  uintptr_t al;
  bool opt = false;
};
using Bufs = std::initializer_list<Buf>;
enum BufFault { kBufOk = 0, kBufNull, kBufAlign, kBufDevice };
constexpr size_t kMaxBufs = 32;        // of one call: its struct's and its own

// The first fault among b[0 .. n): a null buffer that may not be null, then a misaligned one.  With dev,
// then one that is no device pointer on the device of b[0]; *dev is that device, -1 if b[0] is on none.
// Without dev there is no HIP call.
static BufFault check_bufs(const Buf* b, size_t n, int* dev = nullptr) {
  for (size_t i = 0; i < n; ++i)
    if (!b[i].p && !b[i].opt) return kBufNull;
  for (size_t i = 0; i < n; ++i)
    if ((reinterpret_cast<uintptr_t>(b[i].p) & (b[i].al - 1)) != 0) return kBufAlign;
  if (!dev) return kBufOk;
  *dev = -1;
  for (size_t i = 0; i < n; ++i) {
    if (!b[i].p) continue;
    hipPointerAttribute_t pa{};
    const int d = hipPointerGetAttributes(&pa, b[i].p) == hipSuccess ? pa.device : -1;
    if (i == 0) *dev = d;
    if (d < 0 || d != *dev) {
      (void)hipGetLastError();
      return kBufDevice;
    }
  }
  return kBufOk;
}
static BufFault check_bufs(Bufs b) { return check_bufs(b.begin(), b.size()); }

// The refusal of check_bufs's fault, or USV_OK: the one chain of every trainer entry.  msg: for a null buffer, a
// misaligned one, a first buffer that is no device pointer, another that is none on the first's device; without dev
// the last two are not looked for.
using BufMsgs = const char* const (&)[4];
static int refuse_bufs(const Buf* b, size_t n, int* dev, BufMsgs msg) {
  switch (check_bufs(b, n, dev)) {
    case kBufNull: return fail(USV_ERR_ARG, msg[0]);
    case kBufAlign: return fail(USV_ERR_ARG, msg[1]);
    case kBufDevice: return fail(USV_ERR_ARG, *dev < 0 ? msg[2] : msg[3]);
    case kBufOk: break;
  }
  return USV_OK;
}
// ... with the messages of the entries that name no buffer but their 16-B one: `prefix` and `wide`.
static int refuse_bufs(const Buf* b, size_t n, int& dev, const char* prefix, const char* wide) {
  const std::string p = std::string(prefix) + ": ", first = p + "the first buffer is not a device pointer",
                    null = p + "null buffer", align = p + wide + " is not 16-B aligned or a buffer is not 4-B aligned",
                    other = p + "a buffer is not a device pointer on the device that holds the first";
  const char* const msg[4] = {null.c_str(), align.c_str(), first.c_str(), other.c_str()};
  return refuse_bufs(b, n, &dev, msg);
}

// Whether `stream` is recording a graph.  An entry that would synchronise or copy from the host asks first and
// refuses: during a capture either is an error that also invalidates the capture.
static bool stream_capturing(void* stream) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return st != hipStreamCaptureStatusNone;
}

// The device word of a _dev entry `fn` (`what`: "epoch_dev", "word_dev"): not null and 4-B aligned.  No HIP call.
static int refuse_word(const char* fn, const char* what, const void* word) {
  if (!word) return fail(USV_ERR_ARG, std::string(fn) + ": null " + what);
  if ((reinterpret_cast<uintptr_t>(word) & 3) != 0) return fail(USV_ERR_ARG, std::string(fn) + ": " + what + " is not 4-B aligned");
  return USV_OK;
}

// The gathers' check of idx and of their outputs out[0 .. n), before the buffers' device is looked at.
static int refuse_gather_bufs(const char* fn, const int64_t* idx, const Buf* out, size_t n) {
  const std::string p = std::string(fn) + ": ";
  if (!idx) return fail(USV_ERR_ARG, p + "null idx");
  const BufFault of = check_bufs(out, n);
  if (of == kBufNull) return fail(USV_ERR_ARG, p + "null output");
  if ((reinterpret_cast<uintptr_t>(idx) & 7) != 0) return fail(USV_ERR_ARG, p + "idx is not 8-B aligned");
  if (of == kBufAlign) return fail(USV_ERR_ARG, p + "an output is not 4-B aligned");
  return USV_OK;
}

// The launch geometry of the kernels whose waves own kWrapEnvs envs each.
static dim3 wrap_grid(int n) { return dim3((n + kWaves * kWrapEnvs - 1) / (kWaves * kWrapEnvs)); }

static size_t norm_bufs(const usv_norm* z, Buf* out) {
  const void* const ptrs[] = {z->obs_mean, z->obs_var, z->obs_inv_std, z->obs_count, z->ret_mean, z->ret_var,
                              z->ret_inv_std, z->ret_count, z->returns, z->scratch};
  size_t n = 0;
  for (const void* p : ptrs) out[n++] = Buf{p, 8};
  return n;
}

// The shape checks (before any HIP call), then the buffers' device (`more`: the call's own; zn's, if
// given, have passed norm_check); fills the kernel's arguments.
static int wrap_args(const usv_wrap* w, const usv_norm* zn, int64_t j, Bufs more, WrapArgs& a, int& dev) {
  if (!w) return fail(USV_ERR_ARG, "null usv_wrap");
  if (w->n <= 0 || w->obs_dim <= 0 || w->n_stack < 1)
    return fail(USV_ERR_ARG, "usv_wrap: n and obs_dim must be > 0 and n_stack >= 1");
  if (!w->ring) return fail(USV_ERR_ARG, "usv_wrap: null ring");
  if (w->reward_bytes != 4 && w->reward_bytes != 8) return fail(USV_ERR_ARG, "usv_wrap: reward_bytes must be 4 or 8");
  if (j < 0) return fail(USV_ERR_ARG, "usv_wrap: the step counter j must be >= 0");
  if ((w->flags & ~USV_WRAP_CLEAR_KEEPS_SIGN) != 0 || w->reserved != 0)
    return fail(USV_ERR_ARG, "usv_wrap: unknown flags");
  if (!w->ep_ret || !w->ep_len) return fail(USV_ERR_ARG, "usv_wrap: null ep_ret / ep_len");
  if (!!w->cum_ret != !!w->cum_len || !!w->cum_ret != !!w->cum_eps)
    return fail(USV_ERR_ARG, "usv_wrap: cum_ret, cum_len and cum_eps are given together or not at all");
  Buf all[kMaxBufs] = {{w->ring, 4},          {w->ep_ret, 8},        {w->ep_len, 4},       {w->episode, 8, true},
                       {w->cum_ret, 8, true}, {w->cum_len, 8, true}, {w->cum_eps, 8, true}};
  size_t nb = 7;
  for (const Buf& b : more) all[nb++] = b;
  if (zn) nb += norm_bufs(zn, all + nb);
  if (int rc = refuse_bufs(all, nb, &dev, {"usv_wrap: null argument", "usv_wrap: a buffer is not aligned to its element size",
                                          "usv_wrap: ring is not a device pointer",
                                          "usv_wrap: a buffer is not a device pointer on the ring's device"}))
    return rc;
  const int k = w->n_stack;
  a = WrapArgs{w->n, w->obs_dim, k, w->reward_bytes, wrap_slot(j, k), wrap_mirror_slot(j, k),
               wrap_terminal_slot(j, k), (w->flags & USV_WRAP_CLEAR_KEEPS_SIGN) != 0, wrap_ring_stride(w->obs_dim, k), w->ring,
               w->ep_ret, w->ep_len, w->episode, w->cum_ret, (long long*)w->cum_len, (long long*)w->cum_eps};
  return USV_OK;
}

// ---- fused VecNormalize (usv_norm.hpp) in front of the frame stack
size_t usv_norm_scratch_bytes(int32_t n, int32_t obs_dim) {
  return n > 0 && obs_dim > 0 ? (size_t)2 * norm_num_partials(n) * ((size_t)obs_dim + 1) * sizeof(double) : 0;
}

// The checks that need no HIP call; the device of every pointer is wrap_args's to check.
static int norm_check(const usv_wrap* w, const usv_norm* z) {
  if (!z) return fail(USV_ERR_ARG, "null usv_norm");
  if (z->n <= 0 || z->obs_dim <= 0) return fail(USV_ERR_ARG, "usv_norm: n and obs_dim must be > 0");
  if (z->obs_dim > kNormMaxDim) return fail(USV_ERR_ARG, "usv_norm: obs_dim above 4096 (the tables are staged in LDS)");
  if (w && (z->n != w->n || z->obs_dim != w->obs_dim))
    return fail(USV_ERR_ARG, "usv_norm: n and obs_dim must equal the usv_wrap's");
  if ((z->flags & ~(USV_NORM_TRAINING | USV_NORM_OBS | USV_NORM_REWARD)) != 0 || z->reserved != 0)
    return fail(USV_ERR_ARG, "usv_norm: unknown flags");
  if (!(z->clip_obs >= 0.0) || !(z->clip_reward >= 0.0)) return fail(USV_ERR_ARG, "usv_norm: clip_obs and clip_reward must be >= 0");
  if (!(z->gamma >= 0.0 && z->gamma <= 1.0)) return fail(USV_ERR_ARG, "usv_norm: gamma must be in [0, 1]");
  if (!(z->epsilon > 0.0)) return fail(USV_ERR_ARG, "usv_norm: epsilon must be > 0");
  Buf own[kMaxBufs];
  switch (check_bufs(own, norm_bufs(z, own))) {
    case kBufNull: return fail(USV_ERR_ARG, "usv_norm: null buffer");
    case kBufAlign: return fail(USV_ERR_ARG, "usv_norm: a buffer is not 8-B aligned");
    default: return USV_OK;
  }
}

static NormArgs norm_args(const usv_norm* z, bool update) {
  const bool tr = update && (z->flags & USV_NORM_TRAINING) != 0;
  return NormArgs{z->n, z->obs_dim, tr && (z->flags & USV_NORM_OBS) != 0, tr && (z->flags & USV_NORM_REWARD) != 0,
                  (z->flags & USV_NORM_REWARD) != 0, z->clip_obs, z->clip_reward, z->gamma, z->epsilon,
                  z->obs_mean, z->obs_var, z->obs_inv_std, z->obs_count, z->ret_mean, z->ret_var, z->ret_inv_std,
                  z->ret_count, z->returns, z->scratch};
}

extern "C++" {
// Launches 1 and 2 of usv_norm.hpp (nothing if the call updates no statistic).
template <typename RW>
static void norm_reduce(const NormArgs& z, const float* obs, const RW* rew, hipStream_t s) {
  if (!z.upd_obs && !z.upd_ret) return;
  const int P = norm_num_partials(z.n);
  hipLaunchKernelGGL(norm_moments_kernel<RW>, dim3(P), dim3(kBlock), 0, s, z, obs, rew);
  hipLaunchKernelGGL(norm_finalise_kernel, dim3(z.D + 1), dim3(kNormLanes), 0, s, z, P);
}

// The reset's launches; zn null: no normalisation.
template <bool MASKED>
static void wrap_reset_launch(const WrapArgs& a, const usv_norm* zn, const uint8_t* mask, const float* obs, hipStream_t s) {
  const dim3 grid = wrap_grid(a.n), block(kBlock);
  if (!zn) {
    hipLaunchKernelGGL(wrap_reset_kernel<MASKED>, grid, block, 0, s, a, mask, obs);
    return;
  }
  NormArgs z = norm_args(zn, !MASKED);                  // a masked reset updates no statistic
  z.upd_ret = 0;
  norm_reduce<float>(z, obs, nullptr, s);
  if ((zn->flags & USV_NORM_OBS) != 0)
    hipLaunchKernelGGL((wrap_reset_norm_kernel<MASKED, true>), grid, block, (size_t)16 * a.D, s, a, z, mask, obs);
  else
    hipLaunchKernelGGL((wrap_reset_norm_kernel<MASKED, false>), grid, block, 0, s, a, z, mask, obs);
}

// The step's launches; zn null: no normalisation.
template <typename RW>
static void wrap_step_launch(const WrapArgs& a, const usv_norm* zn, const float* obs, const RW* rew, const uint8_t* done,
                             const float* fobs, float* final_stack, float* norm_rew_out, hipStream_t s) {
  const dim3 grid = wrap_grid(a.n), block(kBlock);
  if (!zn) {
    hipLaunchKernelGGL(wrap_step_kernel<RW>, grid, block, 0, s, a, obs, rew, done, fobs, final_stack);
    return;
  }
  const NormArgs z = norm_args(zn, true);
  norm_reduce<RW>(z, obs, rew, s);
  if ((zn->flags & USV_NORM_OBS) != 0)
    hipLaunchKernelGGL((wrap_step_norm_kernel<RW, true>), grid, block, (size_t)16 * a.D, s, a, z, obs, rew, done, fobs,
                       final_stack, norm_rew_out);
  else
    hipLaunchKernelGGL((wrap_step_norm_kernel<RW, false>), grid, block, 0, s, a, z, obs, rew, done, fobs, final_stack,
                       norm_rew_out);
}
}

// usv_wrap_reset and, with a usv_norm that has passed norm_check, usv_wrap_reset_norm.
static int wrap_reset(const usv_wrap* w, const usv_norm* zn, int64_t j, const uint8_t* mask, const float* obs,
                      void* stream) {
  WrapArgs a;
  int dev;
  if (int rc = wrap_args(w, zn, j, {{obs, 4}, {mask, 1, true}}, a, dev)) return rc;
  DeviceGuard g(dev);
  if (mask) wrap_reset_launch<true>(a, zn, mask, obs, (hipStream_t)stream);
  else wrap_reset_launch<false>(a, zn, mask, obs, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// usv_wrap_step and, with a usv_norm that has passed norm_check, usv_wrap_step_norm.
static int wrap_step(const usv_wrap* w, const usv_norm* zn, int64_t j, const float* obs, const void* rew,
                     const uint8_t* done, const float* final_obs, float* final_stack, float* norm_rew_out, void* stream) {
  WrapArgs a;
  int dev;
  if (final_stack && !final_obs && w && w->n > 0 && w->obs_dim > 0 && w->n_stack >= 1 && w->ring)
    return fail(USV_ERR_ARG, "usv_wrap_step: final_stack needs final_obs");
  const float* const fobs = final_stack ? final_obs : nullptr;   // read only with final_stack
  const uintptr_t rb = w ? (uintptr_t)w->reward_bytes : 4;       // wrap_args refuses any but 4 and 8
  if (int rc = wrap_args(w, zn, j, {{obs, 4}, {rew, rb}, {done, 1}, {fobs, 4, true}, {final_stack, 4, true},
                                    {norm_rew_out, 4, !zn}}, a, dev))
    return rc;
  DeviceGuard g(dev);
  if (a.reward_bytes == 8)
    wrap_step_launch(a, zn, obs, (const double*)rew, done, fobs, final_stack, norm_rew_out, (hipStream_t)stream);
  else
    wrap_step_launch(a, zn, obs, (const float*)rew, done, fobs, final_stack, norm_rew_out, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_wrap_reset(const usv_wrap* w, int64_t j, const uint8_t* mask, const float* obs, void* stream) {
  return wrap_reset(w, nullptr, j, mask, obs, stream);
}

int usv_wrap_step(const usv_wrap* w, int64_t j, const float* obs, const void* rew, const uint8_t* done,
                  const float* final_obs, float* final_stack, void* stream) {
  return wrap_step(w, nullptr, j, obs, rew, done, final_obs, final_stack, nullptr, stream);
}

int usv_wrap_reset_norm(const usv_wrap* w, const usv_norm* zn, int64_t j, const uint8_t* mask, const float* obs,
                        void* stream) {
  if (int rc = norm_check(w, zn)) return rc;
  return wrap_reset(w, zn, j, mask, obs, stream);
}

int usv_wrap_step_norm(const usv_wrap* w, const usv_norm* zn, int64_t j, const float* obs, const void* rew,
                       const uint8_t* done, const float* final_obs, float* final_stack, float* norm_rew_out,
                       void* stream) {
  if (int rc = norm_check(w, zn)) return rc;
  return wrap_step(w, zn, j, obs, rew, done, final_obs, final_stack, norm_rew_out, stream);
}

// ---- device rollout buffer (usv_rollout.hpp)
size_t usv_rollout_scratch_bytes(int32_t n) {
  return n > 0 ? 2 * sizeof(long long) + (((size_t)ro_num_chunks(n) * sizeof(int32_t) + 7) & ~(size_t)7) : 0;
}

// The checks that need no HIP call, then the device of every buffer (`more`: the call's own); fills the
// kernels' arguments.
static int rollout_args(const usv_rollout* ro, bool in_range, Bufs more, RoArgs& a, int& dev) {
  if (!ro) return fail(USV_ERR_ARG, "null usv_rollout");
  if (ro->n <= 0 || ro->n_steps <= 0 || ro->obs_width <= 0 || ro->act_dim <= 0)
    return fail(USV_ERR_ARG, "usv_rollout: n, n_steps, obs_width and act_dim must be > 0");
  if (ro->term_cap < 0 || ro->reserved != 0) return fail(USV_ERR_ARG, "usv_rollout: term_cap must be >= 0 and reserved 0");
  if (!in_range) return fail(USV_ERR_ARG, "usv_rollout: t must be in [0, n_steps)");
  Buf all[kMaxBufs] = {{ro->obs, 4},   {ro->act, 4},       {ro->rew, 4},        {ro->val, 4},
                       {ro->logp, 4},  {ro->adv, 4},       {ro->ret, 4},        {ro->start, 1},
                       {ro->term_slot, 4}, {ro->term_count, 4}, {ro->scratch, 8},
                       {ro->term_cap > 0 ? (const void*)ro->term_obs : ro->obs, 4}};
  size_t nb = 12;
  if (check_bufs(all, nb) == kBufNull) return fail(USV_ERR_ARG, "usv_rollout: null buffer");
  for (const Buf& b : more) all[nb++] = b;
  if (int rc = refuse_bufs(all, nb, &dev,
                           {"usv_rollout: null argument", "usv_rollout: a buffer is not aligned to its element size",
                            "usv_rollout: obs is not a device pointer",
                            "usv_rollout: a buffer is not a device pointer on the device that holds obs"}))
    return rc;
  long long* const totals = (long long*)ro->scratch;
  a = RoArgs{ro->n, ro->n_steps, ro->obs_width, ro->act_dim, ro->term_cap, ro->obs, ro->act, ro->rew, ro->val,
             ro->logp, ro->adv, ro->ret, ro->start, ro->term_slot, ro->term_obs, ro->term_count, totals,
             (int32_t*)(totals + 2)};
  return USV_OK;
}

// usv_rollout_put_obs and, with a usv_rollout_frames that has passed rollout_frames_check and has
// frames, usv_rollout_put_obs_frames.
static int rollout_put_obs(const usv_rollout* ro, const usv_rollout_frames* fr, int32_t t, const float* obs_src,
                           size_t stride, const float* act, const float* val, const float* logp, void* stream) {
  RoArgs a;
  int dev;
  const Bufs more = {{obs_src, 4}, {act, 4}, {val, 4}, {logp, 4}};
  if (ro && ro->obs_width > 0 && stride < (size_t)ro->obs_width)
    return fail(USV_ERR_ARG, "usv_rollout_put_obs: the row stride is below obs_width");
  if (check_bufs(more) == kBufAlign) return fail(USV_ERR_ARG, "usv_rollout_put_obs: a buffer is not 4-B aligned");
  usv_rollout r;
  if (ro && fr) {
    r = *ro;
    r.obs = fr->frames;                                 // frame mode has no obs; the frames name the device
    ro = &r;
  }
  if (int rc = rollout_args(ro, ro && t >= 0 && t < ro->n_steps, more, a, dev)) return rc;
  DeviceGuard g(dev);
  const dim3 grid = wrap_grid(a.n), block(kBlock);
  if (fr) {
    const RfArgs f{fr->k, fr->d, fr->flags & USV_ROLLOUT_FRAMES_CLEAR_KEEPS_SIGN, fr->frames, fr->bad_count};
    hipLaunchKernelGGL(rollout_frames_obs_kernel, grid, block, 0, (hipStream_t)stream, a, f, (int)t, obs_src, stride, act,
                       val, logp);
  } else {
    hipLaunchKernelGGL(rollout_obs_kernel, grid, block, 0, (hipStream_t)stream, a, (int)t, obs_src, stride, act, val, logp);
  }
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_rollout_put_obs(const usv_rollout* ro, int32_t t, const float* obs_src, size_t stride, const float* act,
                        const float* val, const float* logp, void* stream) {
  return rollout_put_obs(ro, nullptr, t, obs_src, stride, act, val, logp, stream);
}

int usv_rollout_put_step(const usv_rollout* ro, int32_t t, const void* rew, int32_t reward_bytes, const uint8_t* term,
                         const uint8_t* trunc, const float* final_stack, void* stream) {
  RoArgs a;
  int dev;
  if (reward_bytes != 4 && reward_bytes != 8) return fail(USV_ERR_ARG, "usv_rollout_put_step: reward_bytes must be 4 or 8");
  if (check_bufs({{rew, (uintptr_t)reward_bytes, true}, {final_stack, 4, true}}) == kBufAlign)
    return fail(USV_ERR_ARG, "usv_rollout_put_step: a buffer is not aligned to its element size");
  const bool need_fs = ro && ro->term_cap > 0;          // without slots no terminal row is ever read
  if (int rc = rollout_args(ro, ro && t >= 0 && t < ro->n_steps,
                            {{rew, 4}, {term, 1}, {trunc, 1}, {need_fs ? (const void*)final_stack : rew, 4}}, a, dev))
    return rc;
  DeviceGuard g(dev);
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ro_num_chunks(a.n)), block(kBlock);
  hipLaunchKernelGGL(rollout_count_kernel, grid, block, 0, s, a, term, trunc);
  if (reward_bytes == 8)
    hipLaunchKernelGGL(rollout_step_kernel<double>, grid, block, 0, s, a, (int)t, (const double*)rew, term, trunc, final_stack);
  else
    hipLaunchKernelGGL(rollout_step_kernel<float>, grid, block, 0, s, a, (int)t, (const float*)rew, term, trunc, final_stack);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_rollout_gae(const usv_rollout* ro, const float* last_val, const float* term_val, double gamma,
                    double gae_lambda, void* stream) {
  RoArgs a;
  int dev;
  if (!(gamma >= 0.0 && gamma <= 1.0) || !(gae_lambda >= 0.0 && gae_lambda <= 1.0))
    return fail(USV_ERR_ARG, "usv_rollout_gae: gamma and gae_lambda must be in [0, 1]");
  if (check_bufs({{last_val, 4, true}, {term_val, 4, true}}) == kBufAlign)
    return fail(USV_ERR_ARG, "usv_rollout_gae: a buffer is not 4-B aligned");
  if (ro && ro->term_cap > 0 && !term_val) return fail(USV_ERR_ARG, "usv_rollout_gae: term_val is missing while term_cap > 0");
  if (int rc = rollout_args(ro, true, {{last_val, 4}, {term_val ? term_val : last_val, 4}}, a, dev)) return rc;
  DeviceGuard g(dev);
  const dim3 grid((a.n + kBlock - 1) / kBlock), block(kBlock);
  hipLaunchKernelGGL(rollout_gae_kernel, grid, block, 0, (hipStream_t)stream, a, last_val, term_val, ro_g32(gamma),
                     ro_gl32(gamma, gae_lambda));
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// ---- frame-deduplicated obs storage and the minibatch gather (usv_rollout_frames.hpp)
// The checks of a usv_rollout_frames against its usv_rollout that need no HIP call.
static int rollout_frames_check(const usv_rollout* ro, const usv_rollout_frames* fr) {
  if (!ro) return fail(USV_ERR_ARG, "null usv_rollout");
  if (!fr) return fail(USV_ERR_ARG, "null usv_rollout_frames");
  if (fr->k < 1 || fr->d < 1) return fail(USV_ERR_ARG, "usv_rollout_frames: k and d must be >= 1");
  if (fr->k > kRfMaxStack) return fail(USV_ERR_ARG, "usv_rollout_frames: k must be <= 32");
  if ((int64_t)fr->k * fr->d != (int64_t)ro->obs_width)
    return fail(USV_ERR_ARG, "usv_rollout_frames: k * d must equal obs_width");
  if ((fr->flags & ~USV_ROLLOUT_FRAMES_CLEAR_KEEPS_SIGN) != 0) return fail(USV_ERR_ARG, "usv_rollout_frames: unknown flags");
  if (check_bufs({{fr->frames, 4, true}, {fr->bad_count, 4, true}}) == kBufAlign)
    return fail(USV_ERR_ARG, "usv_rollout_frames: a buffer is not 4-B aligned");
  return USV_OK;
}

int usv_rollout_put_obs_frames(const usv_rollout* ro, const usv_rollout_frames* fr, int32_t t, const float* obs_src,
                               size_t stride, const float* act, const float* val, const float* logp, void* stream) {
  if (int rc = rollout_frames_check(ro, fr)) return rc;
  if (!fr->frames) return fail(USV_ERR_ARG, "usv_rollout_put_obs_frames: the rollout has no frames");
  return rollout_put_obs(ro, fr, t, obs_src, stride, act, val, logp, stream);
}

int usv_rollout_gather(const usv_rollout* ro, const usv_rollout_frames* fr, const int64_t* idx, int32_t B,
                       float* obs_out, float* act_out, float* val_out, float* logp_out, float* adv_out, float* ret_out,
                       void* stream) {
  RoArgs a;
  int dev;
  if (int rc = rollout_frames_check(ro, fr)) return rc;
  if (B <= 0) return fail(USV_ERR_ARG, "usv_rollout_gather: B must be > 0");
  if (!fr->bad_count) return fail(USV_ERR_ARG, "usv_rollout_gather: null bad_count");
  const Bufs more = {{idx, 8},     {fr->bad_count, 4}, {obs_out, 4}, {act_out, 4},
                     {val_out, 4}, {logp_out, 4},      {adv_out, 4}, {ret_out, 4}};
  if (int rc = refuse_gather_bufs("usv_rollout_gather", idx, more.begin() + 2, 6)) return rc;
  usv_rollout r = *ro;
  if (fr->frames) r.obs = fr->frames;
  if (int rc = rollout_args(&r, true, more, a, dev)) return rc;
  DeviceGuard g(dev);
  const RfArgs f{fr->k, fr->d, fr->flags & USV_ROLLOUT_FRAMES_CLEAR_KEEPS_SIGN, fr->frames, fr->bad_count};
  const int per_block = kWaves * kRfRows;
  const dim3 grid((unsigned)(((int64_t)B + per_block - 1) / per_block)), block(kBlock);
  hipLaunchKernelGGL(rollout_gather_kernel, grid, block, 0, (hipStream_t)stream, a, f, idx, (int)B, obs_out, act_out,
                     val_out, logp_out, adv_out, ret_out);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// ---- the gather a graph can replay (usv_rollout_perm.hpp)
size_t usv_rollout_cursor_bytes(void) { return sizeof(RolloutCursor); }

int usv_rollout_gather_perm(const usv_rollout* ro, const usv_rollout_frames* fr, void* cursor_dev, uint64_t seed,
                            int32_t B, int64_t* idx_out, float* obs_out, float* act_out, float* val_out,
                            float* logp_out, float* adv_out, float* ret_out, void* stream) {
  RoArgs a;
  int dev;
  const char* const fn = "usv_rollout_gather_perm";
  if (int rc = rollout_frames_check(ro, fr)) return rc;
  if (B <= 0) return fail(USV_ERR_ARG, "usv_rollout_gather_perm: B must be > 0");
  if (!fr->bad_count) return fail(USV_ERR_ARG, "usv_rollout_gather_perm: null bad_count");
  if (!cursor_dev) return fail(USV_ERR_ARG, "usv_rollout_gather_perm: null cursor block");
  if ((reinterpret_cast<uintptr_t>(cursor_dev) & 15) != 0)
    return fail(USV_ERR_ARG, "usv_rollout_gather_perm: the cursor block is not 16-B aligned");
  const Bufs more = {{cursor_dev, 16}, {fr->bad_count, 4}, {obs_out, 4},  {act_out, 4},      {val_out, 4},
                     {logp_out, 4},    {adv_out, 4},       {ret_out, 4},  {idx_out, 8, true}};
  // refuse_gather_bufs's checks, with the cursor in the place of idx (it is not null) and idx_out as it may be null
  if (int rc = refuse_gather_bufs(fn, (const int64_t*)cursor_dev, more.begin() + 2, 6)) return rc;
  if ((reinterpret_cast<uintptr_t>(idx_out) & 7) != 0) return fail(USV_ERR_ARG, "usv_rollout_gather_perm: idx_out is not 8-B aligned");
  for (const Buf* b = more.begin() + 2; b != more.end(); ++b)
    if (b->p == cursor_dev) return fail(USV_ERR_ARG, "usv_rollout_gather_perm: an output aliases the cursor block");
  if (ro->n > 0 && ro->n_steps > 0) {                   // (rollout_args refuses the rest)
    const int64_t M = (int64_t)ro->n_steps * ro->n;
    if (M % B != 0)
      return fail(USV_ERR_ARG, "usv_rollout_gather_perm: B must divide n_steps * n (a recorded graph has one shape)");
  }
  usv_rollout r = *ro;
  if (fr->frames) r.obs = fr->frames;
  if (int rc = rollout_args(&r, true, more, a, dev)) return rc;
  const int64_t batches = (int64_t)a.T * a.n / B;       // the cursor's batch word is a uint32
  if (batches > 0xffffffffll) return fail(USV_ERR_ARG, "usv_rollout_gather_perm: more than 2^32 - 1 minibatches an epoch");
  const uint32_t n_batches = (uint32_t)batches;
  DeviceGuard g(dev);
  const RfArgs f{fr->k, fr->d, fr->flags & USV_ROLLOUT_FRAMES_CLEAR_KEEPS_SIGN, fr->frames, fr->bad_count};
  const int per_block = kWaves * kRfRows;
  const dim3 grid((unsigned)(((int64_t)B + per_block - 1) / per_block)), block(kBlock);
  RolloutCursor* const cur = (RolloutCursor*)cursor_dev;
  hipLaunchKernelGGL(rollout_gather_perm_kernel, grid, block, 0, (hipStream_t)stream, a, f, (const RolloutCursor*)cur, seed,
                     n_batches, idx_out, (int)B, obs_out, act_out, val_out, logp_out, adv_out, ret_out);
  hipLaunchKernelGGL(rollout_cursor_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, cur, n_batches);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// ---- gSDE heads (usv_sde.hpp)
// The checks that need no HIP call.  sde_shape: what every entry needs of a usv_sde; sde_check: a head that draws
// noise, fills the kernels' arguments; sde_eval_check: the evaluation (the struct's n, key and bounds are not its).
static int sde_shape(const usv_sde* s) {
  if (!s) return fail(USV_ERR_ARG, "null usv_sde");
  if (s->act_dim != 1 && s->act_dim != 2) return fail(USV_ERR_ARG, "usv_sde: act_dim must be 1 or 2");
  if (!sde_latent_ok(s->latent_dim))
    return fail(USV_ERR_ARG, "usv_sde: latent_dim must be a multiple of 4 in [4, 4096]");
  if (s->reserved != 0) return fail(USV_ERR_ARG, "usv_sde: reserved must be 0");
  return USV_OK;
}

static int sde_check(const usv_sde* s, uint32_t epoch, SdeArgs& a) {
  if (s && s->n <= 0) return fail(USV_ERR_ARG, "usv_sde: n must be > 0");
  if (int rc = sde_shape(s)) return rc;
  for (int k = 0; k < s->act_dim; ++k)
    if (!(s->low[k] <= s->high[k])) return fail(USV_ERR_ARG, "usv_sde: low must be <= high (and neither NaN)");
  a = SdeArgs{s->n, s->latent_dim, epoch, s->seed, s->gid0, {s->low[0], s->low[1]}, {s->high[0], s->high[1]}};
  return USV_OK;
}

static int sde_eval_check(const usv_sde* s, int32_t rows) {
  if (int rc = sde_shape(s)) return rc;
  if (rows <= 0) return fail(USV_ERR_ARG, "usv_sde_eval: rows must be > 0");
  return USV_OK;
}

// A row stride (`what`: which, where an entry has two) of entry `fn`.
static int sde_stride(const usv_sde* s, size_t stride, const char* fn, const char* what = "") {
  if (stride >= (size_t)s->latent_dim && stride % 4 == 0) return USV_OK;
  return fail(USV_ERR_ARG, std::string(fn) + ": the " + what + "row stride must be a multiple of 4 and >= latent_dim");
}

static int sde_bufs(const Buf* b, size_t nb, int& dev) { return refuse_bufs(b, nb, dev, "usv_sde", "lat"); }

static size_t sde_scratch_floats(int64_t rows, const usv_sde* s) {
  return (size_t)sde_partials(rows) * (size_t)s->latent_dim * (size_t)s->act_dim;
}

static int64_t sde_wave_blocks(int64_t waves) { return (waves + kWaves - 1) / kWaves; }

extern "C++" {
// k1 / k2, the kernel's act_dim = 1 / 2 instance, on `blocks` blocks.
template <class K, class... Q>
static int sde_launch(const usv_sde* s, K k1, K k2, int64_t blocks, void* stream, Q... args) {
  hipLaunchKernelGGL(s->act_dim == 1 ? k1 : k2, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, args...);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// A backward of `rows` rows, a wave per partial, then g_std from the partials in scratch.
template <class K, class... Q>
static int sde_launch_backward(const usv_sde* s, K k1, K k2, int64_t rows, float* scratch, float* g_std, void* stream,
                               Q... args) {
  const int partials = (int)sde_partials(rows), LA = s->latent_dim * s->act_dim;
  if (int rc = sde_launch(s, k1, k2, sde_wave_blocks(partials), stream, args...)) return rc;
  hipLaunchKernelGGL(sde_std_finalise_kernel, dim3((unsigned)((LA + 15) / 16)), dim3(kBlock), 0, (hipStream_t)stream,
                     partials, LA, scratch, g_std);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}
}  // extern "C++"

// The four entries that draw noise, each behind its two forms: the epoch an argument (epoch_dev null), or a word in
// device memory that the kernel reads (the _dev entries; `epoch` is then not used).
static int sde_sample(const usv_sde* s, uint32_t epoch, const uint32_t* epoch_dev, const float* mean, const float* lat,
                      size_t stride, const float* std, float* act, float* act_env, float* logp, void* stream) {
  SdeArgs a;
  int dev;
  if (int rc = sde_check(s, epoch, a)) return rc;
  if (int rc = sde_stride(s, stride, "usv_sde_sample")) return rc;
  const Buf all[] = {{lat, 16}, {mean, 4}, {std, 4}, {act, 4}, {act_env, 4}, {logp, 4}, {epoch_dev, 4, true}};
  if (int rc = sde_bufs(all, 7, dev)) return rc;
  DeviceGuard g(dev);
  const int64_t blocks = sde_wave_blocks(a.n);
  if (epoch_dev)
    return sde_launch(s, sde_sample_dev_kernel<1>, sde_sample_dev_kernel<2>, blocks, stream, a, epoch_dev, mean, lat,
                      stride, std, act, act_env, logp);
  return sde_launch(s, sde_sample_kernel<1>, sde_sample_kernel<2>, blocks, stream, a, mean, lat, stride, std, act,
                    act_env, logp);
}

int usv_sde_sample(const usv_sde* s, uint32_t epoch, const float* mean, const float* lat, size_t stride,
                   const float* std, float* act, float* act_env, float* logp, void* stream) {
  return sde_sample(s, epoch, nullptr, mean, lat, stride, std, act, act_env, logp, stream);
}

int usv_sde_sample_dev(const usv_sde* s, const uint32_t* epoch_dev, const float* mean, const float* lat, size_t stride,
                       const float* std, float* act, float* act_env, float* logp, void* stream) {
  if (int rc = refuse_word("usv_sde_sample_dev", "epoch_dev", epoch_dev)) return rc;
  return sde_sample(s, 0u, epoch_dev, mean, lat, stride, std, act, act_env, logp, stream);
}

static int sde_weights(const usv_sde* s, uint32_t epoch, const uint32_t* epoch_dev, const float* std, float* w,
                       void* stream) {
  SdeArgs a;
  int dev;
  if (int rc = sde_check(s, epoch, a)) return rc;
  const int64_t threads = (int64_t)a.n * (a.L * s->act_dim / 4);
  if ((threads + kBlock - 1) / kBlock > 2147483647)
    return fail(USV_ERR_ARG, "usv_sde_weights: n * latent_dim * act_dim / 4 is above 2^31 - 1 blocks of 256");
  const Buf all[] = {{w, 4}, {std, 4}, {epoch_dev, 4, true}};
  if (int rc = sde_bufs(all, 3, dev)) return rc;
  DeviceGuard g(dev);
  const int64_t blocks = (threads + kBlock - 1) / kBlock;
  if (epoch_dev)
    return sde_launch(s, sde_weights_dev_kernel<1>, sde_weights_dev_kernel<2>, blocks, stream, a, epoch_dev, std, w);
  return sde_launch(s, sde_weights_kernel<1>, sde_weights_kernel<2>, blocks, stream, a, std, w);
}

int usv_sde_weights(const usv_sde* s, uint32_t epoch, const float* std, float* w, void* stream) {
  return sde_weights(s, epoch, nullptr, std, w, stream);
}

int usv_sde_weights_dev(const usv_sde* s, const uint32_t* epoch_dev, const float* std, float* w, void* stream) {
  if (int rc = refuse_word("usv_sde_weights_dev", "epoch_dev", epoch_dev)) return rc;
  return sde_weights(s, 0u, epoch_dev, std, w, stream);
}

static int sde_squash_forward(const usv_sde* s, uint32_t epoch, const uint32_t* epoch_dev, const float* mean,
                              const float* lat, size_t stride, const float* std, float* act, float* act_env,
                              float* logp, float* gauss, float* var, void* stream) {
  SdeArgs a;
  int dev;
  if (int rc = sde_check(s, epoch, a)) return rc;
  if (int rc = sde_stride(s, stride, "usv_sde_squash_forward")) return rc;
  if ((gauss == nullptr) != (var == nullptr))
    return fail(USV_ERR_ARG, "usv_sde_squash_forward: gauss and var must be both NULL or both set");
  const Buf all[] = {{lat, 16}, {mean, 4}, {std, 4}, {act, 4}, {act_env, 4}, {logp, 4}, {gauss, 4, true}, {var, 4, true},
                     {epoch_dev, 4, true}};
  if (int rc = sde_bufs(all, 9, dev)) return rc;
  DeviceGuard g(dev);
  const int64_t blocks = sde_wave_blocks(a.n);
  if (epoch_dev)
    return sde_launch(s, sde_squash_forward_dev_kernel<1>, sde_squash_forward_dev_kernel<2>, blocks, stream, a,
                      epoch_dev, mean, lat, stride, std, act, act_env, logp, gauss, var);
  return sde_launch(s, sde_squash_forward_kernel<1>, sde_squash_forward_kernel<2>, blocks, stream, a, mean, lat, stride,
                    std, act, act_env, logp, gauss, var);
}

int usv_sde_squash_forward(const usv_sde* s, uint32_t epoch, const float* mean, const float* lat, size_t stride,
                           const float* std, float* act, float* act_env, float* logp, float* gauss, float* var,
                           void* stream) {
  return sde_squash_forward(s, epoch, nullptr, mean, lat, stride, std, act, act_env, logp, gauss, var, stream);
}

int usv_sde_squash_forward_dev(const usv_sde* s, const uint32_t* epoch_dev, const float* mean, const float* lat,
                               size_t stride, const float* std, float* act, float* act_env, float* logp, float* gauss,
                               float* var, void* stream) {
  if (int rc = refuse_word("usv_sde_squash_forward_dev", "epoch_dev", epoch_dev)) return rc;
  return sde_squash_forward(s, 0u, epoch_dev, mean, lat, stride, std, act, act_env, logp, gauss, var, stream);
}

size_t usv_sde_squash_scratch_floats(const usv_sde* s) {
  SdeArgs a;
  return sde_check(s, 0u, a) ? 0 : sde_scratch_floats(a.n, s);
}

static int sde_squash_backward(const usv_sde* s, uint32_t epoch, const uint32_t* epoch_dev, const float* mean,
                               const float* lat, size_t stride, const float* std, const float* gauss, const float* var,
                               const float* g_act, const float* g_logp, float* g_mean, float* g_lat, size_t g_stride,
                               float* g_std, float* scratch, void* stream) {
  SdeArgs a;
  int dev;
  if (int rc = sde_check(s, epoch, a)) return rc;
  if (int rc = sde_stride(s, stride, "usv_sde_squash_backward")) return rc;
  if (int rc = sde_stride(s, g_stride, "usv_sde_squash_backward", "g_lat ")) return rc;
  if (!scratch) return fail(USV_ERR_ARG, "usv_sde_squash_backward: null scratch");
  const Buf all[] = {{lat, 16},  {g_lat, 16}, {scratch, 16},      {mean, 4},           {std, 4},   {gauss, 4},
                     {var, 4},   {g_mean, 4}, {g_act, 4, true},   {g_logp, 4, true},   {g_std, 4}, {epoch_dev, 4, true}};
  if (int rc = sde_bufs(all, 12, dev)) return rc;
  DeviceGuard g(dev);
  const int R = (int)sde_rows_per_partial(a.n);
  if (epoch_dev)
    return sde_launch_backward(s, sde_squash_backward_dev_kernel<1>, sde_squash_backward_dev_kernel<2>, a.n, scratch,
                               g_std, stream, a, epoch_dev, R, mean, lat, stride, std, gauss, var, g_act, g_logp, g_mean,
                               g_lat, g_stride, scratch);
  return sde_launch_backward(s, sde_squash_backward_kernel<1>, sde_squash_backward_kernel<2>, a.n, scratch, g_std,
                             stream, a, R, mean, lat, stride, std, gauss, var, g_act, g_logp, g_mean, g_lat, g_stride,
                             scratch);
}

int usv_sde_squash_backward(const usv_sde* s, uint32_t epoch, const float* mean, const float* lat, size_t stride,
                            const float* std, const float* gauss, const float* var, const float* g_act,
                            const float* g_logp, float* g_mean, float* g_lat, size_t g_stride, float* g_std,
                            float* scratch, void* stream) {
  return sde_squash_backward(s, epoch, nullptr, mean, lat, stride, std, gauss, var, g_act, g_logp, g_mean, g_lat,
                             g_stride, g_std, scratch, stream);
}

int usv_sde_squash_backward_dev(const usv_sde* s, const uint32_t* epoch_dev, const float* mean, const float* lat,
                                size_t stride, const float* std, const float* gauss, const float* var,
                                const float* g_act, const float* g_logp, float* g_mean, float* g_lat, size_t g_stride,
                                float* g_std, float* scratch, void* stream) {
  if (int rc = refuse_word("usv_sde_squash_backward_dev", "epoch_dev", epoch_dev)) return rc;
  return sde_squash_backward(s, 0u, epoch_dev, mean, lat, stride, std, gauss, var, g_act, g_logp, g_mean, g_lat,
                             g_stride, g_std, scratch, stream);
}

int usv_sde_eval_forward(const usv_sde* s, int32_t rows, const float* mean, const float* lat, size_t stride,
                         const float* std, const float* act, const float* old_logp, const float* adv, float clip,
                         float* logp, float* sur, float* ratio, float* var, void* stream) {
  int dev;
  if (int rc = sde_eval_check(s, rows)) return rc;
  if (int rc = sde_stride(s, stride, "usv_sde_eval_forward")) return rc;
  const bool ppo = old_logp != nullptr;
  if ((adv != nullptr) != ppo || (sur != nullptr) != ppo || (ratio != nullptr) != ppo)
    return fail(USV_ERR_ARG, "usv_sde_eval_forward: old_logp, adv, sur and ratio must be all NULL or all set");
  if (ppo && !(clip >= 0.0f)) return fail(USV_ERR_ARG, "usv_sde_eval_forward: clip must be >= 0 (and not NaN)");
  const Buf all[] = {{lat, 16},          {mean, 4},     {std, 4},      {act, 4},        {logp, 4},
                     {old_logp, 4, true}, {adv, 4, true}, {sur, 4, true}, {ratio, 4, true}, {var, 4, true}};
  if (int rc = sde_bufs(all, 10, dev)) return rc;
  DeviceGuard g(dev);
  return sde_launch(s, sde_eval_forward_kernel<1>, sde_eval_forward_kernel<2>, sde_wave_blocks(rows), stream,
                    (int)rows, s->latent_dim, mean, lat, stride, std, act, old_logp, adv, clip, logp, sur, ratio, var);
}

size_t usv_sde_eval_scratch_floats(const usv_sde* s, int32_t rows) {
  return sde_eval_check(s, rows) ? 0 : sde_scratch_floats(rows, s);
}

int usv_sde_eval_backward(const usv_sde* s, int32_t rows, const float* mean, const float* lat, size_t stride,
                          const float* std, const float* act, const float* var, const float* ratio, const float* adv,
                          float clip, const float* g_logp, const float* g_sur, float* g_mean, float* g_lat,
                          size_t g_stride, float* g_std, float* scratch, void* stream) {
  int dev;
  if (int rc = sde_eval_check(s, rows)) return rc;
  if (int rc = sde_stride(s, stride, "usv_sde_eval_backward")) return rc;
  if (g_lat)
    if (int rc = sde_stride(s, g_stride, "usv_sde_eval_backward", "g_lat ")) return rc;
  if ((ratio != nullptr) != (adv != nullptr))
    return fail(USV_ERR_ARG, "usv_sde_eval_backward: ratio and adv must be both NULL or both set");
  if (g_sur && !ratio) return fail(USV_ERR_ARG, "usv_sde_eval_backward: g_sur needs ratio and adv");
  if (ratio && !(clip >= 0.0f)) return fail(USV_ERR_ARG, "usv_sde_eval_backward: clip must be >= 0 (and not NaN)");
  if (!scratch) return fail(USV_ERR_ARG, "usv_sde_eval_backward: null scratch");
  const Buf all[] = {{lat, 16},       {g_lat, 16, true}, {scratch, 16},     {mean, 4},          {std, 4},
                     {act, 4},        {var, 4},          {g_mean, 4},       {g_std, 4},         {ratio, 4, true},
                     {adv, 4, true},  {g_logp, 4, true}, {g_sur, 4, true}};
  if (int rc = sde_bufs(all, 13, dev)) return rc;
  DeviceGuard g(dev);
  return sde_launch_backward(s, sde_eval_backward_kernel<1>, sde_eval_backward_kernel<2>, rows, scratch, g_std,
                             stream, (int)rows, s->latent_dim, (int)sde_rows_per_partial(rows), mean, lat, stride, std, act,
                             var, ratio, adv, clip, g_logp, g_sur, g_mean, g_lat, g_stride, scratch);
}

// ---- device replay buffer (usv_replay.hpp)
// The checks that need no HIP call, then the device of every buffer (`more`: the call's own); fills the
// kernels' arguments.
static int replay_args(const usv_replay* rp, Bufs more, RpArgs& a, int& dev) {
  if (!rp) return fail(USV_ERR_ARG, "null usv_replay");
  if (rp->n <= 0 || rp->rows <= 0 || rp->obs_width <= 0 || rp->act_dim <= 0)
    return fail(USV_ERR_ARG, "usv_replay: n, rows, obs_width and act_dim must be > 0");
  if (rp->k < 1 || rp->k > kRfMaxStack || rp->d < 1) return fail(USV_ERR_ARG, "usv_replay: k must be in [1, 32] and d >= 1");
  if ((int64_t)rp->k * rp->d != (int64_t)rp->obs_width) return fail(USV_ERR_ARG, "usv_replay: k * d must equal obs_width");
  if ((rp->flags & ~USV_REPLAY_CLEAR_KEEPS_SIGN) != 0 || rp->reserved != 0) return fail(USV_ERR_ARG, "usv_replay: unknown flags");
  if (rp_frame_rows(rp->rows, rp->k) > 2147483647) return fail(USV_ERR_ARG, "usv_replay: rows + k - 1 must be below 2^31");
  Buf all[kMaxBufs] = {{rp->frames, 4}, {rp->next_frame, 4}, {rp->act, 4},     {rp->rew, 4},      {rp->done, 1},
                       {rp->timeout, 1}, {rp->age, 1},       {rp->age_now, 1}, {rp->bad_count, 4}};
  size_t nb = 9;
  if (int rc = refuse_bufs(all, nb, nullptr,
                           {"usv_replay: null buffer", "usv_replay: a buffer is not aligned to its element size"}))
    return rc;
  for (const Buf& b : more) all[nb++] = b;
  if (int rc = refuse_bufs(all, nb, &dev,
                           {"usv_replay: null argument", "usv_replay: an argument is not aligned to its element size",
                            "usv_replay: frames is not a device pointer",
                            "usv_replay: a buffer is not a device pointer on the device that holds frames"}))
    return rc;
  a = RpArgs{rp->n, rp->rows, rp->obs_width, rp->act_dim, rp->k, rp->d, rp->flags & USV_REPLAY_CLEAR_KEEPS_SIGN,
             (int)rp_frame_rows(rp->rows, rp->k), rp->frames, rp->next_frame, rp->act, rp->rew, rp->done, rp->timeout,
             rp->age, rp->age_now, rp->bad_count};
  return USV_OK;
}

int usv_replay_put_obs(const usv_replay* rp, int64_t c, const float* stacked, size_t stride, const float* act,
                       void* stream) {
  RpArgs a;
  int dev;
  if (c < 0) return fail(USV_ERR_ARG, "usv_replay_put_obs: the step number c must be >= 0");
  if (rp && rp->obs_width > 0 && stride < (size_t)rp->obs_width)
    return fail(USV_ERR_ARG, "usv_replay_put_obs: the row stride is below obs_width");
  if (int rc = replay_args(rp, {{stacked, 4}, {act, 4}}, a, dev)) return rc;
  DeviceGuard g(dev);
  hipLaunchKernelGGL(replay_obs_kernel, wrap_grid(a.n), dim3(kBlock), 0, (hipStream_t)stream, a, (int)rp_slot(c, a.R),
                     (int)rp_frame_row(c, a.P), (int)(c == 0), stacked, stride, act);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_replay_put_step(const usv_replay* rp, int64_t c, const void* rew, int32_t reward_bytes, const uint8_t* term,
                        const uint8_t* trunc, const float* next_stacked, size_t next_stride, const float* final_stack,
                        void* stream) {
  RpArgs a;
  int dev;
  if (c < 0) return fail(USV_ERR_ARG, "usv_replay_put_step: the step number c must be >= 0");
  if (reward_bytes != 4 && reward_bytes != 8) return fail(USV_ERR_ARG, "usv_replay_put_step: reward_bytes must be 4 or 8");
  if (rp && rp->obs_width > 0 && next_stride < (size_t)rp->obs_width)
    return fail(USV_ERR_ARG, "usv_replay_put_step: the row stride is below obs_width");
  if (int rc = replay_args(rp, {{rew, (uintptr_t)reward_bytes}, {term, 1}, {trunc, 1}, {next_stacked, 4}, {final_stack, 4}},
                           a, dev))
    return rc;
  DeviceGuard g(dev);
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid = wrap_grid(a.n), block(kBlock);
  const int slot = rp_slot(c, a.R);
  if (reward_bytes == 8)
    hipLaunchKernelGGL(replay_step_kernel<double>, grid, block, 0, s, a, slot, (const double*)rew, term, trunc, next_stacked,
                       next_stride, final_stack);
  else
    hipLaunchKernelGGL(replay_step_kernel<float>, grid, block, 0, s, a, slot, (const float*)rew, term, trunc, next_stacked,
                       next_stride, final_stack);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// usv_replay_gather (fn names it; n_steps, table and discount_out are not looked at) and, with nstep,
// usv_replay_gather_nstep.
static int replay_gather(const char* fn, bool nstep, const usv_replay* rp, int64_t count, const int64_t* idx, int32_t B,
                         int32_t n_steps, const float* table, float* obs_out, float* act_out, float* next_obs_out,
                         float* done_out, float* rew_out, float* discount_out, void* stream) {
  RpArgs a;
  int dev;
  const std::string p = std::string(fn) + ": ";
  if (count < 0) return fail(USV_ERR_ARG, p + "count must be >= 0");
  if (B <= 0) return fail(USV_ERR_ARG, p + "B must be > 0");
  RpDiscounts tab = {};
  if (nstep) {
    if (n_steps < 1 || n_steps > kRpMaxNStep) return fail(USV_ERR_ARG, p + "n_steps must be in [1, 32]");
    if (!table) return fail(USV_ERR_ARG, p + "null discount table");
    for (int j = 0; j <= n_steps; ++j) {
      if (!std::isfinite(table[j])) return fail(USV_ERR_ARG, p + "a discount table entry is not finite");
      tab.g[j] = table[j];
    }
  }
  const Bufs more = {{idx, 8},      {obs_out, 4}, {act_out, 4},           {next_obs_out, 4},
                     {done_out, 4}, {rew_out, 4}, {discount_out, 4, !nstep}};
  if (int rc = refuse_gather_bufs(fn, idx, more.begin() + 1, 6)) return rc;
  if (int rc = replay_args(rp, more, a, dev)) return rc;
  DeviceGuard g(dev);
  const int per_block = kWaves * kRpRows;
  const dim3 grid((unsigned)(((int64_t)B + per_block - 1) / per_block)), block(kBlock);
  const RpLaps laps = rp_laps(count, a.R, a.k);
  const long long size = rp_size(count, a.R);
  if (nstep)
    hipLaunchKernelGGL(replay_gather_nstep_kernel, grid, block, 0, (hipStream_t)stream, a, laps, size, idx, (int)B,
                       (int)n_steps, tab, obs_out, act_out, next_obs_out, done_out, rew_out, discount_out);
  else
    hipLaunchKernelGGL(replay_gather_kernel, grid, block, 0, (hipStream_t)stream, a, laps, size, idx, (int)B, obs_out,
                       act_out, next_obs_out, done_out, rew_out);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_replay_gather(const usv_replay* rp, int64_t count, const int64_t* idx, int32_t B, float* obs_out, float* act_out,
                      float* next_obs_out, float* done_out, float* rew_out, void* stream) {
  return replay_gather("usv_replay_gather", false, rp, count, idx, B, 0, nullptr, obs_out, act_out, next_obs_out,
                       done_out, rew_out, nullptr, stream);
}

int usv_replay_gather_nstep(const usv_replay* rp, int64_t count, const int64_t* idx, int32_t B, int32_t n_steps,
                            const float* table, float* obs_out, float* act_out, float* next_obs_out, float* done_out,
                            float* rew_out, float* discount_out, void* stream) {
  return replay_gather("usv_replay_gather_nstep", true, rp, count, idx, B, n_steps, table, obs_out, act_out,
                       next_obs_out, done_out, rew_out, discount_out, stream);
}

// ---- fused SAC update (usv_sac.hpp)
static int sac_bufs(const Buf* b, size_t nb, int& dev) { return refuse_bufs(b, nb, dev, "usv_sac", "scratch"); }

size_t usv_sac_scratch_floats(int32_t rows) { return rows >= 1 ? sac_scratch_floats(rows) : 0; }

int usv_sac_critic_loss(int32_t rows, const float* q1, const float* q2, const float* q1_next, const float* q2_next,
                        const float* rewards, const float* dones, const float* ent, const float* logp_next,
                        const float* discounts, float gamma, float* target, float* loss, float* g_q1, float* g_q2,
                        float* scratch, void* stream) {
  int dev;
  if (rows < 1) return fail(USV_ERR_ARG, "usv_sac_critic_loss: rows must be >= 1");
  if ((ent != nullptr) != (logp_next != nullptr))
    return fail(USV_ERR_ARG, "usv_sac_critic_loss: ent and logp_next must be both NULL or both set");
  const Buf all[] = {{scratch, 16},    {q1, 4},       {q2, 4},           {q1_next, 4},        {q2_next, 4},
                     {rewards, 4},     {dones, 4},    {target, 4},       {loss, 4},           {ent, 4, true},
                     {logp_next, 4, true}, {discounts, 4, true}, {g_q1, 4, true}, {g_q2, 4, true}};
  if (int rc = sac_bufs(all, 14, dev)) return rc;
  DeviceGuard g(dev);
  const SacCriticArgs a{rows, q1, q2, q1_next, q2_next, rewards, dones, ent, logp_next, discounts, gamma,
                        target, loss, g_q1, g_q2, scratch};
  hipLaunchKernelGGL(sac_critic_kernel, dim3((unsigned)sac_partials(rows)), dim3(kBlock), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_sac_policy_loss(int32_t rows, const float* logp, const float* q1_pi, const float* q2_pi, const float* ent,
                        const float* log_ent, float target_entropy, float* actor_loss, float* ent_loss, float* g_logp,
                        float* g_q1, float* g_q2, float* g_log_ent, float* scratch, void* stream) {
  int dev;
  if (rows < 1) return fail(USV_ERR_ARG, "usv_sac_policy_loss: rows must be >= 1");
  if (log_ent && !ent_loss) return fail(USV_ERR_ARG, "usv_sac_policy_loss: log_ent needs ent_loss");
  const Buf all[] = {{scratch, 16},      {logp, 4},          {q1_pi, 4},        {q2_pi, 4},       {ent, 4},
                     {actor_loss, 4},    {log_ent, 4, true}, {ent_loss, 4, true}, {g_logp, 4, true}, {g_q1, 4, true},
                     {g_q2, 4, true},    {g_log_ent, 4, true}};
  if (int rc = sac_bufs(all, 12, dev)) return rc;
  DeviceGuard g(dev);
  const SacPolicyArgs a{rows, logp, q1_pi, q2_pi, ent, log_ent, target_entropy, actor_loss, ent_loss, g_logp,
                        g_q1, g_q2, g_log_ent, scratch};
  hipLaunchKernelGGL(sac_policy_kernel, dim3((unsigned)sac_partials(rows)), dim3(kBlock), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_sac_loss_backward(int32_t rows, const float* up, const float* g1, const float* g2, const float* g3, float* o1,
                          float* o2, float* o3, const float* up_s, const float* gs, float* os, void* stream) {
  int dev;
  if (rows < 1) return fail(USV_ERR_ARG, "usv_sac_loss_backward: rows must be >= 1");
  if ((o2 && !g2) || (o3 && !g3) || (os && !gs))
    return fail(USV_ERR_ARG, "usv_sac_loss_backward: an output is given without its unit gradient");
  const Buf all[] = {{o1, 4},       {g1, 4},       {up, 4, true},   {g2, 4, true}, {g3, 4, true}, {o2, 4, true},
                     {o3, 4, true}, {up_s, 4, true}, {gs, 4, true}, {os, 4, true}};
  if (int rc = sac_bufs(all, 10, dev)) return rc;
  DeviceGuard g(dev);
  const SacScaleArgs a{rows, up, {g1, g2, g3}, {o1, o2, o3}, up_s, gs, os};
  hipLaunchKernelGGL(sac_scale_kernel, dim3((unsigned)(((int64_t)rows + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// ---- CAPS regulariser (usv_caps.hpp)
static int caps_bufs(const Buf* b, size_t nb, int& dev) { return refuse_bufs(b, nb, dev, "usv_caps", "scratch"); }

// usv_caps_perturb's two forms, as the gSDE entries have them.
static int caps_perturb(const char* fn, int32_t rows, int32_t width, const float* obs, float* out, float eps,
                        uint64_t seed, uint32_t epoch, const uint32_t* epoch_dev, void* stream) {
  int dev;
  const std::string p = std::string(fn) + ": ";
  if (rows < 1) return fail(USV_ERR_ARG, p + "rows must be >= 1");
  if (width < 1) return fail(USV_ERR_ARG, p + "width must be >= 1");
  if ((int64_t)rows * width > 2147483647) return fail(USV_ERR_ARG, p + "rows * width is above 2^31 - 1");
  if (!caps_weight_ok(eps)) return fail(USV_ERR_ARG, p + "eps must be finite and >= 0");
  const Buf all[] = {{obs, 4}, {out, 4}, {epoch_dev, 4, true}};
  if (int rc = caps_bufs(all, 3, dev)) return rc;
  DeviceGuard g(dev);
  const int row_blocks = (int)caps_row_blocks(width);
  const CapsPerturbArgs a{(long long)rows * row_blocks, width, row_blocks, obs, out, eps, seed, epoch};
  const dim3 grid((unsigned)((a.blocks + kBlock - 1) / kBlock));
  if (epoch_dev)
    hipLaunchKernelGGL(caps_perturb_dev_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a, epoch_dev);
  else
    hipLaunchKernelGGL(caps_perturb_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_caps_perturb(int32_t rows, int32_t width, const float* obs, float* out, float eps, uint64_t seed, uint32_t epoch,
                     void* stream) {
  return caps_perturb("usv_caps_perturb", rows, width, obs, out, eps, seed, epoch, nullptr, stream);
}

int usv_caps_perturb_dev(int32_t rows, int32_t width, const float* obs, float* out, float eps, uint64_t seed,
                         const uint32_t* epoch_dev, void* stream) {
  if (int rc = refuse_word("usv_caps_perturb_dev", "epoch_dev", epoch_dev)) return rc;
  return caps_perturb("usv_caps_perturb_dev", rows, width, obs, out, eps, seed, 0u, epoch_dev, stream);
}

int usv_caps_loss(int32_t rows, int32_t act_dim, int32_t squash, const float* mean, const float* mean_next,
                  const float* mean_near, float lambda_t, float lambda_s, float* out3, float* g_mean, float* g_next,
                  float* g_near, float* scratch, void* stream) {
  int dev;
  if (rows < 1) return fail(USV_ERR_ARG, "usv_caps_loss: rows must be >= 1");
  if (!caps_act_ok(act_dim)) return fail(USV_ERR_ARG, "usv_caps_loss: act_dim must be in [1, 8]");
  if ((int64_t)rows * act_dim > 2147483647) return fail(USV_ERR_ARG, "usv_caps_loss: rows * act_dim is above 2^31 - 1");
  if (!caps_weight_ok(lambda_t)) return fail(USV_ERR_ARG, "usv_caps_loss: lambda_t must be finite and >= 0");
  if (!caps_weight_ok(lambda_s)) return fail(USV_ERR_ARG, "usv_caps_loss: lambda_s must be finite and >= 0");
  const Buf all[] = {{scratch, 16}, {mean, 4}, {mean_next, 4}, {mean_near, 4}, {out3, 4},
                     {g_mean, 4, true}, {g_next, 4, true}, {g_near, 4, true}};
  if (int rc = caps_bufs(all, 8, dev)) return rc;
  DeviceGuard g(dev);
  const CapsLossArgs a{rows, squash != 0, mean, mean_next, mean_near, lambda_t, lambda_s, out3, g_mean, g_next, g_near,
                       scratch};
  hipLaunchKernelGGL(kCapsLossKernels[act_dim - 1], dim3((unsigned)sac_partials(rows)), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// ---- kernels over a tensor list (usv_optim.hpp): Polyak's pairs and Adam's tensors behind one walk
// One tensor of either list, as the table has it: what the kernels write, what they read.
struct ListItem {
  float* p;
  const float* g;
  int64_t numel;
};
static ListItem list_item(const usv_polyak_pair& x) { return {x.dst, x.src, x.numel}; }
static ListItem list_item(const usv_adam_tensor& x) { return {x.param, x.grad, x.numel}; }

// The words of an entry's refusals: its name, its list, the list's length and its struct's two pointers.
struct ListWords {
  const char *fn, *list, *n, *a, *b;
};
static const ListWords kPolyakWords = {"usv_polyak_update","pairs", "n_pairs", "src", "dst"};
static const ListWords kAdamWords = {"usv_adam_step", "tensors", "n", "param", "grad"};

extern "C++" {
// The tensors that hold elements, their chunks and their state floats; a refusal's message, or none.  With
// pointers: they are looked at too.
template <class T>
static std::string list_count(const ListWords& w, const T* ts, int32_t n, bool pointers, int64_t& live, int64_t& chunks,
                              int64_t& state) {
  const std::string p = std::string(w.fn) + ": ", ab = std::string(w.a) + " or " + w.b;
  live = chunks = state = 0;
  if (!ts) return p + "null " + w.list;
  if (n < 1) return p + w.n + " must be >= 1";
  for (int32_t i = 0; i < n; ++i) {
    const ListItem t = list_item(ts[i]);
    if (t.numel < 0) return p + "numel must be >= 0";
    if (t.numel == 0) continue;
    if (pointers) {
      if (!t.p || !t.g) return p + "null " + ab;
      if (((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g)) & 3) != 0) return p + ab + " is not 4-B aligned";
      if (t.p == t.g) return p + w.a + " and " + w.b + " are the same address";
    }
    ++live;
    chunks += optim_chunks(t.numel);
    state += optim_state_floats(t.numel);
  }
  if (chunks > 2147483647) return p + "above 2^31 - 1 chunks of 4096 elements";
  return {};
}

// The pointers of the tensors that hold elements, behind those already in bufs.
template <class T>
static void list_bufs(const T* ts, int32_t n, std::vector<Buf>& bufs) {
  for (int32_t i = 0; i < n; ++i)
    if (const ListItem t = list_item(ts[i]); t.numel > 0) {
      bufs.push_back(Buf{t.p, 4});
      bufs.push_back(Buf{t.g, 4});
    }
}

// One pass: launch(tab, grid) for the list in launches of at most kTableTensors tensors, chunks and state offsets
// running through.
template <class T, class L>
static void list_pass(const T* ts, int32_t n, L&& launch) {
  TensorTable tab;
  int64_t chunk = 0, at = 0;
  tab.n = 0;
  for (int32_t i = 0; i <= n; ++i) {
    if (i < n && ts[i].numel > 0) {
      const ListItem t = list_item(ts[i]);
      const int k = tab.n++;
      tab.p[k] = t.p;
      tab.g[k] = t.g;
      tab.numel[k] = (long long)t.numel;
      tab.state[k] = (long long)at;
      tab.first[k] = (int)chunk;
      chunk += optim_chunks(t.numel);
      at += optim_state_floats(t.numel);
    }
    if (tab.n == kTableTensors || (i == n && tab.n > 0)) {
      tab.first[tab.n] = (int)chunk;
      launch(tab, dim3((unsigned)(chunk - tab.first[0])));
      tab.n = 0;
    }
  }
}
}  // extern "C++"

static size_t polyak_bytes(int64_t live, int64_t chunks) {
  return (size_t)live * sizeof(PolyakPair) + (size_t)chunks * sizeof(PolyakChunk);
}

size_t usv_polyak_table_bytes(const usv_polyak_pair* pairs, int32_t n_pairs) {
  int64_t live, chunks, state;
  return list_count(kPolyakWords, pairs, n_pairs, true, live, chunks, state).empty() ? polyak_bytes(live, chunks) : 0;
}

// usv_polyak_update (step) and usv_polyak_prepare (the upload alone; tau is then not looked at, nothing is launched).
static int polyak_call(const char* fn, const usv_polyak_pair* pairs, int32_t n_pairs, void* table, size_t table_bytes,
                       bool upload, bool step, double tau, void* stream) {
  int64_t live, chunks, state;
  int dev;
  const std::string p = std::string(fn) + ": ";
  ListWords words = kPolyakWords;
  words.fn = fn;
  if (const std::string why = list_count(words, pairs, n_pairs, true, live, chunks, state); !why.empty())
    return fail(USV_ERR_ARG, why);
  if (step && !polyak_tau_ok(tau)) return fail(USV_ERR_ARG, p + "tau must be in [0, 1]");
  if (live == 0) return USV_OK;
  if (!table) return fail(USV_ERR_ARG, p + "null table");
  if ((reinterpret_cast<uintptr_t>(table) & 7) != 0) return fail(USV_ERR_ARG, p + "the table is not 8-B aligned");
  if (table_bytes < polyak_bytes(live, chunks)) return fail(USV_ERR_ARG, p + "the table is too small");
  std::vector<Buf> bufs = {{table, 8}};
  if (upload) list_bufs(pairs, n_pairs, bufs);
  if (check_bufs(bufs.data(), bufs.size(), &dev) == kBufDevice)
    return fail(USV_ERR_ARG, p + (dev < 0 ? "the table is not a device pointer"
                                          : "a tensor is not a device pointer on the table's device"));
  DeviceGuard g(dev);
  static_assert(sizeof(PolyakPair) == 24 && sizeof(PolyakChunk) == 8, "the table's layout");
  if (upload) {
    // the upload synchronises and copies from the host: both are errors while the stream records a graph
    if (step && stream_capturing(stream))
      return fail(USV_ERR_ARG, p + "the table upload is pending while the stream is capturing: call usv_polyak_prepare "
                                   "(DevicePolyak.prepare()) before the capture begins");
    std::vector<unsigned char> host(polyak_bytes(live, chunks));
    PolyakPair* const hp = reinterpret_cast<PolyakPair*>(host.data());
    PolyakChunk* const hc = reinterpret_cast<PolyakChunk*>(host.data() + (size_t)live * sizeof(PolyakPair));
    int64_t at = 0, c = 0;
    for (int32_t i = 0; i < n_pairs; ++i) {
      if (pairs[i].numel == 0) continue;
      hp[at] = PolyakPair{pairs[i].src, pairs[i].dst, (long long)pairs[i].numel};
      for (int64_t k = 0; k < polyak_chunks(pairs[i].numel); ++k) hc[c++] = PolyakChunk{(int)at, (int)k};
      ++at;
    }
    HIP_TRY(hipDeviceSynchronize());                 // launches in flight may read the old table
    HIP_TRY(hipMemcpy(table, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
  }
  if (!step) return USV_OK;
  float tau_f, om;
  polyak_coeffs(tau, tau_f, om);
  const PolyakPair* const dp = (const PolyakPair*)table;
  const PolyakChunk* const dc = (const PolyakChunk*)((const char*)table + (size_t)live * sizeof(PolyakPair));
  hipLaunchKernelGGL(polyak_kernel, dim3((unsigned)chunks), dim3(kBlock), 0, (hipStream_t)stream, dp, dc, tau_f, om);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_polyak_update(const usv_polyak_pair* pairs, int32_t n_pairs, void* table, size_t table_bytes, int32_t upload,
                      double tau, void* stream) {
  return polyak_call("usv_polyak_update", pairs, n_pairs, table, table_bytes, upload != 0, true, tau, stream);
}

int usv_polyak_prepare(const usv_polyak_pair* pairs, int32_t n_pairs, void* table, size_t table_bytes) {
  return polyak_call("usv_polyak_prepare", pairs, n_pairs, table, table_bytes, true, false, 0.0, nullptr);
}

size_t usv_adam_state_floats(const usv_adam_tensor* tensors, int32_t n) {
  int64_t live, chunks, state;
  return list_count(kAdamWords, tensors, n, false, live, chunks, state).empty() ? (size_t)state : 0;
}

size_t usv_adam_scratch_floats(const usv_adam_tensor* tensors, int32_t n) {
  int64_t live, chunks, state;
  return list_count(kAdamWords, tensors, n, false, live, chunks, state).empty() ? optim_scratch_floats(chunks) : 0;
}

size_t usv_adam_clock_bytes(void) { return sizeof(AdamClock); }

// usv_adam_step (clock null: `step` and `lr` are the caller's) and usv_adam_step_dev (they live in the clock block).
static int adam_step(const char* fn, const usv_adam_tensor* tensors, int32_t n, float* m, float* v, size_t state_floats,
                     int64_t step, double lr, void* clock, double beta1, double beta2, double eps,
                     double max_grad_norm, float* scratch, size_t scratch_floats, float* norm_out, void* stream) {
  int64_t live, chunks, state;
  int dev;
  const std::string p = std::string(fn) + ": ";
  const bool host_clock = clock == nullptr;
  ListWords words = kAdamWords;
  words.fn = fn;
  if (const std::string why = list_count(words, tensors, n, true, live, chunks, state); !why.empty())
    return fail(USV_ERR_ARG, why);
  if (host_clock && step < 1) return fail(USV_ERR_ARG, p + "step must be >= 1");
  if (host_clock && !adam_rate_ok(lr)) return fail(USV_ERR_ARG, p + "lr must be finite and >= 0");
  if (!adam_rate_ok(eps)) return fail(USV_ERR_ARG, p + "eps must be finite and >= 0");
  if (!adam_beta_ok(beta1) || !adam_beta_ok(beta2)) return fail(USV_ERR_ARG, p + "the betas must be in [0, 1)");
  if (max_grad_norm != max_grad_norm) return fail(USV_ERR_ARG, p + "max_grad_norm is NaN");
  const bool clip = max_grad_norm >= 0.0;
  if (clip && !norm_out) return fail(USV_ERR_ARG, p + "clipping needs norm_out");
  if (!m || !v) return fail(USV_ERR_ARG, p + "null state");
  if (clip && !scratch) return fail(USV_ERR_ARG, p + "clipping needs scratch");
  if (state_floats < (size_t)state) return fail(USV_ERR_ARG, p + "the state is too small");
  if (clip && scratch_floats < optim_scratch_floats(chunks)) return fail(USV_ERR_ARG, p + "the scratch is too small");
  std::vector<Buf> bufs = {{m, 16}, {v, 16}, {clip ? scratch : nullptr, 16, true}, {clip ? norm_out : nullptr, 4, true},
                           {clock, 16, true}};
  bufs.reserve(5 + 2 * (size_t)live);
  list_bufs(tensors, n, bufs);
  const std::string null = p + "null state",
                    align = p + "state, scratch or the clock block is not 16-B aligned or norm_out is not 4-B aligned",
                    first = p + "the state is not a device pointer",
                    other = p + "a buffer is not a device pointer on the state's device";
  const char* const msg[4] = {null.c_str(), align.c_str(), first.c_str(), other.c_str()};
  if (int rc = refuse_bufs(bufs.data(), bufs.size(), nullptr, msg)) return rc;
  if (live == 0) return USV_OK;
  if (int rc = refuse_bufs(bufs.data(), bufs.size(), &dev, msg)) return rc;
  DeviceGuard g(dev);
  // with a clock block: one launch ahead of the passes moves the step on and derives its scalars, once however many
  // launches the list takes; the scalars below that depend on the step are then not read
  const AdamScalars sc = adam_scalars(host_clock ? step : 1, host_clock ? lr : 0.0, beta1, beta2, eps);
  if (!host_clock) {
    hipLaunchKernelGGL(adam_clock_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (AdamClock*)clock, beta1, beta2);
    HIP_TRY(hipGetLastError());
  }
  if (clip) {
    list_pass(tensors, n, [&](const TensorTable& tab, dim3 grid) {
      const OptimSqsumArgs a{tab, (int)chunks, scratch, norm_out};
      hipLaunchKernelGGL(optim_sqsum_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
    });
    HIP_TRY(hipGetLastError());
  }
  list_pass(tensors, n, [&](const TensorTable& tab, dim3 grid) {
    if (host_clock) {
      const OptimAdamArgs a{tab, m, v, clip ? norm_out : nullptr, (float)max_grad_norm, sc};
      hipLaunchKernelGGL(optim_adam_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
    } else {
      const OptimAdamDevArgs a{tab, m, v, clip ? norm_out : nullptr, (float)max_grad_norm, sc, (const AdamClock*)clock};
      hipLaunchKernelGGL(optim_adam_dev_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
    }
  });
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_adam_step(const usv_adam_tensor* tensors, int32_t n, float* m, float* v, size_t state_floats, int64_t step,
                  double lr, double beta1, double beta2, double eps, double max_grad_norm, float* scratch,
                  size_t scratch_floats, float* norm_out, void* stream) {
  return adam_step("usv_adam_step", tensors, n, m, v, state_floats, step, lr, nullptr, beta1, beta2, eps,
                   max_grad_norm, scratch, scratch_floats, norm_out, stream);
}

int usv_adam_step_dev(const usv_adam_tensor* tensors, int32_t n, float* m, float* v, size_t state_floats,
                      void* clock_dev, size_t clock_bytes, double beta1, double beta2, double eps, double max_grad_norm,
                      float* scratch, size_t scratch_floats, float* norm_out, void* stream) {
  if (!clock_dev) return fail(USV_ERR_ARG, "usv_adam_step_dev: null clock block");
  if ((reinterpret_cast<uintptr_t>(clock_dev) & 15) != 0)
    return fail(USV_ERR_ARG, "usv_adam_step_dev: the clock block is not 16-B aligned");
  if (clock_bytes < sizeof(AdamClock)) return fail(USV_ERR_ARG, "usv_adam_step_dev: the clock block is too small");
  return adam_step("usv_adam_step_dev", tensors, n, m, v, state_floats, 0, 0.0, clock_dev, beta1, beta2,
                   eps, max_grad_norm, scratch, scratch_floats, norm_out, stream);
}

int usv_counter_add(uint32_t* word_dev, uint32_t inc, void* stream) {
  int dev;
  if (int rc = refuse_word("usv_counter_add", "word_dev", word_dev)) return rc;
  const Buf all[] = {{word_dev, 4}};
  if (check_bufs(all, 1, &dev) != kBufOk) return fail(USV_ERR_ARG, "usv_counter_add: word_dev is not a device pointer");
  DeviceGuard g(dev);
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, word_dev, inc);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

// ---- fused PPO loss (usv_ppo.hpp)
static int ppo_bufs(const Buf* b, size_t nb, int& dev) { return refuse_bufs(b, nb, dev, "usv_ppo", "scratch"); }

size_t usv_ppo_scratch_floats(int32_t rows) { return rows >= 1 ? ppo_scratch_floats(rows) : 0; }

int usv_ppo_loss(int32_t rows, const float* logp, const float* old_logp, const float* adv, const float* values,
                 const float* old_values, const float* returns, const float* entropy, int32_t normalize, float clip,
                 float clip_vf, float ent_coef, float vf_coef, float* moments, float* out, float* g_logp,
                 float* g_values, float* g_entropy, float* scratch, void* stream) {
  int dev;
  if (rows < 1) return fail(USV_ERR_ARG, "usv_ppo_loss: rows must be >= 1");
  if (!ppo_range_ok(clip)) return fail(USV_ERR_ARG, "usv_ppo_loss: clip must be finite and >= 0");
  if (old_values ? !ppo_range_ok(clip_vf) : clip_vf != 0.0f)
    return fail(USV_ERR_ARG, old_values ? "usv_ppo_loss: clip_vf must be finite and >= 0"
                                        : "usv_ppo_loss: old_values and clip_vf come together (clip_vf is 0 without old_values)");
  if (g_entropy && !entropy) return fail(USV_ERR_ARG, "usv_ppo_loss: g_entropy needs entropy");
  const Buf all[] = {{scratch, 16},  {logp, 4},          {old_logp, 4},      {adv, 4},          {values, 4},
                     {returns, 4},   {moments, 4},       {out, 4},           {old_values, 4, true}, {entropy, 4, true},
                     {g_logp, 4, true}, {g_values, 4, true}, {g_entropy, 4, true}};
  if (int rc = ppo_bufs(all, 13, dev)) return rc;
  DeviceGuard g(dev);
  const dim3 grid((unsigned)sac_partials(rows)), block(kBlock);
  const bool norm = normalize != 0 && rows > 1;
  if (norm) {
    const PpoMomentArgs m{rows, adv, nullptr, moments, nullptr, scratch};
    hipLaunchKernelGGL(ppo_sum_kernel, grid, block, 0, (hipStream_t)stream, m);
    hipLaunchKernelGGL(ppo_sqdev_kernel, grid, block, 0, (hipStream_t)stream, m);
  }
  const PpoLossArgs a{rows, PpoForm{norm, old_values != nullptr, entropy != nullptr, clip, clip_vf, ent_coef, vf_coef},
                      logp, old_logp, adv, values, old_values, returns, entropy, moments,
                      out, g_logp, g_values, g_entropy, scratch};
  hipLaunchKernelGGL(ppo_loss_kernel, grid, block, 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

int usv_ppo_explained_variance(int32_t rows, const float* values, const float* returns, float* out, float* scratch,
                               void* stream) {
  int dev;
  if (rows < 1) return fail(USV_ERR_ARG, "usv_ppo_explained_variance: rows must be >= 1");
  const Buf all[] = {{scratch, 16}, {values, 4}, {returns, 4}, {out, 4}};
  if (int rc = ppo_bufs(all, 4, dev)) return rc;
  DeviceGuard g(dev);
  const dim3 grid((unsigned)sac_partials(rows)), block(kBlock);
  const PpoMomentArgs m{rows, returns, values, scratch + kPpoScratchMeans, out, scratch};
  hipLaunchKernelGGL(ppo_sum_kernel, grid, block, 0, (hipStream_t)stream, m);
  hipLaunchKernelGGL(ppo_sqdev_kernel, grid, block, 0, (hipStream_t)stream, m);
  HIP_TRY(hipGetLastError());
  return USV_OK;
}

}  // extern "C"
