// usv_layout.hpp -- where the state lives: the constants the layout depends on, the regions of a
// handle's device slab (slab_layout) and, one row per USV_FIELD_*, where each public field sits in it
// (field_table).  Plain host C++17 (no HIP), so the layout is tested on its own
// (tests/test_state_layout.py); the device headers take the constants from here.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "usv_hip.h"
#include "usv_variant.hpp"

namespace usv {

constexpr int kSensors = 128;                      // simple_env.py:11
constexpr int kAsmcN = 16;                         // unique UsvAsmc state values

// rows of State::freal
enum RealField {
  F_X, F_Y, F_PSI, F_U, F_V, F_R, F_LAST_U, F_LAST_R, F_PROGRESS,
  F_PX0, F_PY0, F_PX1, F_PY1, F_MAX_U, F_MAX_R, F_REF_V, F_NREAL
};
// rows of State::fint.  I_TURNS (f32 usv-simple / usv-asmc-simple): whole turns of the heading, see store_heading
enum IntField { I_NOBS, I_ELAPSED, I_EPISODE, I_SCAN, I_TURNS, I_NINT };
// rows of State::v0 (legacy envs): last[9], aux[3], target[6], action_last, ye_int, ye_last
constexpr int kV0Last = 0, kV0Aux = 9, kV0Target = 12, kV0ALast = 18, kV0Ye = 19, kV0N = 21;
// custom experiment record (usv_experiment, simple_env.py:292-300), in R: n, path start (2),
// path angle, pose (3), pad, then x[cap], y[cap], r[cap]
constexpr int kExpN = 0, kExpPS = 1, kExpAngle = 3, kExpPose = 4, kExpObs = 8;
constexpr int kQRec = 16;      // f32 values of an env record of the block-queue step (usv_queue_step.hpp)
constexpr int kNpRngN = 10;    // uint32 rows of State::nprng (USV_FIELD_NP_RNG)
constexpr int kNpMtN = 625;    // uint32 rows of State::npmt (USV_FIELD_NP_MT): MT19937 key[624], pos
// obstacle plane stride: cap rounded up to a multiple of 4
constexpr int obst_stride(int cap) { return (cap + 3) & ~3; }

// The slab's regions in slab order; one State pointer (or Handle::exp_buf) each.
enum Region {
  R_FREAL, R_FINT, R_OBST, R_SENSOR_LAST, R_ASMC, R_V0, R_RAY_TAB, R_POSE, R_QREC, R_NPRNG, R_EXP, R_NPMT, R_COUNT
};
struct SlabLayout {
  size_t off[R_COUNT], size[R_COUNT];   // bytes; size rounded up to 256 (0: the region is absent)
  size_t fstride;                       // elements between SoA rows: >= N, a row of R is 256-B aligned
  size_t ostride;                       // obst_stride(cap)
  size_t total;
};
// real_bytes: sizeof(R) of the handle's precision.  Each region starts where the one before it ends.
inline SlabLayout slab_layout(const usv_config& c, size_t real_bytes) {
  const size_t N = (size_t)c.num_envs, cap = (size_t)c.obstacle_cap, sR = real_bytes;
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  SlabLayout L{};
  L.fstride = al(N * sR) / sR;          // also >= N int32 (sR >= 4)
  L.ostride = (size_t)obst_stride((int)cap);
  auto add = [&](Region r, size_t bytes) { L.off[r] = L.total; L.size[r] = al(bytes); L.total += L.size[r]; };
  add(R_FREAL, F_NREAL * L.fstride * sR);
  add(R_FINT, I_NINT * L.fstride * 4);
  add(R_OBST, N * 3 * L.ostride * sR);
  add(R_SENSOR_LAST, N * kSensors * sR);
  add(R_ASMC, kAsmcN * N * sR);
  add(R_V0, kV0N * L.fstride * sR);
  add(R_RAY_TAB, 2 * kSensors * sR);
  add(R_POSE, 2 * N * 4 * sR);          // two 4-vectors of R per env
  add(R_QREC, N * kQRec * 4);
  add(R_NPRNG, kNpRngN * L.fstride * 4);
  add(R_EXP, (kExpObs + 3 * cap) * sR);
  add(R_NPMT, is_legacy(c.mode) ? kNpMtN * L.fstride * 4 : 0);   // legacy ids only
  return L;
}

// A public field: component c of env e is element first + e * env_stride + c * comp_stride of its
// region, counted in R (real fields) or int32 (int fields).  On the host it is [N][per] row-major.
struct Field {
  const char* name;
  int is_int;
  int per;                              // values per env
  Region region;
  size_t first, env_stride, comp_stride;
};
struct FieldTable { Field row[USV_FIELD_COUNT]; };
// One row per USV_FIELD_*, in enum order.  A new field is one row here (and its enum entry).
inline FieldTable field_table(const usv_config& c, const SlabLayout& L) {
  const size_t N = (size_t)c.num_envs, fs = L.fstride, os = L.ostride;
  const int cap = c.obstacle_cap;
  auto real = [&](const char* name, int f) { return Field{name, 0, 1, R_FREAL, f * fs, 1, 0}; };
  auto integer = [&](const char* name, int i) { return Field{name, 1, 1, R_FINT, i * fs, 1, 0}; };
  auto plane = [&](const char* name, int p) { return Field{name, 0, cap, R_OBST, p * os, 3 * os, 1}; };
  auto v0 = [&](const char* name, int per, int r) { return Field{name, 0, per, R_V0, r * fs, 1, fs}; };
  const Field rows[] = {
      real("x", F_X), real("y", F_Y), real("psi", F_PSI), real("u", F_U), real("v", F_V), real("r", F_R),
      real("last_u", F_LAST_U), real("last_r", F_LAST_R), real("progress", F_PROGRESS),
      real("path_x0", F_PX0), real("path_y0", F_PY0), real("path_x1", F_PX1), real("path_y1", F_PY1),
      real("max_u", F_MAX_U), real("max_r", F_MAX_R), real("ref_v", F_REF_V),
      integer("n_obs", I_NOBS), integer("elapsed", I_ELAPSED), integer("episode", I_EPISODE),
      integer("scan_valid", I_SCAN),
      plane("obs_x", 0), plane("obs_y", 1), plane("obs_r", 2),
      {"sensor_last", 0, kSensors, R_SENSOR_LAST, 0, (size_t)kSensors, 1},     // [N][128]
      {"asmc", 0, kAsmcN, R_ASMC, 0, 1, N},                                    // [16][N]
      v0("v0_last", 9, kV0Last), v0("v0_aux", 3, kV0Aux), v0("v0_target", 6, kV0Target),
      v0("v0_action_last", 1, kV0ALast), v0("v0_ye", 2, kV0Ye),
      {"np_rng", 1, kNpRngN, R_NPRNG, 0, 1, fs},
      {"np_mt", 1, is_legacy(c.mode) ? kNpMtN : 0, R_NPMT, 0, 1, fs},          // legacy ids only
  };
  static_assert(sizeof(rows) / sizeof(rows[0]) == USV_FIELD_COUNT, "one row per USV_FIELD_*");
  FieldTable t{};
  for (int f = 0; f < USV_FIELD_COUNT; ++f) t.row[f] = rows[f];
  return t;
}
// bytes of a field on the host: float64 or int32 per value
inline size_t field_bytes(const usv_config& c, const Field& fd) {
  return (size_t)c.num_envs * fd.per * (fd.is_int ? 4 : 8);
}

}  // namespace usv
