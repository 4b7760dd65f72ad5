// usv_norm_math.hpp -- the arithmetic and the work split of the fused VecNormalize (usv_norm.hpp):
// how a column's (count, mean, M2) is accumulated, in which order partial moments combine, how a batch
// merges into the running statistics (SB3 RunningMeanStd.update_from_moments), and the transform of a
// value.  Plain C++ marked __host__ __device__, no HIP types: the kernels and a stand-alone host program
// (tests/test_norm_math.py) run the same functions in the same order.
//
// Moments are (n, mean, M2 = sum (x - mean)^2), never (sum x, sum x^2): every term added to M2 is a
// square times a non-negative factor, so M2 >= 0 always, and a constant column has every delta == 0
// exactly, hence M2 == 0 exactly.
//
// Work split of one [N][D] batch (norm_* functions below are the single source of it):
//   chunk   block b owns the rows [b R, min(N, (b + 1) R)), R = norm_chunk_rows(N): kNormBlockRows = 64
//           up to 65 536 envs, then growing in steps of 64 so that there are never more than
//           kNormMaxPartials = 1024 chunks (2^23 envs: R = 8192).  One partial per chunk and column.
//   group   a chunk is cut into groups of kNormGroupRows = 16 consecutive rows (the last one of the
//           batch may be short).  Group gi of a chunk belongs to wave gi mod kNormWaves; a wave takes
//           its groups in increasing order.
//   lane    within a 64-column tile, lane l is column 64 tile + l: it reads its column of the group's
//           rows (one row = one contiguous 256-B wave load), accumulates them in row order with
//           norm_group_add (Welford; the reciprocals 1/2 .. 1/16 are literals once unrolled, so the hot
//           loop has no division), and folds the group into its running partial with norm_combine.
//   block   the kNormWaves wave partials of a column combine in wave order 0, 1, 2, 3.
//   batch   the P partials of a column combine in block-index order as a fixed tree: lane l of the
//           finalising wave folds the partials [l per, (l + 1) per), per = ceil(P / 64), in increasing
//           order; then the 64 lane results fold pairwise, (l, l + s) for s = 1, 2, 4 .. 32, the lower
//           index always the left operand.  At most 16 + 6 dependent combines, whatever N.
// Nothing here depends on which block or wave runs first.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__CUDACC__)
#define USV_NORM_HD __host__ __device__ inline
#else
#define USV_NORM_HD inline
#endif

namespace usv {

constexpr int kNormGroupRows = 16;     // rows a wave accumulates before it combines
constexpr int kNormWaves = 4;          // waves of a block
constexpr int kNormBlockRows = kNormGroupRows * kNormWaves;   // smallest chunk: 64 rows
constexpr int kNormMaxPartials = 1024;
constexpr int kNormLanes = 64;         // lanes of the finalising wave = columns of a tile

struct NormMoments { double n, mean, m2; };

// Rows per chunk and number of chunks (= partials per column) of a batch of N rows.
USV_NORM_HD int norm_chunk_rows(int64_t N) {
  const int64_t per = (int64_t)kNormBlockRows * kNormMaxPartials;
  const int64_t m = (N + per - 1) / per;
  return (int)(kNormBlockRows * (m > 0 ? m : 1));
}
USV_NORM_HD int norm_num_partials(int64_t N) {
  const int64_t R = norm_chunk_rows(N);
  return (int)((N + R - 1) / R);
}
USV_NORM_HD int64_t norm_chunk_begin(int64_t N, int b) { return (int64_t)b * norm_chunk_rows(N); }
USV_NORM_HD int64_t norm_chunk_end(int64_t N, int b) {
  const int64_t e = norm_chunk_begin(N, b) + norm_chunk_rows(N);
  return e < N ? e : N;
}
USV_NORM_HD int norm_chunk_groups(int64_t N) { return norm_chunk_rows(N) / kNormGroupRows; }
USV_NORM_HD int norm_group_wave(int gi) { return gi % kNormWaves; }
// First row of group gi of chunk b and its row count (<= 0: past the end of the batch).
USV_NORM_HD int64_t norm_group_begin(int64_t N, int b, int gi) {
  return norm_chunk_begin(N, b) + (int64_t)gi * kNormGroupRows;
}
USV_NORM_HD int norm_group_rows(int64_t N, int b, int gi) {
  const int64_t left = norm_chunk_end(N, b) - norm_group_begin(N, b, gi);
  return left < kNormGroupRows ? (int)left : kNormGroupRows;
}

// The partials lane l of the finalising wave folds: [begin, end) of P.
USV_NORM_HD void norm_final_run(int P, int l, int* begin, int* end) {
  const int per = (P + kNormLanes - 1) / kNormLanes;
  const int b = l * per, e = b + per;
  *begin = b < P ? b : P;
  *end = e < P ? e : P;
}

// Welford: x is element i (0-based) of a group that started from {0, 0, 0}.
USV_NORM_HD void norm_group_add(NormMoments& g, double x, int i) {
  const double inv = 1.0 / (double)(i + 1);
  const double d = x - g.mean;
  g.n = (double)(i + 1);
  g.mean += d * inv;
  g.m2 += (d * d) * ((double)i * inv);
}

// Chan: a (the earlier rows) and b as one set.  An empty side leaves the other unchanged.
USV_NORM_HD NormMoments norm_combine(const NormMoments& a, const NormMoments& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double n = a.n + b.n, inv = 1.0 / n, d = b.mean - a.mean;
  NormMoments r;
  r.n = n;
  r.mean = a.mean + d * (b.n * inv);
  r.m2 = (a.m2 + b.m2) + (d * d) * (a.n * b.n * inv);
  return r;
}

// RunningMeanStd.update_from_moments (SB3 common/running_mean_std.py) with the batch given as moments:
// batch_var * batch_count there is b.m2 here.  `count` is read, not written (every column of a batch
// merges against the same old count; norm_count_after gives the new one).
USV_NORM_HD void norm_merge(double& mean, double& var, double count, const NormMoments& b) {
  if (b.n == 0.0) return;
  const double delta = b.mean - mean, tot = count + b.n;
  mean = mean + delta * b.n / tot;
  const double m2 = var * count + b.m2 + delta * delta * count * b.n / tot;
  var = m2 / tot;
}
USV_NORM_HD double norm_count_after(double count, double n) { return count + n; }

// The published reciprocal: 1 / sqrt(var + epsilon).  SB3 divides by sqrt(var + epsilon) where
// norm_apply multiplies by this; see norm_apply.
USV_NORM_HD double norm_inv_std(double var, double epsilon) { return 1.0 / sqrt(var + epsilon); }

// VecNormalize.normalize_obs / normalize_reward (mean = 0 for the reward):
// float(clip((x - mean) * inv_std, -clip, clip)).  A subtraction followed by a multiplication: there is
// no a * b + c in it, so no FMA can form, and NumPy's ((x - mean) * inv).clip(-c, c).astype(f32) gives
// the same bits from the same mean and inv_std.  Against SB3's division by the square root the value
// before the rounding to f32 differs by at most one f64 ulp.
USV_NORM_HD float norm_apply(double x, double mean, double inv_std, double clip) {
  double y = (x - mean) * inv_std;
  y = y < -clip ? -clip : y;
  y = y > clip ? clip : y;
  return (float)y;
}

// returns = returns * gamma + reward (VecNormalize.step_wait), product and sum rounded separately.
USV_NORM_HD double norm_discount(double returns, double gamma, double reward) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double p = returns * gamma;
  return p + reward;
}

}  // namespace usv
