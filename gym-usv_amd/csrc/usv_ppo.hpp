// usv_ppo.hpp -- the fused PPO loss as HIP kernels (include/usv_hip.h: usv_ppo_loss / usv_ppo_explained_variance):
// the loss lines of SB3's PPO.train for one minibatch with their gradients at unit upstream, approx_kl,
// clip_fraction and explained_variance.  The arithmetic and the summation order are usv_ppo_math.hpp's; the row
// loop, the finish and the hand-off are usv_sac.hpp's two forms (sac_for_rows, sac_finish), with kPpoSums floats per
// partial as the stride; the backward is sac_scale_kernel.
//
//   ppo_sum_kernel     S of one or two row streams, x and (with sub) x - sub; sac_finish's thread writes the means
//                      to mom[0], mom[1].
//   ppo_sqdev_kernel   S((. - mean)^2) of the same streams, the means read from mom, which the launch before it
//                      wrote (stream order).  sac_finish's thread writes the unbiased std to mom[1] (one stream: the
//                      advantages) or 1 - v_r / v_y to ev[0] (two: the explained variance of x = returns, sub = values).
//   ppo_loss_kernel    one pass over the rows: the five sums through sac_finish<5>, the per-row unit gradients that
//                      are asked for; sac_finish's thread writes the loss and the five statistics.
#pragma once

#include "usv_ppo_math.hpp"
#include "usv_sac.hpp"

namespace usv {

struct PpoMomentArgs {
  int rows;
  const float *x, *sub;                              // sub: null for one stream
  float *mom, *ev, *scratch;                         // ev: ppo_sqdev_kernel's, with sub
};

__global__ __launch_bounds__(kBlock) void ppo_sum_kernel(PpoMomentArgs a) {
  float s[2] = {0.0f, 0.0f};
  sac_for_rows(a.rows, [&](int64_t i) {
    const float x = a.x[i];
    s[0] = s[0] + x;
    if (a.sub) s[1] = s[1] + (x - a.sub[i]);
  });
  if (sac_finish(s, blockIdx.x, (int)gridDim.x, kPpoSums, a.scratch)) {
    a.mom[0] = ppo_mean(s[0], a.rows);
    if (a.sub) a.mom[1] = ppo_mean(s[1], a.rows);
  }
}

__global__ __launch_bounds__(kBlock) void ppo_sqdev_kernel(PpoMomentArgs a) {
  const float m0 = a.mom[0], m1 = a.sub ? a.mom[1] : 0.0f;
  float s[2] = {0.0f, 0.0f};
  sac_for_rows(a.rows, [&](int64_t i) {
    const float x = a.x[i];
    s[0] = s[0] + ppo_sqdev(x, m0);
    if (a.sub) s[1] = s[1] + ppo_sqdev(x - a.sub[i], m1);
  });
  if (sac_finish(s, blockIdx.x, (int)gridDim.x, kPpoSums, a.scratch)) {
    if (a.sub) a.ev[0] = ppo_explained(s[0], s[1], a.rows);
    else a.mom[1] = ppo_std(s[0], a.rows);
  }
}

struct PpoLossArgs {
  int rows;
  PpoForm form;
  const float *logp, *old_logp, *adv, *values, *old_values, *returns, *entropy, *mom;
  float *out, *g_logp, *g_values, *g_entropy, *scratch;
};

__global__ __launch_bounds__(kBlock) void ppo_loss_kernel(PpoLossArgs a) {
  const PpoForm f = a.form;
  const float mean = f.normalize ? a.mom[0] : 0.0f, std = f.normalize ? a.mom[1] : 1.0f;
  const float g_ent = ppo_entropy_grad(f.ent_coef, a.rows);
  float s[kPpoSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  sac_for_rows(a.rows, [&](int64_t i) {
    float t[kPpoSums], gl, gv;
    ppo_row(f, a.logp[i], a.old_logp[i], ppo_advantage(a.adv[i], f.normalize, mean, std), a.values[i],
            f.vclip ? a.old_values[i] : 0.0f, a.returns[i], f.with_entropy ? a.entropy[i] : 0.0f, a.rows, t, gl, gv);
    if (a.g_logp) a.g_logp[i] = gl;
    if (a.g_values) a.g_values[i] = gv;
    if (a.g_entropy) a.g_entropy[i] = g_ent;
#pragma unroll
    for (int k = 0; k < kPpoSums; ++k) s[k] = s[k] + t[k];
  });
  if (sac_finish(s, blockIdx.x, (int)gridDim.x, kPpoSums, a.scratch)) {
    float out[kPpoOuts];
    ppo_finish(s, f.ent_coef, f.vf_coef, a.rows, out);
#pragma unroll
    for (int k = 0; k < kPpoOuts; ++k) a.out[k] = out[k];
  }
}

}  // namespace usv
