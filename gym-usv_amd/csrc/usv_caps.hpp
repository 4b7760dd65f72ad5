// usv_caps.hpp -- the CAPS smoothness regulariser as HIP kernels (include/usv_hip.h: usv_caps_perturb /
// usv_caps_loss): the perturbed observations of the spatial term and the two distance terms with their gradients at
// unit upstream.  The arithmetic and the summation order are usv_caps_math.hpp's; the backward is sac_scale_kernel.
//
//   caps_perturb_kernel
//       A thread per Philox block: four consecutive elements of one row, the last block of a row cut at W.  A thread
//       whose four elements are all there and 16-B aligned in both arrays moves them with one 16-B load and one 16-B
//       store; any other takes them one by one (rows of 715 floats: every fourth row is aligned).  Each thread reads
//       its elements before it writes them, so out may be obs.
//   caps_perturb_dev_kernel
//       The same text (usv_caps_noise.inc) with the epoch read from a word in device memory (usv_caps_perturb_dev).
//   caps_loss_kernel<A>
//       sac_policy_kernel's shape, from the same two forms (usv_sac.hpp): sac_for_rows with the row's 3 A means in
//       registers and the two distances as the strand's terms, then sac_finish and its thread's write.
#pragma once

#include "usv_caps_math.hpp"
#include "usv_sac.hpp"

namespace usv {

struct CapsPerturbArgs {
  long long blocks;                                  // rows * row_blocks: the threads that have work
  int W, row_blocks;
  const float* obs;
  float* out;
  float eps;
  uint64_t seed;
  uint32_t epoch;
};

#define USV_NOISE_KERNEL(name) name##_kernel
#define USV_NOISE_EPOCH_PARAM
#define USV_NOISE_PROLOGUE
#include "usv_caps_noise.inc"
#undef USV_NOISE_KERNEL
#undef USV_NOISE_EPOCH_PARAM
#undef USV_NOISE_PROLOGUE

// caps_perturb_dev_kernel (usv_caps_perturb_dev): the epoch is the word epoch_dev points to, read once by each wave.
#define USV_NOISE_KERNEL(name) name##_dev_kernel
#define USV_NOISE_EPOCH_PARAM , const uint32_t* __restrict__ epoch_dev
#define USV_NOISE_PROLOGUE a.epoch = sde_epoch_word(epoch_dev);
#include "usv_caps_noise.inc"
#undef USV_NOISE_KERNEL
#undef USV_NOISE_EPOCH_PARAM
#undef USV_NOISE_PROLOGUE

struct CapsLossArgs {
  int rows, squash;
  const float *mean, *mean_next, *mean_near;
  float lambda_t, lambda_s;
  float *out3, *g_mean, *g_next, *g_near, *scratch;
};

template <int A>
__global__ __launch_bounds__(kBlock) void caps_loss_kernel(CapsLossArgs a) {
  const bool squash = a.squash != 0, grads = a.g_mean || a.g_next || a.g_near;
  float s[2] = {0.0f, 0.0f};
  sac_for_rows(a.rows, [&](int64_t i) {
    float m[A], mn[A], mr[A], gm[A], gn[A], gr[A];
#pragma unroll
    for (int k = 0; k < A; ++k) {
      m[k] = a.mean[i * A + k];
      mn[k] = a.mean_next[i * A + k];
      mr[k] = a.mean_near[i * A + k];
    }
    float nT, nS;
    caps_row<A>(m, mn, mr, squash, a.lambda_t, a.lambda_s, a.rows, nT, nS, grads, gm, gn, gr);
#pragma unroll
    for (int k = 0; k < A; ++k) {
      if (a.g_mean) a.g_mean[i * A + k] = gm[k];
      if (a.g_next) a.g_next[i * A + k] = gn[k];
      if (a.g_near) a.g_near[i * A + k] = gr[k];
    }
    s[0] = s[0] + nT;
    s[1] = s[1] + nS;
  });
  if (sac_finish(s, blockIdx.x, (int)gridDim.x, kSacScratchSums, a.scratch)) {
    float out[3];
    caps_loss(s[0], s[1], a.lambda_t, a.lambda_s, a.rows, out);
    a.out3[0] = out[0];
    a.out3[1] = out[1];
    a.out3[2] = out[2];
  }
}

// caps_loss_kernel<A> for A = 1 .. kCapsMaxAct.
static void (*const kCapsLossKernels[kCapsMaxAct])(CapsLossArgs) = {
    caps_loss_kernel<1>, caps_loss_kernel<2>, caps_loss_kernel<3>, caps_loss_kernel<4>,
    caps_loss_kernel<5>, caps_loss_kernel<6>, caps_loss_kernel<7>, caps_loss_kernel<8>};

}  // namespace usv
