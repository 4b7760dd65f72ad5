// usv_optim.hpp -- the fused optimizer step as HIP kernels (include/usv_hip.h: usv_adam_step): torch's
// clip_grad_norm_ and Adam.step() over a whole parameter list, one launch without clipping and two with it.  The
// arithmetic and the summation order are usv_optim_math.hpp's.
//
// The tensor table travels by value in the kernel arguments (OptimTable, at most kOptimTensors tensors a launch; a
// longer list takes more launches per pass): a gradient made after zero_grad(set_to_none=True) has a new address on
// every backward, and a device table would have to be uploaded, with a synchronise, on every step.  A block owns one
// chunk of C = 4096 elements and finds its tensor by a binary search over the wave-uniform chunk starts.
//
//   optim_sqsum_kernel   the chunk's sum of squares: thread t is strand t, a 16-B load per group where the chunk's
//                        gradient pointer is 16-B aligned and four 4-B loads where it is not, the same groups either
//                        way.  Block sums by sac_block_sums; the chunk's sum goes to the scratch at its global chunk
//                        number and the block that draws the last ticket of the whole list, over all launches of the
//                        pass, adds the chunk sums in ascending order and writes the norm (sac_combine_at).  No block
//                        waits for another.
//   optim_adam_kernel    coef from the norm (with clipping), then one read each of p, g, m, v and one write each of
//                        p, m, v per element: 16-B accesses where p and g are both 16-B aligned, 4-B accesses for the
//                        tail of numel % 4 and for misaligned tensors.  The state segments are always 16-B aligned.
#pragma once

#include "usv_optim_math.hpp"

namespace usv {

static_assert(kOptimStrands == kBlock, "usv_optim_math.hpp's strands are this block's threads");

constexpr int kOptimTensors = 96;                    // K

struct OptimTable {
  float* p[kOptimTensors];
  const float* g[kOptimTensors];
  long long numel[kOptimTensors];
  long long state[kOptimTensors];                    // the segment's offset in m and v, floats
  int first[kOptimTensors + 1];                      // global number of the tensor's first chunk; [n]: the launch's end
  int n;
};

struct OptimSqsumArgs {
  OptimTable tab;
  int chunks;                                        // of the whole list: the ticket's target
  float *scratch, *norm_out;
};

struct OptimAdamArgs {
  OptimTable tab;
  float *m, *v;
  const float* total;                                // the norm, or null without clipping
  float max_norm;
  AdamScalars s;
};
static_assert(sizeof(OptimSqsumArgs) <= 3584 && sizeof(OptimAdamArgs) <= 3584,
              "the arguments and the hidden ones stay under HIP's 4 KiB");

// The block's chunk: its tensor's slot in the table, its offset in the tensor and its element count.
__device__ __forceinline__ int optim_find(const OptimTable& tab, long long& off, int& count) {
  const int chunk = tab.first[0] + (int)blockIdx.x;
  int lo = 0, hi = tab.n;                            // first[lo] <= chunk < first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (tab.first[mid] <= chunk) lo = mid; else hi = mid;
  }
  off = (long long)(chunk - tab.first[lo]) * kOptimChunk;
  const long long left = tab.numel[lo] - off;
  count = left < kOptimChunk ? (int)left : kOptimChunk;
  return lo;
}

__global__ __launch_bounds__(kBlock) void optim_sqsum_kernel(OptimSqsumArgs a) {
  __shared__ float red[1][kSacWaves];
  long long off;
  int count;
  const int t = optim_find(a.tab, off, count);
  const float* const g = a.tab.g[t] + off;
  float s[1] = {0.0f};
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
#pragma unroll
    for (int j = 0; j < kOptimStrandGroups; ++j) {
      const int q = (int)threadIdx.x + j * kOptimStrands, at = kOptimGroup * q;
      if (at + kOptimGroup <= count) {
        const float4 x = reinterpret_cast<const float4*>(g)[q];
        s[0] = optim_sq_add(optim_sq_add(optim_sq_add(optim_sq_add(s[0], x.x), x.y), x.z), x.w);
      } else {
        for (int k = 0; k < kOptimGroup; ++k)
          if (at + k < count) s[0] = optim_sq_add(s[0], g[at + k]);
      }
    }
  } else {
    s[0] = optim_strand_sqsum(g, count, (int)threadIdx.x);
  }
  sac_block_sums(s, red);
  if (a.chunks > 1) {
    float total[1];
    if (!sac_combine_at(s, (size_t)(a.tab.first[0] + (int)blockIdx.x), a.chunks, 1, a.scratch, total)) return;
    s[0] = total[0];
  }
  if (threadIdx.x == 0) a.norm_out[0] = optim_norm(s[0]);
}

__global__ __launch_bounds__(kBlock) void optim_adam_kernel(OptimAdamArgs a) {
  long long off;
  int count;
  const int t = optim_find(a.tab, off, count);
  const bool clip = a.total != nullptr;
  const float coef = clip ? adam_clip_coef(a.total[0], a.max_norm) : 1.0f;
  float* const p = a.tab.p[t] + off;
  const float* const g = a.tab.g[t] + off;
  float* const m = a.m + a.tab.state[t] + off;
  float* const v = a.v + a.tab.state[t] + off;
  const AdamScalars s = a.s;
  int done = 0;
  if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g)) & 15) == 0) {
    const int n4 = count / 4;
    for (int i = threadIdx.x; i < n4; i += kBlock) {
      float4 pp = reinterpret_cast<float4*>(p)[i];
      float4 gg = reinterpret_cast<const float4*>(g)[i];
      float4 mm = reinterpret_cast<float4*>(m)[i];
      float4 vv = reinterpret_cast<float4*>(v)[i];
      if (clip) {
        gg.x = adam_clipped(gg.x, coef);
        gg.y = adam_clipped(gg.y, coef);
        gg.z = adam_clipped(gg.z, coef);
        gg.w = adam_clipped(gg.w, coef);
      }
      adam_value(pp.x, mm.x, vv.x, gg.x, s);
      adam_value(pp.y, mm.y, vv.y, gg.y, s);
      adam_value(pp.z, mm.z, vv.z, gg.z, s);
      adam_value(pp.w, mm.w, vv.w, gg.w, s);
      reinterpret_cast<float4*>(p)[i] = pp;
      reinterpret_cast<float4*>(m)[i] = mm;
      reinterpret_cast<float4*>(v)[i] = vv;
    }
    done = 4 * n4;
  }
  for (int i = done + threadIdx.x; i < count; i += kBlock) {
    float pp = p[i], mm = m[i], vv = v[i];
    const float gg = clip ? adam_clipped(g[i], coef) : g[i];
    adam_value(pp, mm, vv, gg, s);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
  }
}

}  // namespace usv
