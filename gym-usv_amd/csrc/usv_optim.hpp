// usv_optim.hpp -- the kernels over a list of tensors (include/usv_hip.h: usv_adam_step, usv_polyak_update): torch's
// clip_grad_norm_ and Adam.step() over a whole parameter list, one launch without clipping and two with it, and SB3's
// polyak_update over a list of pairs, one launch.  The arithmetic and the summation order are usv_optim_math.hpp's;
// Polyak's arithmetic is usv_sac_math.hpp's.
//
// Adam's tensor table travels by value in the kernel arguments (TensorTable, at most kTableTensors tensors a launch;
// a longer list takes more launches per pass): a gradient made after zero_grad(set_to_none=True) has a new address on
// every backward, and a device table would have to be uploaded, with a synchronise, on every step.  A block owns one
// chunk of C = 4096 elements and finds its tensor by a binary search over the wave-uniform chunk starts (table_find).
// Polyak's pairs rarely move, and its kernel is short enough for the 3.5 KB of arguments to show (3.7 against 3.3 us
// queued): it keeps a device table, uploaded when an address has changed.
// chunk_elements is the element loop of optim_adam_kernel and polyak_kernel: 16-B accesses where the caller says the
// chunk's pointers are 16-B aligned, 4-B accesses for the tail of numel % 4 and for misaligned tensors.
//
//   optim_sqsum_kernel   the chunk's sum of squares: thread t is strand t, a 16-B load per group where the chunk's
//                        gradient pointer is 16-B aligned and four 4-B loads where it is not, the same groups either
//                        way.  sac_finish (usv_sac.hpp) with the chunk's sum at its global chunk number: the block
//                        that draws the last ticket of the whole list, over all launches of the pass, adds the chunk
//                        sums in ascending order, and its thread writes the norm.  No block waits for another.
//   optim_adam_kernel    coef from the norm (with clipping), then one read each of p, g, m, v and one write each of
//                        p, m, v per element, wide where p and g are both 16-B aligned.  The state segments are
//                        always 16-B aligned.
//   optim_adam_dev_kernel  the same pass (optim_adam_chunk) with step_size and bc2_sqrt read from the clock block in
//                        device memory, which adam_clock_tick_kernel (one thread, one launch per step) advanced and
//                        derived just before: a captured graph replays a step that counts.
//   counter_add_kernel   one thread adds to a uint32 in device memory: the noise epoch of a capturable head.
//   polyak_kernel        a block per chunk of one tensor pair, found through the device table of pairs and the table
//                        of (pair, chunk) per block: one read of src and dst and one write of dst per element, wide
//                        where both are 16-B aligned.
#pragma once

#include "usv_optim_math.hpp"

namespace usv {

static_assert(kOptimStrands == kBlock, "usv_optim_math.hpp's strands are this block's threads");

constexpr int kTableTensors = 96;                    // K

struct TensorTable {
  float* p[kTableTensors];                           // written: Adam's parameter, Polyak's dst
  const float* g[kTableTensors];                     // read: Adam's gradient, Polyak's src
  long long numel[kTableTensors];
  long long state[kTableTensors];                    // the segment's offset in m and v, floats (Adam alone)
  int first[kTableTensors + 1];                      // global number of the tensor's first chunk; [n]: the launch's end
  int n;
};

struct OptimSqsumArgs {
  TensorTable tab;
  int chunks;                                        // of the whole list: the ticket's target
  float *scratch, *norm_out;
};

struct OptimAdamArgs {
  TensorTable tab;
  float *m, *v;
  const float* total;                                // the norm, or null without clipping
  float max_norm;
  AdamScalars s;
};

struct OptimAdamDevArgs {                             // OptimAdamArgs with the clock block behind it
  TensorTable tab;
  float *m, *v;
  const float* total;
  float max_norm;
  AdamScalars s;                                     // step_size and bc2_sqrt are the clock's, not these
  const AdamClock* clock;
};

static_assert(sizeof(OptimSqsumArgs) <= 3584 && sizeof(OptimAdamArgs) <= 3584 && sizeof(OptimAdamDevArgs) <= 3584,
              "the arguments and the hidden ones stay under HIP's 4 KiB");

// Polyak's device table: the pairs that hold elements, then a (pair, chunk) per block.
struct PolyakPair {
  const float* src;
  float* dst;
  long long numel;
};
struct PolyakChunk {
  int pair, chunk;
};

// The block's chunk: its tensor's slot in the table, its offset in the tensor and its element count.
__device__ __forceinline__ int table_find(const TensorTable& tab, long long& off, int& count) {
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

template <int W>
struct alignas(4 * W) FloatPack {                    // what one access moves
  float v[W];
};

// The element loop of a chunk of `count` elements: f(x, y) for every element, x its values in the arrays rw (written
// back) and y those in ro.  wide: every pointer is 16-B aligned, and whole groups of four go by 16-B accesses.
template <int NW, int NR, class F>
__device__ __forceinline__ void chunk_elements(float* const (&rw)[NW], const float* const (&ro)[NR], int count, bool wide,
                                               F&& f) {
  auto at = [&](int i, auto pack) {
    using V = decltype(pack);
    constexpr int W = sizeof(V) / sizeof(float);
    V x[NW], y[NR];
#pragma unroll
    for (int n = 0; n < NW; ++n) x[n] = reinterpret_cast<const V*>(rw[n])[i];
#pragma unroll
    for (int n = 0; n < NR; ++n) y[n] = reinterpret_cast<const V*>(ro[n])[i];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      float xe[NW], ye[NR];
#pragma unroll
      for (int n = 0; n < NW; ++n) xe[n] = x[n].v[k];
#pragma unroll
      for (int n = 0; n < NR; ++n) ye[n] = y[n].v[k];
      f(xe, ye);
#pragma unroll
      for (int n = 0; n < NW; ++n) x[n].v[k] = xe[n];
    }
#pragma unroll
    for (int n = 0; n < NW; ++n) reinterpret_cast<V*>(rw[n])[i] = x[n];
  };
  int done = 0;
  if (wide) {
    const int n4 = count / 4;
    for (int i = threadIdx.x; i < n4; i += kBlock) at(i, FloatPack<4>{});
    done = 4 * n4;
  }
  for (int i = done + threadIdx.x; i < count; i += kBlock) at(i, FloatPack<1>{});
}

__device__ __forceinline__ bool both_wide(const void* a, const void* b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

__global__ __launch_bounds__(kBlock) void optim_sqsum_kernel(OptimSqsumArgs a) {
  long long off;
  int count;
  const int t = table_find(a.tab, off, count);
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
  if (sac_finish(s, (size_t)(a.tab.first[0] + (int)blockIdx.x), a.chunks, 1, a.scratch)) a.norm_out[0] = optim_norm(s[0]);
}

// The Adam pass of a block's chunk under both kernels: `scalars(a)` is the step's AdamScalars.
template <class Args, class Scalars>
__device__ __forceinline__ void optim_adam_chunk(const Args& a, Scalars&& scalars) {
  long long off;
  int count;
  const int t = table_find(a.tab, off, count);
  const bool clip = a.total != nullptr;
  const float coef = clip ? adam_clip_coef(a.total[0], a.max_norm) : 1.0f;
  float* const p = a.tab.p[t] + off;
  const float* const g = a.tab.g[t] + off;
  const AdamScalars s = scalars(a);
  chunk_elements({p, a.m + a.tab.state[t] + off, a.v + a.tab.state[t] + off}, {g}, count, both_wide(p, g),
                 [&](float (&x)[3], const float (&y)[1]) {
                   adam_value(x[0], x[1], x[2], clip ? adam_clipped(y[0], coef) : y[0], s);
                 });
}

__global__ __launch_bounds__(kBlock) void optim_adam_kernel(OptimAdamArgs a) {
  optim_adam_chunk(a, [](const OptimAdamArgs& x) { return x.s; });
}

// usv_adam_step_dev's: step_size and bc2_sqrt come from the clock block, which adam_clock_tick_kernel wrote in the
// launch before this pass (stream order); a block reads the two words once, wave-uniform.
__global__ __launch_bounds__(kBlock) void optim_adam_dev_kernel(OptimAdamDevArgs a) {
  optim_adam_chunk(a, [](const OptimAdamDevArgs& x) {
    AdamScalars s = x.s;
    s.step_size = x.clock->step_size;
    s.bc2_sqrt = x.clock->bc2_sqrt;
    return s;
  });
}

// One thread: the step moves on by one and its two scalars are derived from it and lr, in double, each cast once.
// Once per usv_adam_step_dev, ahead of its other launches, however many launches the list takes.
__global__ void adam_clock_tick_kernel(AdamClock* __restrict__ clock, double beta1, double beta2) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t t = clock->step + 1;
  float step_size, bc2_sqrt;
  adam_clock_scalars(t, clock->lr, beta1, beta2, step_size, bc2_sqrt);
  clock->step = t;
  clock->step_size = step_size;
  clock->bc2_sqrt = bc2_sqrt;
}

// One thread: *word += inc, wrapping (usv_counter_add: a noise epoch that lives in device memory).
__global__ void counter_add_kernel(uint32_t* __restrict__ word, uint32_t inc) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  word[0] = counter_added(word[0], inc);
}

__global__ __launch_bounds__(kBlock) void polyak_kernel(const PolyakPair* __restrict__ pairs,
                                                        const PolyakChunk* __restrict__ chunks, float tau_f, float om) {
  const PolyakChunk c = chunks[blockIdx.x];
  const PolyakPair pr = pairs[c.pair];
  const long long off = (long long)c.chunk * kPolyakChunk;
  const long long left = pr.numel - off;
  const int count = left < kPolyakChunk ? (int)left : kPolyakChunk;
  float* const dst = pr.dst + off;
  const float* const src = pr.src + off;
  chunk_elements({dst}, {src}, count, both_wide(dst, src),
                 [&](float (&x)[1], const float (&y)[1]) { x[0] = polyak_value(x[0], y[0], tau_f, om); });
}

}  // namespace usv
