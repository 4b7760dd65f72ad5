// usv_row_copy.hpp -- the row copy of the trainer kernels: a wave moves W floats of each of its `ne`
// (<= kWrapEnvs) consecutive rows from a strided source to a strided destination.  The frame push of the
// fused wrappers (usv_wrap.hpp, with the normalising transform: usv_norm.hpp) and the obs stores of the
// rollout buffer (usv_rollout.hpp, usv_rollout_frames.hpp) are this one routine.
//
// Pieces.  Each row is cut into pieces of four floats, P = ceil(W / 4) per row, the last one moved back
// to end with the row (it re-copies up to three floats of its neighbour: the same values from the same
// wave).  Lane l takes pieces l, l + 64, ... of the wave's ne P: one 16-B load and one or two 16-B stores
// each, 1 KiB of contiguous source per wave instruction when the source rows are contiguous; W = 143:
// 9 pieces per lane.  Three pieces are taken per pass: their addresses are worked out first and their
// loads issued back to back, so three are in flight per lane before the first store.
// Alignment.  Rows are 4-B aligned in general (143 floats = 572 B), and the accesses are declared so
// (WrapQuad): a 16-B global access needs dword alignment only, and is full rate when the address happens
// to be 16-B aligned.  The stores are plain ("Store policy: plain").
// W < 4 takes one float per piece.
#pragma once

#include "usv_state.hpp"

namespace usv {

constexpr int kWrapEnvs = 16;   // envs per wave: 4 096 waves at 65 536 envs, each moving ~27 KB

// four floats at dword alignment: one global_load / global_store_dwordx4
typedef float WrapQuad4 __attribute__((ext_vector_type(4)));
typedef WrapQuad4 WrapQuad __attribute__((aligned(4)));

// The transform of a copy: what is stored for the four floats from column c on, or for the one of
// column c.  This one stores what it loaded.
struct RowCopyPlain {
  __device__ __forceinline__ WrapQuad4 quad(WrapQuad4 v, int) const { return v; }
  __device__ __forceinline__ float one(float v, int) const { return v; }
};

// span / dst: the wave's first row; mirror: every store is repeated `mir` floats further on.
// SS / DS: the types the row strides are multiplied in (int keeps a row index in 32 bits).
template <typename SS, typename DS, typename XF>
__device__ __forceinline__ void copy_rows(const float* span, SS sstride, float* dst, DS dstride, bool mirror,
                                          ptrdiff_t mir, int W, int ne, int l, const XF& xf) {
  if (W >= 4) {
    const int P = (W + 3) / 4, np = ne * P;             // pieces per row, of the wave
    const int dk = kWave / P, dr = kWave % P;
    int k = l / P, r = l - k * P;                       // piece l + 64 i: row k, piece r of it
    for (int q = l; q < np; q += 3 * kWave) {
      const float* sp[3];
      float* dp[3];
      int cc[3];
      WrapQuad4 v[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int c = min(4 * r, W - 4);
        cc[i] = c;
        sp[i] = span + (SS)k * sstride + c;
        dp[i] = dst + (DS)k * dstride + c;
        k += dk;
        r += dr;
        if (r >= P) { r -= P; ++k; }
      }
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (q + i * kWave < np) v[i] = *reinterpret_cast<const WrapQuad*>(sp[i]);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (q + i * kWave < np) {
          const WrapQuad4 o = xf.quad(v[i], cc[i]);
          *reinterpret_cast<WrapQuad*>(dp[i]) = o;
          if (mirror) *reinterpret_cast<WrapQuad*>(dp[i] + mir) = o;
        }
    }
  } else {
    for (int q = l; q < ne * W; q += kWave) {
      const int k = q / W, c = q - k * W;
      const float v = xf.one(span[(SS)k * sstride + c], c);
      float* const d = dst + (DS)k * dstride + c;
      d[0] = v;
      if (mirror) d[mir] = v;
    }
  }
}

}  // namespace usv
