// usv_sde_noise.inc -- the four gSDE kernels that draw noise, stated once and included twice by usv_sde.hpp:
//   USV_NOISE_KERNEL(name)   name_kernel, then name_dev_kernel
//   USV_NOISE_EPOCH_PARAM    nothing, then `const uint32_t* __restrict__ epoch_dev,`
//   USV_NOISE_PROLOGUE       nothing, then `a.epoch = sde_epoch_word(epoch_dev);`: each wave reads the word once
// The first inclusion is token for token the kernels with the epoch in their arguments, so their code is what it
// was before the _dev kernels existed (an inlined shared body was not: tools/asm_same.py, DESIGN.md).
template <int A>
__global__ __launch_bounds__(kBlock) void USV_NOISE_KERNEL(sde_sample)(
    SdeArgs a, USV_NOISE_EPOCH_PARAM const float* __restrict__ mean, const float* __restrict__ lat, size_t stride,
    const float* __restrict__ std, float* __restrict__ act, float* __restrict__ act_env, float* __restrict__ logp) {
  USV_NOISE_PROLOGUE
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int64_t e = (int64_t)blockIdx.x * kWaves + wave;
  if (e >= a.n) return;                                 // wave-uniform
  float noise[A], var[A];
  sde_row_sums<A, true>(a.L, l, lat + (size_t)e * stride, std, a.seed, a.gid0 + (uint64_t)e, a.epoch, noise, var);
  if (l != 0) return;
  float lp = 0.0f;
#pragma unroll
  for (int k = 0; k < A; ++k) {
    const float m = mean[(size_t)e * A + k];
    const float ak = sde_action(m, noise[k]);
    act[(size_t)e * A + k] = ak;
    act_env[(size_t)e * A + k] = sde_clip(ak, a.low[k], a.high[k]);
    lp = lp + sde_logp_term(ak, m, var[k]);
  }
  logp[e] = lp;
}

// The squashed head's forward: the tanh tail.  gauss and var (the backward's saved u and var_k) are NULL together
// on a call that will not be differentiated.
template <int A>
__global__ __launch_bounds__(kBlock) void USV_NOISE_KERNEL(sde_squash_forward)(
    SdeArgs a, USV_NOISE_EPOCH_PARAM const float* __restrict__ mean, const float* __restrict__ lat, size_t stride,
    const float* __restrict__ std, float* __restrict__ act, float* __restrict__ act_env, float* __restrict__ logp,
    float* __restrict__ gauss, float* __restrict__ var_out) {
  USV_NOISE_PROLOGUE
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int64_t e = (int64_t)blockIdx.x * kWaves + wave;
  if (e >= a.n) return;                                 // wave-uniform
  float noise[A], var[A];
  sde_row_sums<A, true>(a.L, l, lat + (size_t)e * stride, std, a.seed, a.gid0 + (uint64_t)e, a.epoch, noise, var);
  if (l != 0) return;
  float lp = 0.0f;
#pragma unroll
  for (int k = 0; k < A; ++k) {
    const float m = mean[(size_t)e * A + k];
    const float u = sde_action(m, noise[k]);
    float t, om;
    sde_squash(u, t, om);
    act[(size_t)e * A + k] = t;
    act_env[(size_t)e * A + k] = sde_unscale(t, a.low[k], a.high[k]);
    if (gauss) {
      gauss[(size_t)e * A + k] = u;
      var_out[(size_t)e * A + k] = var[k];
    }
    lp = lp + sde_squash_logp_term(u, m, var[k], om);
  }
  logp[e] = lp;
}

// The squashed head's backward.  A wave owns partial p of g_std: rows [p R, min(n, (p + 1) R)), R =
// sde_rows_per_partial(n).  Pass-outer, row-inner: within a pass of 256 latents a lane keeps the 4 A std values
// and 4 A g_std accumulators of its elements in registers at any L, walks the partial's rows in ascending order,
// rebuilds each row's normals as the forward did, stores its four g_lat values with one 16-B store and adds its
// terms of g_std; then it stores the 4 A partial sums to scratch [P][L][A].  The price: the row tail (G, gn, gv:
// two exp, a tanh, a few divisions, wave-uniform) is recomputed in every pass.  Lane 0 stores g_mean in its
// first pass.  No lane waits for another; a lane at or past L stores nothing.
template <int A>
__global__ __launch_bounds__(kBlock) void USV_NOISE_KERNEL(sde_squash_backward)(
    SdeArgs a, USV_NOISE_EPOCH_PARAM int R, const float* __restrict__ mean, const float* __restrict__ lat,
    size_t stride, const float* __restrict__ std, const float* __restrict__ gauss, const float* __restrict__ var,
    const float* __restrict__ g_act, const float* __restrict__ g_logp, float* __restrict__ g_mean,
    float* __restrict__ g_lat, size_t g_stride, float* __restrict__ part) {
  USV_NOISE_PROLOGUE
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int l = lane_id();
  const int64_t p = (int64_t)blockIdx.x * kWaves + wave;
  const int64_t e0 = p * R;
  if (e0 >= a.n) return;                                // wave-uniform
  const int64_t e1 = e0 + R < a.n ? e0 + R : a.n;
  for (int j0 = kSdePerLane * l; j0 < a.L; j0 += kSdePass) {
    float s[4 * A], gs[4 * A];
#pragma unroll
    for (int i = 0; i < 4 * A; ++i) {
      s[i] = std[(size_t)j0 * A + i];
      gs[i] = 0.0f;
    }
    for (int64_t e = e0; e < e1; ++e) {
      const float gl = g_logp ? g_logp[e] : 0.0f;
      float gn[A], gv[A];
#pragma unroll
      for (int k = 0; k < A; ++k) {
        const size_t at = (size_t)e * A + k;
        float G;
        sde_squash_grad_tail(gauss[at], mean[at], var[at], g_act ? g_act[at] : 0.0f, gl, G, gn[k], gv[k]);
        if (j0 == 0) g_mean[at] = G;                    // lane 0, first pass
      }
      const float4 lv = *reinterpret_cast<const float4*>(lat + (size_t)e * stride + j0);
      const float x[4] = {lv.x, lv.y, lv.z, lv.w};
      float gx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int m = 0; m < A; ++m) {
        uint32_t o[4];
        float z[4];
        sde_block(a.seed, a.gid0 + (uint64_t)e, a.epoch, (uint32_t)(j0 / 4) * A + m, o);
        sde_normals(o, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = 4 * m + q;
          sde_grad_accum(x[i / A], s[i], z[q], gn[i % A], gv[i % A], gx[i / A], gs[i]);
        }
      }
      *reinterpret_cast<float4*>(g_lat + (size_t)e * g_stride + j0) = make_float4(gx[0], gx[1], gx[2], gx[3]);
    }
    float* const dst = part + ((size_t)p * a.L + j0) * A;     // 16-B aligned: scratch is, and (p L + j0) A % 4 == 0
#pragma unroll
    for (int m = 0; m < A; ++m)
      *reinterpret_cast<float4*>(dst + 4 * m) = make_float4(gs[4 * m], gs[4 * m + 1], gs[4 * m + 2], gs[4 * m + 3]);
  }
}

// blocks_per_env = L * A / 4; thread t of the grid owns block t % blocks_per_env of env t / blocks_per_env.
template <int A>
__global__ __launch_bounds__(kBlock) void USV_NOISE_KERNEL(sde_weights)(
    SdeArgs a, USV_NOISE_EPOCH_PARAM const float* __restrict__ std, float* __restrict__ w) {
  USV_NOISE_PROLOGUE
  const int bpe = a.L * A / 4;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= (int64_t)a.n * bpe) return;
  const int64_t e = t / bpe;
  const uint32_t b = (uint32_t)(t - e * bpe);
  uint32_t o[4];
  float z[4];
  sde_block(a.seed, a.gid0 + (uint64_t)e, a.epoch, b, o);
  sde_normals(o, z);
  float* const dst = w + (size_t)e * a.L * A + 4 * (size_t)b;
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[q] = sde_weight(std[4 * (size_t)b + q], z[q]);
}
