// usv_caps_noise.inc -- caps_perturb_kernel, stated once and included twice by usv_caps.hpp, as usv_sde_noise.inc is:
//   USV_NOISE_KERNEL(name)   name_kernel, then name_dev_kernel
//   USV_NOISE_EPOCH_PARAM    nothing, then `, const uint32_t* __restrict__ epoch_dev`
//   USV_NOISE_PROLOGUE       nothing, then `a.epoch = sde_epoch_word(epoch_dev);`
__global__ __launch_bounds__(kBlock) void USV_NOISE_KERNEL(caps_perturb)(CapsPerturbArgs a USV_NOISE_EPOCH_PARAM) {
  USV_NOISE_PROLOGUE
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= a.blocks) return;
  const long long r = t / a.row_blocks;
  const int b = (int)(t - r * a.row_blocks);
  const int count = a.W - 4 * b < 4 ? a.W - 4 * b : 4;
  const long long at = r * a.W + 4 * b;
  const float* const src = a.obs + at;
  float* const dst = a.out + at;
  float z[4];
  caps_block_normals(a.seed, (uint64_t)r, a.epoch, (uint32_t)b, z);
  if (count == 4 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    float4 v = *reinterpret_cast<const float4*>(src);
    v.x = caps_near(v.x, a.eps, z[0]);
    v.y = caps_near(v.y, a.eps, z[1]);
    v.z = caps_near(v.z, a.eps, z[2]);
    v.w = caps_near(v.w, a.eps, z[3]);
    *reinterpret_cast<float4*>(dst) = v;
    return;
  }
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (q < count) v[q] = src[q];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (q < count) dst[q] = caps_near(v[q], a.eps, z[q]);
}
