// The two larger pieces the layer files share (se_tail.h and through it se.hip / se_wide.hip; vgg.hip, autoencoder.hip,
// unet.hip): the recomputed BatchNorm affine of a channel quad and the fold of a loss's block partials.
#pragma once
#include "common.h"

// scale / shift, mean and invstd of 4 channels of window w.  Forward and backward of a layer form z through THIS struct from
// the same (mean, invstd, gamma, beta) floats, so they agree bit for bit on every ReLU and pool decision taken from z.
struct Bn4 {
  f32x4 sc, sh, mu, is;
  __device__ __forceinline__ void load(const float* __restrict__ mean, const float* __restrict__ invstd,
                                       const float* __restrict__ gamma, const float* __restrict__ beta, size_t w, int C, int c0) {
    mu = ld4(mean + w * C + c0);
    is = ld4(invstd + w * C + c0);
    const f32x4 ga = ld4(gamma + c0), be = ld4(beta + c0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a, b;
      bn_scale_shift(mu[e], is[e], ga[e], be[e], a, b);
      sc[e] = a;
      sh[e] = b;
    }
  }
  __device__ __forceinline__ f32x4 z(const f32x4& y) const {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = fmaf(y[e], sc[e], sh[e]);
    return r;
  }
};

// loss[0] = inv_n sum of the block partials: thread t takes partials t, t + 256, ... in order, then the 256 in order
static __global__ __launch_bounds__(256) void loss_fold_kernel(const float* __restrict__ partials, int n, float inv_n,
                                                               float* __restrict__ loss) {
  __shared__ float red[256];
  float t = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) t += partials[i];
  red[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < 256; ++i) s += red[i];
    loss[0] = s * inv_n;
  }
}
