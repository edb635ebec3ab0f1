// The pieces of the Squeeze-and-Excitation tail that do not depend on the gate's width, shared by se.hip (C <= 512, the
// BasicBlock nets) and se_wide.hip (C <= 2048, the bottleneck nets): the elementwise scale kernels
// (grid-stride, any C % 8 == 0) and the fold of the parameter-gradient partials.
#pragma once
#include "layer_shared.h"      // Bn4: the recomputed BatchNorm affine of a channel quad

// thread = 8 channels of one position: out and one byte of ReLU decisions (bit e = channel c0 + e; byte index = element / 8)
static __global__ __launch_bounds__(256) void se_scale_fwd_kernel(const float* __restrict__ y2, const float* __restrict__ res,
                                                           float* __restrict__ out, unsigned char* __restrict__ mask, size_t npos,
                                                           int L, int Wn, int C, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ s) {
  const int no = C >> 3;
  const size_t total = npos * no;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int o8 = (int)(idx % no);
    const size_t pos = idx / no, row = pos / L, w = pos / Wn;
    unsigned bits = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c0 = o8 * 8 + h * 4;
      Bn4 bn;
      bn.load(mean, invstd, gamma, beta, w, C, c0);
      const f32x4 z = bn.z(*reinterpret_cast<const f32x4*>(y2 + pos * C + c0));
      const f32x4 sv = *reinterpret_cast<const f32x4*>(s + row * C + c0);
      const f32x4 rv = *reinterpret_cast<const f32x4*>(res + pos * C + c0);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = fmaxf(fmaf(z[e], sv[e], rv[e]), 0.f);
        bits |= (o[e] > 0.f ? 1u : 0u) << (h * 4 + e);
      }
      *reinterpret_cast<f32x4*>(out + pos * C + c0) = o;
    }
    mask[idx] = (unsigned char)bits;
  }
}

// the chunks folded in chunk order into the four destinations
static __global__ __launch_bounds__(256) void se_pgrad_fold_kernel(const float* __restrict__ part, int nchunks, int C, int Cr,
                                                            float* __restrict__ dw2, float* __restrict__ db2,
                                                            float* __restrict__ dw1, float* __restrict__ db1, int accumulate) {
  const int P = 2 * C * Cr + C + Cr;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float t = 0.f;
  for (int k = 0; k < nchunks; ++k) t += part[(size_t)k * P + i];
  float* o;
  if (i < C * Cr) o = dw2 + i;
  else if (i < C * Cr + C) o = db2 + (i - C * Cr);
  else if (i < 2 * C * Cr + C) o = dw1 + (i - C * Cr - C);
  else o = db1 + (i - 2 * C * Cr - C);
  *o = accumulate ? *o + t : t;
}

static __global__ __launch_bounds__(256) void se_bwd_scale_kernel(const float* __restrict__ g, const float* __restrict__ s,
                                                           const float* __restrict__ dpool, float* __restrict__ dz, size_t npos,
                                                           int L, int C) {
  const int nq = C >> 2;
  const size_t total = npos * nq;
  const float fl = (float)L;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    const size_t pos = idx / nq, row = pos / L;
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + pos * C + c0);
    const f32x4 sv = *reinterpret_cast<const f32x4*>(s + row * C + c0);
    const f32x4 dv = *reinterpret_cast<const f32x4*>(dpool + row * C + c0);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaf(gv[e], sv[e], dv[e] / fl);
    *reinterpret_cast<f32x4*>(dz + pos * C + c0) = o;
  }
}

