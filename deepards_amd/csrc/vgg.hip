// The pooled stages and the feature layout of the VGG backbones (reference models/vgg.py:37-50 make_layers, :15,20-24):
//
//     stage      out[row][j][c] = max(relu(z[2j]), relu(z[2j+1])),   z = bn(y) = fmaf(y, sc, sh)   (bn_scale_shift, common.h)
//     features   feat[row][c * Lout + i] = mean of x[row][floor(i Lin / Lout) : ceil((i + 1) Lin / Lout)][c]
//
// float activations (rows, L, C) channels-last, BatchNorm windows of R rows, statistics (W, C).  The activated full-resolution
// map relu(z) is NEVER stored, and neither is its gradient dz: the backward recomputes z, the ReLU decision and the pool's
// routing from the stored conv output y in both of its passes, through ONE device function, so the two passes and the forward
// agree bit for bit on where a gradient goes.
//
//   da_bn_relu_maxpool2_fwd   one pass over y
//   da_bn_relu_maxpool2_bwd   pass 1: per (window, channel) sums of dz and dz xhat, as chunk partials folded in chunk order;
//                             pass 2: dy = gamma invstd (dz - sum dz / n - xhat sum dz xhat / n), n = R Lin.
//                             MaxPool1d(2, 2) floors: the last position of an odd row is in no pair -- its dz is 0, but it is
//                             part of the BatchNorm window, so its dy is NOT 0 (the two mean terms remain).
//   da_bn_mean_bias           mean + conv bias per window (the running mean of BN(conv + b)); optionally writes the exact zero
//                             that is the conv bias's gradient
//   da_adaptive_avgpool_flat_fwd / _bwd
//
// Every sum runs in an order fixed by the shape alone (thread-private chains, LDS folds in slot order, partials in chunk order):
// no atomics, the same bits every call.  Nothing is allocated or synchronised here.
#include "layer_shared.h"      // Bn4

#define VP_CG 32                      // channels per block of the backward passes: 8 quads x 32 slots = 256 threads
#define VP_SLOTS 32
#define VP_CHUNK 256                  // pairs per block (8 per slot)

// The gradient of the two members of a pool pair from the pair's gradient d: the pool hands it to the FIRST maximum of
// (relu(z0), relu(z1)) (ATen's MaxPool1d: the second wins only when strictly greater), the ReLU passes it where z > 0.
__device__ __forceinline__ void vp_route(float z0, float z1, float d, float& g0, float& g1) {
  const float a0 = fmaxf(z0, 0.f), a1 = fmaxf(z1, 0.f);
  const bool first = a0 >= a1;
  g0 = (first && z0 > 0.f) ? d : 0.f;
  g1 = first ? 0.f : d;                 // (a1 > a0 >= 0: z1 > 0)
}

// ---- forward: thread = 4 channels of one output position ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void vp_fwd_kernel(const float* __restrict__ y, int ldy, float* __restrict__ out, size_t npairs,
                                                     int Lo, int Lin, int R, int C, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta) {
  const int nq = C >> 2;
  const size_t total = npairs * nq;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    const size_t pr = idx / nq, row = pr / Lo, j = pr - row * Lo;
    Bn4 bn;
    bn.load(mean, invstd, gamma, beta, row / R, C, c0);
    const float* p = y + (row * Lin + 2 * j) * (size_t)ldy + c0;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + ldy);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaxf(fmaxf(fmaf(a[e], bn.sc[e], bn.sh[e]), fmaf(b[e], bn.sc[e], bn.sh[e])), 0.f);
    *reinterpret_cast<f32x4*>(out + pr * C + c0) = o;
  }
}

// ---- backward, pass 1: block = (window, 32 channels, chunk of VP_CHUNK pairs); thread = (channel quad, slot) ------------------
// part[w][chunk][{sum dz, sum dz xhat}][C]
__global__ __launch_bounds__(256) void vp_bwd_partial_kernel(const float* __restrict__ dout, const float* __restrict__ y, int ldy,
                                                             float* __restrict__ part, int R, int Lin, int Lo, int C,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta) {
  __shared__ float red[2][VP_SLOTS][VP_CG];
  const int w = blockIdx.x, cg = blockIdx.y, pc = blockIdx.z, P = gridDim.z;
  const int q = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int c0 = cg * VP_CG + q * 4;
  Bn4 bn;
  bn.load(mean, invstd, gamma, beta, (size_t)w, C, c0);
  const int npw = R * Lo, p_beg = pc * VP_CHUNK, p_end = min(npw, p_beg + VP_CHUNK);
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pi = p_beg + slot; pi < p_end; pi += VP_SLOTS) {
    const int r = pi / Lo, j = pi - r * Lo;
    const size_t row = (size_t)w * R + r;
    const float* p = y + (row * Lin + 2 * j) * (size_t)ldy + c0;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + ldy);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dout + (row * Lo + j) * (size_t)C + c0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float g0, g1;
      vp_route(fmaf(a[e], bn.sc[e], bn.sh[e]), fmaf(b[e], bn.sc[e], bn.sh[e]), d[e], g0, g1);
      s1[e] += g0 + g1;                                              // (one of the two is 0: exact)
      s2[e] = fmaf(g0, (a[e] - bn.mu[e]) * bn.is[e], s2[e]);
      s2[e] = fmaf(g1, (b[e] - bn.mu[e]) * bn.is[e], s2[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[0][slot][q * 4 + e] = s1[e];
    red[1][slot][q * 4 + e] = s2[e];
  }
  __syncthreads();
  if (threadIdx.x < 2 * VP_CG) {
    const int k = threadIdx.x >> 5, c = threadIdx.x & 31;
    float t = 0.f;
    for (int s = 0; s < VP_SLOTS; ++s) t += red[k][s][c];
    part[(((size_t)w * P + pc) * 2 + k) * C + cg * VP_CG + c] = t;
  }
}

// ---- backward, pass 2: the same blocks; the chunk partials folded in chunk order by every thread for its 4 channels -----------
__global__ __launch_bounds__(256) void vp_bwd_apply_kernel(const float* __restrict__ dout, const float* __restrict__ y, int ldy,
                                                           float* __restrict__ dy, const float* __restrict__ part,
                                                           float* __restrict__ ds1, float* __restrict__ ds2, int R, int Lin, int Lo,
                                                           int C, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta) {
  const int w = blockIdx.x, cg = blockIdx.y, pc = blockIdx.z, P = gridDim.z;
  const int q = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int c0 = cg * VP_CG + q * 4;
  Bn4 bn;
  bn.load(mean, invstd, gamma, beta, (size_t)w, C, c0);
  const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c0);
  f32x4 t1 = {0.f, 0.f, 0.f, 0.f}, t2 = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < P; ++p) {
    const float* o = part + (((size_t)w * P + p) * 2) * C + c0;
    const f32x4 a = *reinterpret_cast<const f32x4*>(o), b = *reinterpret_cast<const f32x4*>(o + C);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      t1[e] += a[e];
      t2[e] += b[e];
    }
  }
  if (pc == 0 && slot == 0) {
    *reinterpret_cast<f32x4*>(ds1 + (size_t)w * C + c0) = t1;
    *reinterpret_cast<f32x4*>(ds2 + (size_t)w * C + c0) = t2;
  }
  const float inv_n = 1.0f / (float)(R * Lin);                     // the FULL window, a dropped odd position included
  f32x4 k, m1, m2;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    k[e] = ga[e] * bn.is[e];
    m1[e] = t1[e] * inv_n;
    m2[e] = t2[e] * inv_n;
  }
  const int npw = R * Lo, p_beg = pc * VP_CHUNK, p_end = min(npw, p_beg + VP_CHUNK);
  const bool odd = (Lin & 1) != 0;
  for (int pi = p_beg + slot; pi < p_end; pi += VP_SLOTS) {
    const int r = pi / Lo, j = pi - r * Lo;
    const size_t row = (size_t)w * R + r;
    const size_t pos = row * Lin + 2 * j;
    const float* p = y + pos * (size_t)ldy + c0;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + ldy);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dout + (row * Lo + j) * (size_t)C + c0);
    f32x4 da, db;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float g0, g1;
      vp_route(fmaf(a[e], bn.sc[e], bn.sh[e]), fmaf(b[e], bn.sc[e], bn.sh[e]), d[e], g0, g1);
      da[e] = k[e] * (g0 - m1[e] - (a[e] - bn.mu[e]) * bn.is[e] * m2[e]);
      db[e] = k[e] * (g1 - m1[e] - (b[e] - bn.mu[e]) * bn.is[e] * m2[e]);
    }
    *reinterpret_cast<f32x4*>(dy + pos * C + c0) = da;
    *reinterpret_cast<f32x4*>(dy + (pos + 1) * C + c0) = db;
    if (odd && j == Lo - 1) {                                       // the position the pool dropped: dz = 0, dy is not
      const f32x4 c = *reinterpret_cast<const f32x4*>(p + 2 * (size_t)ldy);
      f32x4 dc;
#pragma unroll
      for (int e = 0; e < 4; ++e) dc[e] = k[e] * (0.f - m1[e] - (c[e] - bn.mu[e]) * bn.is[e] * m2[e]);
      *reinterpret_cast<f32x4*>(dy + (pos + 2) * C + c0) = dc;
    }
  }
}

__global__ __launch_bounds__(256) void vp_mean_bias_kernel(const float* __restrict__ mean, const float* __restrict__ bias,
                                                           float* __restrict__ mean_b, int W, int C, float* __restrict__ dbias) {
  const int total = W * C;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int c = i % C;
    mean_b[i] = mean[i] + bias[c];
    if (dbias && i < C) dbias[i] = 0.f;
  }
}

// ---- AdaptiveAvgPool1d(Lout) + view: thread = one feature (c fastest: the reads coalesce) --------------------------------------
__device__ __forceinline__ void ap_window(int i, int Lin, int Lout, int& s, int& e) {
  s = (int)(((long long)i * Lin) / Lout);
  e = (int)((((long long)(i + 1)) * Lin + Lout - 1) / Lout);
}

__global__ __launch_bounds__(256) void ap_flat_fwd_kernel(const float* __restrict__ x, float* __restrict__ feat, size_t rows, int Lin,
                                                          int Lout, int C) {
  const size_t total = rows * Lout * C;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const size_t t = idx / C, row = t / Lout;
    const int i = (int)(t - row * Lout);
    int s, e;
    ap_window(i, Lin, Lout, s, e);
    float acc = 0.f;
    for (int l = s; l < e; ++l) acc += x[(row * Lin + l) * C + c];
    feat[(row * C + c) * Lout + i] = acc / (float)(e - s);
  }
}

// thread = one input element; the windows that hold position l, in window order
__global__ __launch_bounds__(256) void ap_flat_bwd_kernel(const float* __restrict__ dfeat, float* __restrict__ dx, size_t rows, int Lin,
                                                          int Lout, int C) {
  const size_t total = rows * Lin * C;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const size_t t = idx / C, row = t / Lin;
    const int l = (int)(t - row * Lin);
    // window i holds l iff floor(i Lin / Lout) <= l < ceil((i + 1) Lin / Lout): candidates lie between these two
    int i0 = (int)(((long long)l * Lout) / Lin) - 1, i1 = (int)((((long long)(l + 1)) * Lout + Lin - 1) / Lin);
    i0 = max(i0, 0);
    i1 = min(i1, Lout - 1);
    float acc = 0.f;
    for (int i = i0; i <= i1; ++i) {
      int s, e;
      ap_window(i, Lin, Lout, s, e);
      if (s <= l && l < e) acc += dfeat[(row * C + c) * Lout + i] / (float)(e - s);
    }
    dx[idx] = acc;
  }
}

extern "C" {

static bool vp_shape_ok(int rows, int R, int Lin, int C, int ldy) {
  return rows >= 0 && R >= 1 && rows % R == 0 && Lin >= 2 && C >= 32 && C % 32 == 0 && C / VP_CG <= 65535 && ldy >= C && ldy % 4 == 0 &&
         fits32((size_t)rows, (size_t)Lin, (size_t)ldy);
}

static int vp_chunks(int R, int Lin) { return (R * (Lin / 2) + VP_CHUNK - 1) / VP_CHUNK; }

// y [rows][Lin][ldy], statistics (W, C) -> out [rows][Lin / 2][C] = max(relu(bn(y[2j])), relu(bn(y[2j + 1])))
int da_bn_relu_maxpool2_fwd(const float* y, int ldy, float* out, int rows, int R, int Lin, int C, const float* mean,
                            const float* invstd, const float* gamma, const float* beta, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!y || !out || !mean || !invstd || !gamma || !beta || !vp_shape_ok(rows, R, Lin, C, ldy)) return DA_EINVAL;
  if (rows == 0) return DA_OK;
  const int Lo = Lin / 2;
  const size_t npairs = (size_t)rows * Lo;
  hipLaunchKernelGGL(vp_fwd_kernel, dim3(grid_stride_blocks(npairs * (C / 4))), dim3(256), 0, stream, y, ldy, out, npairs, Lo, Lin, R, C, mean,
                     invstd, gamma, beta);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// bytes of scratch da_bn_relu_maxpool2_bwd needs: the chunk partials [W][chunks][2][C]
size_t da_bn_relu_maxpool2_bwd_workspace(int rows, int R, int Lin, int C) {
  if (rows < 0 || R < 1 || rows % R || Lin < 2 || C < 1) return 0;
  return (size_t)(rows / R) * vp_chunks(R, Lin) * 2 * (size_t)C * sizeof(float);
}

// dout [rows][Lin / 2][C], y [rows][Lin][ldy] -> dy [rows][Lin][C], ds [2][W][C] (sum dz, sum dz xhat: da_bn_param_grad_multi)
int da_bn_relu_maxpool2_bwd(const float* dout, const float* y, int ldy, float* dy, float* ds, float* workspace, int rows, int R,
                            int Lin, int C, const float* mean, const float* invstd, const float* gamma, const float* beta,
                            hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!dout || !y || !dy || !ds || !workspace || !mean || !invstd || !gamma || !beta || !vp_shape_ok(rows, R, Lin, C, ldy))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  const int W = rows / R, Lo = Lin / 2, P = vp_chunks(R, Lin);
  if (P > 65535 || (size_t)R * Lin >= 0x7fffffffull) return DA_EINVAL;
  const dim3 grid(W, C / VP_CG, P);
  hipLaunchKernelGGL(vp_bwd_partial_kernel, grid, dim3(256), 0, stream, dout, y, ldy, workspace, R, Lin, Lo, C, mean, invstd, gamma,
                     beta);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(vp_bwd_apply_kernel, grid, dim3(256), 0, stream, dout, y, ldy, dy, workspace, ds, ds + (size_t)W * C, R, Lin, Lo, C,
                     mean, invstd, gamma, beta);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// mean_b[w][c] = mean[w][c] + bias[c]; dbias (may be NULL): C exact zeros
int da_bn_mean_bias(const float* mean, const float* bias, float* mean_b, int W, int C, float* dbias, hipStream_t stream) {
  DA_ENTER();
  if (!mean || !bias || !mean_b || W < 0 || C < 1 || (size_t)W * C >= 0x7fffffffull) return DA_EINVAL;
  if (W == 0 && !dbias) return DA_OK;
  if (W == 0) return DA_EINVAL;
  hipLaunchKernelGGL(vp_mean_bias_kernel, dim3(grid_stride_blocks((size_t)W * C)), dim3(256), 0, stream, mean, bias, mean_b, W, C, dbias);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// x [rows][Lin][C] -> feat [rows][C * Lout]
int da_adaptive_avgpool_flat_fwd(const float* x, float* feat, int rows, int Lin, int Lout, int C, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!x || !feat || rows < 0 || Lin < 1 || Lout < 1 || C < 1 || !fits32((size_t)rows, (size_t)Lin, (size_t)C) ||
      !fits32((size_t)rows, (size_t)Lout, (size_t)C))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  hipLaunchKernelGGL(ap_flat_fwd_kernel, dim3(grid_stride_blocks((size_t)rows * Lout * C)), dim3(256), 0, stream,
                     x, feat, (size_t)rows, Lin, Lout, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// dfeat [rows][C * Lout] -> dx [rows][Lin][C]
int da_adaptive_avgpool_flat_bwd(const float* dfeat, float* dx, int rows, int Lin, int Lout, int C, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!dfeat || !dx || rows < 0 || Lin < 1 || Lout < 1 || C < 1 || !fits32((size_t)rows, (size_t)Lin, (size_t)C) ||
      !fits32((size_t)rows, (size_t)Lout, (size_t)C))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  hipLaunchKernelGGL(ap_flat_bwd_kernel, dim3(grid_stride_blocks((size_t)rows * Lin * C)), dim3(256), 0, stream,
                     dfeat, dx, (size_t)rows, Lin, Lout, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
