// The memory-bound layers between the convs of the reference's UNet (models/unet.py: double_conv = Conv1d(k3, p1, bias) -> ReLU
// twice, MaxPool1d(2) with the full-resolution map kept as a skip, Upsample(scale_factor=2, 'linear', align_corners=True),
// torch.cat with the skip, Conv1d(64, 1, 1); MSELoss against the input).  NO BatchNorm: the conv biases are real.
//
//     bias_relu        a = relu(y + b) in place
//     pool             a = relu(y + b) in place (the skip: it stays where the conv wrote it, in the concat buffer) and
//                      pooled[j] = a[2j+1] > a[2j] ? a[2j+1] : a[2j]   (ATen's MaxPool1d: the second wins only when strictly greater)
//     upsample         x = relu(y + b) formed on the fly, never stored;  D = 2L - 1:
//                      out[2j+1] = ((L+j)/D) x[j] + ((L-1-j)/D) x[j+1];  out[0] = x[0];  out[2j] = ((D-j)/D) x[j] + (j/D) x[j-1]
//                      (align_corners=True at scale 2, exact in rationals; every weight an integer ratio rounded once)
//     output           recon[n][l] = b + sum_c a[n][l][c] w[c];  dr = 2 (recon - x) / (rows L);  loss = mean (recon - x)^2
//
// float activations (rows, L, C) channels-last, C % 32 == 0; a thread owns 4 channels (16-byte accesses); operands named with a
// pitch may be channel slices of a pitched buffer (ld >= C, ld % 4 == 0).  No pool decision is stored: the backward re-derives
// the winner from the stored a.  relu is v > 0 ? v : +0.0 everywhere, and a mask is the same float compare.
//
// Every sum runs in an order fixed by the shape alone (thread-private chains, xor-shuffle trees, LDS folds in slot order, block
// partials folded in index order): no atomics, the same bits every call.  Nothing is allocated or synchronised here.
#include "layer_shared.h"      // loss_fold_kernel

#define UN_OUT_C 64                   // channels in front of conv_last (Conv1d(64, 1, 1))
#define UN_OUT_POS 16                 // positions per block pass of the output stage: 16 quads x 16 positions
#define UN_OUT_BLOCKS 512             // most blocks (= partials / records) of an output-stage launch
#define UN_OUT_REC 68                 // floats per block record of the output backward: dw [64], db, padding

enum { UN_BIAS_RELU = 0, UN_POOL_FWD, UN_UP_FWD, UN_UP_BWD, UN_POOL_SKIP_BWD, UN_RELU_BWD, UN_OUT_FWD, UN_OUT_BWD, UN_OPS };

__device__ __forceinline__ f32x4 un_relu_add(const f32x4& y, const f32x4& b) {
  f32x4 a;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float v = y[e] + b[e];
    a[e] = v > 0.f ? v : 0.f;
  }
  return a;
}

// ---- a = relu(y + b) in place: thread = 4 channels of one position ---------------------------------------------------------------
__global__ __launch_bounds__(256) void un_bias_relu_kernel(float* __restrict__ y, int ld, const float* __restrict__ bias, size_t npos,
                                                           int C) {
  const int nq = C >> 2;
  const size_t total = npos * nq;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    float* p = y + (idx / nq) * (size_t)ld + c0;
    st4(p, un_relu_add(ld4(p), ld4(bias + c0)));
  }
}

// ---- relu + MaxPool1d(2): thread = 4 channels of one pair (positions 2j, 2j + 1 of a row: pair pr overall is position 2 pr) ------
__global__ __launch_bounds__(256) void un_pool_fwd_kernel(float* __restrict__ y, int ld, const float* __restrict__ bias,
                                                          float* __restrict__ pooled, size_t npairs, int C) {
  const int nq = C >> 2;
  const size_t total = npairs * nq;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    const size_t pr = idx / nq;
    float* p = y + 2 * pr * (size_t)ld + c0;
    const f32x4 b = ld4(bias + c0);
    const f32x4 a0 = un_relu_add(ld4(p), b), a1 = un_relu_add(ld4(p + ld), b);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = a1[e] > a0[e] ? a1[e] : a0[e];
    st4(p, a0);
    st4(p + ld, a1);
    st4(pooled + pr * C + c0, o);
  }
}

// ---- relu + upsample x2: thread = 4 channels of one low-resolution position j; writes out[2j], out[2j + 1] ------------------------
__global__ __launch_bounds__(256) void un_up_fwd_kernel(const float* __restrict__ y, const float* __restrict__ bias,
                                                        float* __restrict__ out, int ldo, size_t npos, int L, int C) {
  const int nq = C >> 2;
  const size_t total = npos * nq;
  const float D = (float)(2 * L - 1);
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    const size_t pos = idx / nq;
    const int j = (int)(pos % L);
    const float* p = y + pos * C + c0;
    const f32x4 b = ld4(bias + c0), zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 x = un_relu_add(ld4(p), b);
    const f32x4 xm = j > 0 ? un_relu_add(ld4(p - C), b) : zero;          // (weight j / D = 0 at j = 0: never read)
    const f32x4 xp = j < L - 1 ? un_relu_add(ld4(p + C), b) : zero;      // (weight (L - 1 - j) / D = 0 at j = L - 1)
    const float we = (float)(2 * L - 1 - j) / D, wm = (float)j / D;        // out[2j]
    const float wo = (float)(L + j) / D, wp = (float)(L - 1 - j) / D;      // out[2j + 1]
    f32x4 oe, oo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      oe[e] = fmaf(wm, xm[e], we * x[e]);
      oo[e] = fmaf(wp, xp[e], wo * x[e]);
    }
    float* o = out + 2 * pos * (size_t)ldo + c0;
    st4(o, oe);
    st4(o + ldo, oo);
  }
}

// ---- its transpose as a gather of at most four terms in a fixed order, masked by y + b > 0 ----------------------------------------
__global__ __launch_bounds__(256) void un_up_bwd_kernel(const float* __restrict__ d, int ld, const float* __restrict__ y,
                                                        const float* __restrict__ bias, float* __restrict__ dy, size_t npos, int L,
                                                        int C) {
  const int nq = C >> 2;
  const size_t total = npos * nq;
  const float D = (float)(2 * L - 1);
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    const size_t pos = idx / nq;
    const int j = (int)(pos % L);
    const float* q = d + 2 * pos * (size_t)ld + c0;                        // d[2j] of this row
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 d1 = ld4(q + ld), d0 = ld4(q);
    const f32x4 dm = j > 0 ? ld4(q - ld) : zero, dp = j < L - 1 ? ld4(q + 2 * (size_t)ld) : zero;
    const float w1 = (float)(L + j) / D, w0 = (float)(2 * L - 1 - j) / D, wm = (float)(L - j) / D, wp = (float)(j + 1) / D;
    const f32x4 yv = ld4(y + pos * C + c0), b = ld4(bias + c0);
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = fmaf(w0, d0[e], w1 * d1[e]);
      if (j > 0) t = fmaf(wm, dm[e], t);
      if (j < L - 1) t = fmaf(wp, dp[e], t);
      g[e] = yv[e] + b[e] > 0.f ? t : 0.f;
    }
    st4(dy + pos * C + c0, g);
  }
}

// ---- the two gradients that reach a skip map: thread = 4 channels of one pair ------------------------------------------------------
__global__ __launch_bounds__(256) void un_pool_skip_bwd_kernel(const float* __restrict__ dpooled, const float* __restrict__ dskip,
                                                               int ld, const float* __restrict__ a, int lda, float* __restrict__ dy,
                                                               size_t npairs, int C) {
  const int nq = C >> 2;
  const size_t total = npairs * nq;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    const size_t pr = idx / nq;
    const float* pa = a + 2 * pr * (size_t)lda + c0;
    const float* ps = dskip + 2 * pr * (size_t)ld + c0;
    const f32x4 a0 = ld4(pa), a1 = ld4(pa + lda), s0 = ld4(ps), s1 = ld4(ps + ld), dp = ld4(dpooled + pr * C + c0);
    f32x4 g0, g1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool second = a1[e] > a0[e];
      const float t0 = second ? s0[e] : s0[e] + dp[e], t1 = second ? s1[e] + dp[e] : s1[e];
      g0[e] = a0[e] > 0.f ? t0 : 0.f;
      g1[e] = a1[e] > 0.f ? t1 : 0.f;
    }
    float* o = dy + 2 * pr * C + c0;
    st4(o, g0);
    st4(o + C, g1);
  }
}

// ---- dy = dout [a > 0] (dy may be dout) --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void un_relu_bwd_kernel(const float* dout, const float* __restrict__ a, int lda, float* dy, size_t npos,
                                                          int C) {
  const int nq = C >> 2;
  const size_t total = npos * nq;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    const size_t pos = idx / nq;
    const f32x4 av = ld4(a + pos * (size_t)lda + c0), d = ld4(dout + pos * C + c0);
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = av[e] > 0.f ? d[e] : 0.f;
    st4(dy + pos * C + c0, g);
  }
}

// ---- the output stage: Conv1d(64, 1, 1) and the MSE against x; thread = (position of 16, channel quad of 16) ----------------------
__global__ __launch_bounds__(256) void un_out_fwd_kernel(const float* __restrict__ a, const float* __restrict__ w,
                                                         const float* __restrict__ bias, const float* __restrict__ x,
                                                         float* __restrict__ recon, float* __restrict__ dr,
                                                         float* __restrict__ partials, size_t npos, float scale) {
  __shared__ float red[UN_OUT_POS];
  const int quad = threadIdx.x & 15, ps = threadIdx.x >> 4;
  const f32x4 wv = ld4(w + quad * 4);
  const float b = bias[0];
  float sq = 0.f;
  for (size_t base = (size_t)blockIdx.x * UN_OUT_POS; base < npos; base += (size_t)gridDim.x * UN_OUT_POS) {
    const size_t pos = base + ps;
    const bool valid = pos < npos;
    float r = 0.f;
    if (valid) {
      const f32x4 av = ld4(a + pos * UN_OUT_C + quad * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) r = fmaf(av[e], wv[e], r);
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) r += __shfl_xor(r, o, 64);       // the 16 quads of a position: neighbouring lanes
    if (valid && quad == 0) {
      const float rc = r + b, e0 = rc - x[pos];
      recon[pos] = rc;
      dr[pos] = e0 * scale;
      sq = fmaf(e0, e0, sq);
    }
  }
  if (quad == 0) red[ps] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int s = 0; s < UN_OUT_POS; ++s) t += red[s];
    partials[blockIdx.x] = t;
  }
}

// dy = dr w [a > 0];  rec[block][c] = sum over the block's positions of dr a[c];  rec[block][64] = sum dr
__global__ __launch_bounds__(256) void un_out_bwd_kernel(const float* __restrict__ drp, const float* __restrict__ a,
                                                         const float* __restrict__ w, float* __restrict__ dy, float* __restrict__ rec,
                                                         size_t npos) {
  __shared__ float red[UN_OUT_POS][UN_OUT_C + 1];
  const int quad = threadIdx.x & 15, ps = threadIdx.x >> 4;
  const f32x4 wv = ld4(w + quad * 4);
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, sdr = 0.f;
  for (size_t base = (size_t)blockIdx.x * UN_OUT_POS; base < npos; base += (size_t)gridDim.x * UN_OUT_POS) {
    const size_t pos = base + ps;
    if (pos >= npos) continue;
    const float d = drp[pos];
    const f32x4 av = ld4(a + pos * UN_OUT_C + quad * 4);
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      g[e] = av[e] > 0.f ? d * wv[e] : 0.f;
      acc[e] = fmaf(d, av[e], acc[e]);
    }
    sdr += d;
    st4(dy + pos * UN_OUT_C + quad * 4, g);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[ps][quad * 4 + e] = acc[e];
  if (quad == 0) red[ps][UN_OUT_C] = sdr;
  __syncthreads();
  if (threadIdx.x <= UN_OUT_C) {
    float t = 0.f;
    for (int s = 0; s < UN_OUT_POS; ++s) t += red[s][threadIdx.x];
    rec[(size_t)blockIdx.x * UN_OUT_REC + threadIdx.x] = t;
  }
}

// one block: thread = (sum of 65 [padded to 128], slot of 2): slot s folds records s, s + 2, ... in order, then slot 0 + slot 1
__global__ __launch_bounds__(256) void un_out_bwd_merge_kernel(const float* __restrict__ rec, int nrec, float* __restrict__ dw,
                                                               float* __restrict__ db, int accumulate) {
  __shared__ float red[2][128];
  const int i = threadIdx.x & 127, slot = threadIdx.x >> 7;
  float t = 0.f;
  if (i <= UN_OUT_C)
    for (int r = slot; r < nrec; r += 2) t += rec[(size_t)r * UN_OUT_REC + i];
  red[slot][i] = t;
  __syncthreads();
  if (slot == 0 && i <= UN_OUT_C) {
    const float s = red[0][i] + red[1][i];
    float* dst = i < UN_OUT_C ? dw + i : db;
    *dst = accumulate ? *dst + s : s;
  }
}

// a (rows, L, C) map at channel pitch ld: 32-bit element offsets, and L small enough for the upsample's integer weights
static bool un_shape_ok(int rows, int L, int C, int ld) {
  return rows >= 0 && L >= 1 && L < (1 << 22) && C >= 32 && C % 32 == 0 && ld >= C && ld % 4 == 0 &&
         fits32((size_t)rows, (size_t)L, (size_t)ld);
}

static int un_out_blocks(int rows, int L) {
  const size_t b = ((size_t)rows * L + UN_OUT_POS - 1) / UN_OUT_POS;
  return (int)(b < UN_OUT_BLOCKS ? b : UN_OUT_BLOCKS);
}

extern "C" {

// Launch geometry of entry point `op` (the order of the declarations below: 0 da_unet_bias_relu ... 7 da_unet_out_bwd) on a
// (rows, L, C) map whose widest operand has channel pitch ld, without launching: blocks of 256 threads of its main kernel and
// the bytes of workspace it asks for.  L is the length the entry point is called with (the pool's full-resolution length, the
// upsample's LOW-resolution length); DA_EINVAL for a shape the entry point refuses.
int da_unet_plan(int op, int rows, int L, int C, int ld, int* blocks, size_t* workspace) {
  if (!blocks || !workspace || op < 0 || op >= UN_OPS || rows < 1) return DA_EINVAL;
  const bool pairs = op == UN_POOL_FWD || op == UN_POOL_SKIP_BWD, up = op == UN_UP_FWD || op == UN_UP_BWD;
  if (pairs && (L < 2 || L % 2)) return DA_EINVAL;
  if (!un_shape_ok(rows, up ? 2 * L : L, C, ld)) return DA_EINVAL;    // (the upsample's pitched operand has 2 L positions)
  *workspace = 0;
  if (op == UN_OUT_FWD || op == UN_OUT_BWD) {
    if (C != UN_OUT_C || ld != C) return DA_EINVAL;
    *blocks = un_out_blocks(rows, L);
    *workspace = (size_t)*blocks * (op == UN_OUT_FWD ? 1 : UN_OUT_REC) * sizeof(float);
    return DA_OK;
  }
  *blocks = grid_stride_blocks((size_t)rows * (pairs ? L / 2 : L) * (C / 4));
  return DA_OK;
}

#define UN_PLAN(op, L, ld)                                                              \
  int blocks;                                                                           \
  size_t ws;                                                                            \
  if (g_act_bf16 || rows < 0) return DA_EINVAL;                                         \
  if (rows == 0) return DA_OK;                                                          \
  if (da_unet_plan(op, rows, L, C, ld, &blocks, &ws) != DA_OK) return DA_EINVAL;        \
  (void)ws

// y [rows][L][ld] (C channels of it) = relu(y + bias)
int da_unet_bias_relu(float* y, int ld, const float* bias, int rows, int L, int C, hipStream_t stream) {
  DA_ENTER();
  if (!y || !bias) return DA_EINVAL;
  UN_PLAN(UN_BIAS_RELU, L, ld);
  hipLaunchKernelGGL(un_bias_relu_kernel, dim3(blocks), dim3(256), 0, stream, y, ld, bias, (size_t)rows * L, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// y [rows][L][ld] = relu(y + bias) in place;  pooled [rows][L / 2][C] = MaxPool1d(2) of it
int da_unet_bias_relu_pool2_fwd(float* y, int ld, const float* bias, float* pooled, int rows, int L, int C, hipStream_t stream) {
  DA_ENTER();
  if (!y || !bias || !pooled) return DA_EINVAL;
  UN_PLAN(UN_POOL_FWD, L, ld);
  hipLaunchKernelGGL(un_pool_fwd_kernel, dim3(blocks), dim3(256), 0, stream, y, ld, bias, pooled, (size_t)rows * (L / 2), C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// y [rows][L][C] -> out [rows][2 L][ld_out] = upsample2(relu(y + bias))
int da_unet_relu_upsample2_fwd(const float* y, const float* bias, float* out, int ld_out, int rows, int L, int C, hipStream_t stream) {
  DA_ENTER();
  if (!y || !bias || !out) return DA_EINVAL;
  UN_PLAN(UN_UP_FWD, L, ld_out);
  hipLaunchKernelGGL(un_up_fwd_kernel, dim3(blocks), dim3(256), 0, stream, y, bias, out, ld_out, (size_t)rows * L, L, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// d [rows][2 L][ld], y [rows][L][C] -> dy [rows][L][C] = upsample2^T(d) [y + bias > 0]
int da_unet_relu_upsample2_bwd(const float* d, int ld, const float* y, const float* bias, float* dy, int rows, int L, int C,
                               hipStream_t stream) {
  DA_ENTER();
  if (!d || !y || !bias || !dy) return DA_EINVAL;
  UN_PLAN(UN_UP_BWD, L, ld);
  hipLaunchKernelGGL(un_up_bwd_kernel, dim3(blocks), dim3(256), 0, stream, d, ld, y, bias, dy, (size_t)rows * L, L, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// dpooled [rows][L / 2][C], dskip [rows][L][ld], a [rows][L][ld_a] (the stored skip) -> dy [rows][L][C]
int da_unet_pool2_skip_bwd(const float* dpooled, const float* dskip, int ld, const float* a, int ld_a, float* dy, int rows, int L,
                           int C, hipStream_t stream) {
  DA_ENTER();
  if (!dpooled || !dskip || !a || !dy) return DA_EINVAL;
  UN_PLAN(UN_POOL_SKIP_BWD, L, ld > ld_a ? ld : ld_a);
  if (!un_shape_ok(rows, L, C, ld) || !un_shape_ok(rows, L, C, ld_a)) return DA_EINVAL;
  hipLaunchKernelGGL(un_pool_skip_bwd_kernel, dim3(blocks), dim3(256), 0, stream, dpooled, dskip, ld, a, ld_a, dy,
                     (size_t)rows * (L / 2), C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// dout [rows][L][C], a [rows][L][ld_a] -> dy [rows][L][C] = dout [a > 0]; dy may be dout
int da_unet_relu_bwd(const float* dout, const float* a, int ld_a, float* dy, int rows, int L, int C, hipStream_t stream) {
  DA_ENTER();
  if (!dout || !a || !dy) return DA_EINVAL;
  UN_PLAN(UN_RELU_BWD, L, ld_a);
  hipLaunchKernelGGL(un_relu_bwd_kernel, dim3(blocks), dim3(256), 0, stream, dout, a, ld_a, dy, (size_t)rows * L, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// a [rows][L][64], w [64], bias [1], x [rows][L] -> recon, dr [rows][L], loss[1]; partials: da_unet_plan(6)'s workspace
int da_unet_out_fwd(const float* a, const float* w, const float* bias, const float* x, float* recon, float* dr, float* partials,
                    float* loss, int rows, int L, hipStream_t stream) {
  DA_ENTER();
  const int C = UN_OUT_C;
  if (!a || !w || !bias || !x || !recon || !dr || !partials || !loss || rows < 1) return DA_EINVAL;
  UN_PLAN(UN_OUT_FWD, L, C);
  const float n = (float)rows * (float)L;
  hipLaunchKernelGGL(un_out_fwd_kernel, dim3(blocks), dim3(256), 0, stream, a, w, bias, x, recon, dr, partials, (size_t)rows * L,
                     2.0f / n);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_fold_kernel, dim3(1), dim3(256), 0, stream, partials, blocks, 1.0f / n, loss);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// dr [rows][L], a [rows][L][64] -> dy [rows][L][64] = dr w [a > 0], dw [64] and db [1] (+)=; workspace: da_unet_plan(7)'s
int da_unet_out_bwd(const float* dr, const float* a, const float* w, float* dy, float* dw, float* db, float* workspace, int rows,
                    int L, int accumulate, hipStream_t stream) {
  DA_ENTER();
  const int C = UN_OUT_C;
  if (!dr || !a || !w || !dy || !dw || !db || !workspace || rows < 1) return DA_EINVAL;
  UN_PLAN(UN_OUT_BWD, L, C);
  hipLaunchKernelGGL(un_out_bwd_kernel, dim3(blocks), dim3(256), 0, stream, dr, a, w, dy, workspace, (size_t)rows * L);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(un_out_bwd_merge_kernel, dim3(1), dim3(256), 0, stream, workspace, blocks, dw, db, accumulate ? 1 : 0);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
