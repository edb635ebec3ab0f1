// The layers of the reference's autoencoder that no other model has (models/autoencoder_cnn.py: four Conv1d / BatchNorm1d /
// MaxPool1d(2, return_indices) stages, four MaxUnpool1d(2) / ConvTranspose1d stages, NO ReLU; MSELoss against the input):
//
//     pool     out[row][j][c] = sel ? z[2j+1] : z[2j],   z = bn(y) = fmaf(y, sc, sh)   (bn_scale_shift, common.h)
//              sel = z[2j+1] > z[2j]  (ATen's MaxPool1d: the second member wins only when strictly greater; -0.0 / +0.0 tie)
//     unpool   out[row][2j+sel][c] = v[row][j][c] + bias[c],  the partner exactly +0.0
//     output   recon[n][l] = bias4 + sum_{c,t} u[n][l+1-t][c] w4[c][0][t],  u = unpool(v + bias3, sel1) formed on the fly;
//              dr = 2 (recon - x) / (rows L);  loss = mean (recon - x)^2
//
// float activations (rows, L, C) channels-last.  A pool decision is ONE BIT per pooled element, 32 channels to a uint32:
// word ((row Lo + j) C + c) / 32, bit c % 32.  A thread owns 4 channels of one pooled position, so 8 neighbouring lanes hold one
// word: they build it with three xor-shuffles, and a consumer reads the word once per lane group (one address: a broadcast).
// Neither z nor dz, nor the 64-channel full-resolution map u of the output stage or its gradient, is ever stored.
//
// Every sum runs in an order fixed by the shape alone (thread-private chains, xor-shuffle trees, LDS folds in slot order, chunk
// or block partials folded in index order): no atomics, the same bits every call.  Nothing is allocated or synchronised here.
#include "layer_shared.h"      // Bn4, loss_fold_kernel

#define AE_CG 32                      // channels per block of the pool backward: 8 quads x 32 slots = 256 threads
#define AE_SLOTS 32
#define AE_OUT_C 64                   // channels of the output stage's input (conv_up4: ConvTranspose1d(64, 1))
#define AE_OUT_POS 16                 // pooled positions per block pass of the output stage: 16 quads x 16 positions
#define AE_OUT_BLOCKS 512             // most blocks (= partials) of an output-stage launch
#define AE_OUT_REC 196                // floats per block record of the output backward: dw4 [64][3], db4, padding

// ---- pool forward: thread = 4 channels of one pooled position; idx / 8 is the decision word, 4 (idx % 8) the nibble's shift --
__global__ __launch_bounds__(256) void ae_pool_fwd_kernel(const float* __restrict__ y, int ldy, float* __restrict__ out,
                                                          uint32_t* __restrict__ sel, const uint32_t* __restrict__ sel_in,
                                                          size_t npairs, int Lo, int Lin, int R, int C,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta) {
  const int nq = C >> 2;                                             // (a multiple of 8: the 8 lanes of a word stay together)
  const size_t total = npairs * nq;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    const size_t pr = idx / nq, row = pr / Lo, j = pr - row * Lo;
    Bn4 bn;
    bn.load(mean, invstd, gamma, beta, row / R, C, c0);
    const float* p = y + (row * Lin + 2 * j) * (size_t)ldy + c0;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + ldy);
    const int sh = 4 * (int)(idx & 7);
    f32x4 z0, z1, o;
    uint32_t nib = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      z0[e] = fmaf(a[e], bn.sc[e], bn.sh[e]);
      z1[e] = fmaf(b[e], bn.sc[e], bn.sh[e]);
      nib |= (z1[e] > z0[e] ? 1u : 0u) << e;
    }
    if (sel_in) nib = (sel_in[idx >> 3] >> sh) & 15u;                // teacher forcing: the bits as given
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = ((nib >> e) & 1u) ? z1[e] : z0[e];
    *reinterpret_cast<f32x4*>(out + pr * C + c0) = o;
    if (sel) {
      uint32_t word = nib << sh;
      word |= (uint32_t)__shfl_xor((int)word, 1, 64);
      word |= (uint32_t)__shfl_xor((int)word, 2, 64);
      word |= (uint32_t)__shfl_xor((int)word, 4, 64);
      if ((idx & 7) == 0) sel[idx >> 3] = word;
    }
  }
}

// ---- pool backward, pass 1: block = (window, 32 channels, chunk of pairs); thread = (channel quad, slot) ----------------------
// part[w][chunk][{sum dz, sum dz xhat}][C]
__global__ __launch_bounds__(256) void ae_pool_bwd_partial_kernel(const float* __restrict__ dout, const uint32_t* __restrict__ sel,
                                                                  const float* __restrict__ y, int ldy, float* __restrict__ part,
                                                                  int R, int Lin, int Lo, int C, int chunk,
                                                                  const float* __restrict__ mean, const float* __restrict__ invstd) {
  __shared__ float red[2][AE_SLOTS][AE_CG];
  const int w = blockIdx.x, cg = blockIdx.y, pc = blockIdx.z, P = gridDim.z;
  const int q = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int c0 = cg * AE_CG + q * 4, wpp = C >> 5;                   // (decision words per pooled position)
  const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + (size_t)w * C + c0);
  const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + (size_t)w * C + c0);
  const int npw = R * Lo, p_beg = pc * chunk, p_end = min(npw, p_beg + chunk);
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  for (int pi = p_beg + slot; pi < p_end; pi += AE_SLOTS) {
    const int r = pi / Lo, j = pi - r * Lo;
    const size_t row = (size_t)w * R + r, pr = row * Lo + j;
    const float* p = y + (row * Lin + 2 * j) * (size_t)ldy + c0;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + ldy);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dout + pr * (size_t)C + c0);
    const uint32_t nib = sel[pr * wpp + cg] >> (4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ys = ((nib >> e) & 1u) ? b[e] : a[e];
      s1[e] += d[e];
      s2[e] = fmaf(d[e], (ys - mu[e]) * is[e], s2[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[0][slot][q * 4 + e] = s1[e];
    red[1][slot][q * 4 + e] = s2[e];
  }
  __syncthreads();
  if (threadIdx.x < 2 * AE_CG) {
    const int k = threadIdx.x >> 5, c = threadIdx.x & 31;
    float t = 0.f;
    for (int s = 0; s < AE_SLOTS; ++s) t += red[k][s][c];
    part[(((size_t)w * P + pc) * 2 + k) * C + cg * AE_CG + c] = t;
  }
}

// ---- pool backward, merge: block = (window, 32 channels); thread = (sum, slot of 4, channel): chunks slot, slot + 4, ... in
// order, then the 4 slots in order -> ds[k][w][c]
__global__ __launch_bounds__(256) void ae_pool_bwd_merge_kernel(const float* __restrict__ part, float* __restrict__ ds, int W, int P,
                                                                int C) {
  __shared__ float red[2][4][AE_CG];
  const int w = blockIdx.x, cg = blockIdx.y;
  const int k = threadIdx.x >> 7, slot = (threadIdx.x >> 5) & 3, c = threadIdx.x & 31;
  float t = 0.f;
  for (int p = slot; p < P; p += 4) t += part[(((size_t)w * P + p) * 2 + k) * C + cg * AE_CG + c];
  red[k][slot][c] = t;
  __syncthreads();
  if (slot == 0) ds[((size_t)k * W + w) * C + cg * AE_CG + c] = ((red[k][0][c] + red[k][1][c]) + red[k][2][c]) + red[k][3][c];
}

// ---- pool backward, pass 2: the blocks of pass 1; dy = gamma invstd (dz - sum dz / n - xhat sum dz xhat / n), n = R Lin -------
__global__ __launch_bounds__(256) void ae_pool_bwd_apply_kernel(const float* __restrict__ dout, const uint32_t* __restrict__ sel,
                                                                const float* __restrict__ y, int ldy, float* __restrict__ dy,
                                                                const float* __restrict__ ds, int W, int R, int Lin, int Lo, int C,
                                                                int chunk, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, const float* __restrict__ gamma) {
  const int w = blockIdx.x, cg = blockIdx.y, pc = blockIdx.z;
  const int q = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int c0 = cg * AE_CG + q * 4, wpp = C >> 5;
  const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + (size_t)w * C + c0);
  const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + (size_t)w * C + c0);
  const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c0);
  const f32x4 t1 = *reinterpret_cast<const f32x4*>(ds + (size_t)w * C + c0);
  const f32x4 t2 = *reinterpret_cast<const f32x4*>(ds + ((size_t)W + w) * C + c0);
  const float inv_n = 1.0f / (float)((size_t)R * Lin);
  f32x4 k, m1, m2;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    k[e] = ga[e] * is[e];
    m1[e] = t1[e] * inv_n;
    m2[e] = t2[e] * inv_n;
  }
  const int npw = R * Lo, p_beg = pc * chunk, p_end = min(npw, p_beg + chunk);
  for (int pi = p_beg + slot; pi < p_end; pi += AE_SLOTS) {
    const int r = pi / Lo, j = pi - r * Lo;
    const size_t row = (size_t)w * R + r, pr = row * Lo + j, pos = row * Lin + 2 * j;
    const float* p = y + pos * (size_t)ldy + c0;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + ldy);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dout + pr * (size_t)C + c0);
    const uint32_t nib = sel[pr * wpp + cg] >> (4 * q);
    f32x4 da, db;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool second = ((nib >> e) & 1u) != 0;
      da[e] = k[e] * ((second ? 0.f : d[e]) - m1[e] - (a[e] - mu[e]) * is[e] * m2[e]);
      db[e] = k[e] * ((second ? d[e] : 0.f) - m1[e] - (b[e] - mu[e]) * is[e] * m2[e]);
    }
    *reinterpret_cast<f32x4*>(dy + pos * C + c0) = da;
    *reinterpret_cast<f32x4*>(dy + (pos + 1) * C + c0) = db;
  }
}

// ---- unpool: thread = 4 channels of one pooled position ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ae_unpool_fwd_kernel(const float* __restrict__ v, const float* __restrict__ bias,
                                                            const uint32_t* __restrict__ sel, float* __restrict__ out, size_t npairs,
                                                            int C) {
  const int nq = C >> 2;
  const size_t total = npairs * nq;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    const size_t pr = idx / nq;
    f32x4 a = *reinterpret_cast<const f32x4*>(v + pr * C + c0);
    if (bias) {
      const f32x4 bi = *reinterpret_cast<const f32x4*>(bias + c0);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += bi[e];
    }
    const uint32_t nib = sel[idx >> 3] >> (4 * (int)(idx & 7));
    f32x4 o0, o1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool second = ((nib >> e) & 1u) != 0;
      o0[e] = second ? 0.f : a[e];
      o1[e] = second ? a[e] : 0.f;
    }
    float* o = out + 2 * pr * C + c0;                                // (Lin = 2 Lo: position 2j of the row is pair 2 pr overall)
    *reinterpret_cast<f32x4*>(o) = o0;
    *reinterpret_cast<f32x4*>(o + C) = o1;
  }
}

__global__ __launch_bounds__(256) void ae_unpool_bwd_kernel(const float* __restrict__ dout, const uint32_t* __restrict__ sel,
                                                            float* __restrict__ dv, size_t npairs, int C) {
  const int nq = C >> 2;
  const size_t total = npairs * nq;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % nq) * 4;
    const size_t pr = idx / nq;
    const float* p = dout + 2 * pr * C + c0;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + C);
    const uint32_t nib = sel[idx >> 3] >> (4 * (int)(idx & 7));
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = ((nib >> e) & 1u) ? b[e] : a[e];
    *reinterpret_cast<f32x4*>(dv + pr * C + c0) = o;
  }
}

// ---- the output stage: ConvTranspose1d(64, 1, 3, padding=1) on unpool(v + bias3, sel1), and the MSE against x -----------------
// thread = (pooled position of 16, channel quad of 16); the pooled position pr = row Lo + j owns outputs 2 pr and 2 pr + 1.
// (v + bias3)[pr] of the thread's 4 channels and its decision nibble
__device__ __forceinline__ void ae_out_load(const float* __restrict__ v, const f32x4& b3, const uint32_t* __restrict__ sel1, size_t pr,
                                            int quad, f32x4& a, uint32_t& nib) {
  a = *reinterpret_cast<const f32x4*>(v + pr * AE_OUT_C + quad * 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] += b3[e];
  nib = sel1[pr * 2 + (quad >> 3)] >> (4 * (quad & 7));
}

__global__ __launch_bounds__(256) void ae_out_fwd_kernel(const float* __restrict__ v, const float* __restrict__ bias3,
                                                         const uint32_t* __restrict__ sel1, const float* __restrict__ w4,
                                                         const float* __restrict__ bias4, const float* __restrict__ x,
                                                         float* __restrict__ recon, float* __restrict__ dr,
                                                         float* __restrict__ partials, size_t npos, int Lo, float scale) {
  __shared__ float red[AE_OUT_POS];
  const int quad = threadIdx.x & 15, ps = threadIdx.x >> 4;
  const f32x4 b3 = *reinterpret_cast<const f32x4*>(bias3 + quad * 4);
  float w[4][3];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int t = 0; t < 3; ++t) w[e][t] = w4[(quad * 4 + e) * 3 + t];
  const float b4 = bias4[0];
  float sq = 0.f;
  for (size_t base = (size_t)blockIdx.x * AE_OUT_POS; base < npos; base += (size_t)gridDim.x * AE_OUT_POS) {
    const size_t pr = base + ps;
    const bool valid = pr < npos;
    float r0 = 0.f, r1 = 0.f;
    if (valid) {
      const int j = (int)(pr % Lo);
      f32x4 a, am = {0.f, 0.f, 0.f, 0.f}, ap = {0.f, 0.f, 0.f, 0.f};
      uint32_t nj, nm = 0u, np = 15u;                               // (no left neighbour: nothing second; no right: nothing first)
      ae_out_load(v, b3, sel1, pr, quad, a, nj);
      if (j > 0) ae_out_load(v, b3, sel1, pr - 1, quad, am, nm);
      if (j < Lo - 1) ae_out_load(v, b3, sel1, pr + 1, quad, ap, np);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool s = ((nj >> e) & 1u) != 0;
        const float ue = s ? 0.f : a[e], uo = s ? a[e] : 0.f;        // u[2j], u[2j + 1]
        const float um = ((nm >> e) & 1u) ? am[e] : 0.f;             // u[2j - 1]
        const float up = ((np >> e) & 1u) ? 0.f : ap[e];             // u[2j + 2]
        r0 = fmaf(uo, w[e][0], r0);                                  // recon[l] = sum_t u[l + 1 - t] w[t]
        r0 = fmaf(ue, w[e][1], r0);
        r0 = fmaf(um, w[e][2], r0);
        r1 = fmaf(up, w[e][0], r1);
        r1 = fmaf(uo, w[e][1], r1);
        r1 = fmaf(ue, w[e][2], r1);
      }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {                               // the 16 quads of a position: neighbouring lanes
      r0 += __shfl_xor(r0, o, 64);
      r1 += __shfl_xor(r1, o, 64);
    }
    if (valid && quad == 0) {
      const float x0 = x[2 * pr], x1 = x[2 * pr + 1];
      const float e0 = (r0 + b4) - x0, e1 = (r1 + b4) - x1;
      recon[2 * pr] = r0 + b4;
      recon[2 * pr + 1] = r1 + b4;
      dr[2 * pr] = e0 * scale;
      dr[2 * pr + 1] = e1 * scale;
      sq = fmaf(e0, e0, sq);
      sq = fmaf(e1, e1, sq);
    }
  }
  if (quad == 0) red[ps] = sq;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int s = 0; s < AE_OUT_POS; ++s) t += red[s];
    partials[blockIdx.x] = t;
  }
}

// rec[block][c * 3 + t] = sum over the block's positions of (v + bias3)[c] dr[2j + sel - 1 + t];  rec[block][192] = sum dr
__global__ __launch_bounds__(256) void ae_out_bwd_kernel(const float* __restrict__ drp, const float* __restrict__ v,
                                                         const float* __restrict__ bias3, const uint32_t* __restrict__ sel1,
                                                         const float* __restrict__ w4, float* __restrict__ dv, float* __restrict__ rec,
                                                         size_t npos, int Lo) {
  __shared__ float red[AE_OUT_POS][AE_OUT_C * 3 + 1];
  const int quad = threadIdx.x & 15, ps = threadIdx.x >> 4;
  const f32x4 b3 = *reinterpret_cast<const f32x4*>(bias3 + quad * 4);
  float w[4][3], acc[4][3];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      w[e][t] = w4[(quad * 4 + e) * 3 + t];
      acc[e][t] = 0.f;
    }
  float sdr = 0.f;
  for (size_t base = (size_t)blockIdx.x * AE_OUT_POS; base < npos; base += (size_t)gridDim.x * AE_OUT_POS) {
    const size_t pr = base + ps;
    if (pr >= npos) continue;
    const int j = (int)(pr % Lo);
    f32x4 a;
    uint32_t nib;
    ae_out_load(v, b3, sel1, pr, quad, a, nib);
    float d[4];                                                      // dr[2j - 1 .. 2j + 2], 0 outside the row
    d[0] = j > 0 ? drp[2 * pr - 1] : 0.f;
    d[1] = drp[2 * pr];
    d[2] = drp[2 * pr + 1];
    d[3] = j < Lo - 1 ? drp[2 * pr + 2] : 0.f;
    sdr += d[1] + d[2];
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool s = ((nib >> e) & 1u) != 0;
      const float g0 = s ? d[1] : d[0], g1 = s ? d[2] : d[1], g2 = s ? d[3] : d[2];
      g[e] = fmaf(g2, w[e][2], fmaf(g1, w[e][1], g0 * w[e][0]));
      acc[e][0] = fmaf(a[e], g0, acc[e][0]);
      acc[e][1] = fmaf(a[e], g1, acc[e][1]);
      acc[e][2] = fmaf(a[e], g2, acc[e][2]);
    }
    *reinterpret_cast<f32x4*>(dv + pr * AE_OUT_C + quad * 4) = g;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int t = 0; t < 3; ++t) red[ps][(quad * 4 + e) * 3 + t] = acc[e][t];
  if (quad == 0) red[ps][AE_OUT_C * 3] = sdr;
  __syncthreads();
  if (threadIdx.x < AE_OUT_C * 3 + 1) {
    float t = 0.f;
    for (int s = 0; s < AE_OUT_POS; ++s) t += red[s][threadIdx.x];
    rec[(size_t)blockIdx.x * AE_OUT_REC + threadIdx.x] = t;
  }
}

// block = 8 of the 193 sums x 32 slots: slot s folds records s, s + 32, ... in order, then the 32 slots in order
__global__ __launch_bounds__(256) void ae_out_bwd_merge_kernel(const float* __restrict__ rec, int nrec, float* __restrict__ dw4,
                                                               float* __restrict__ db4, int accumulate) {
  __shared__ float red[32][8];
  const int o = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int i = blockIdx.x * 8 + o;
  float t = 0.f;
  if (i <= AE_OUT_C * 3)
    for (int r = slot; r < nrec; r += 32) t += rec[(size_t)r * AE_OUT_REC + i];
  red[slot][o] = t;
  __syncthreads();
  if (slot == 0 && i <= AE_OUT_C * 3) {
    float s = 0.f;
    for (int k = 0; k < 32; ++k) s += red[k][o];
    float* dst = i < AE_OUT_C * 3 ? dw4 + i : db4;
    *dst = accumulate ? *dst + s : s;
  }
}

extern "C" {

static bool ae_pool_shape_ok(int rows, int R, int Lin, int C, int ldy) {
  return rows >= 0 && R >= 1 && rows % R == 0 && Lin >= 2 && Lin % 2 == 0 && C >= 32 && C % 32 == 0 && C / AE_CG <= 65535 && ldy >= C &&
         ldy % 4 == 0 && fits32((size_t)rows, (size_t)Lin, (size_t)ldy);
}

// Chunk geometry of da_bn_maxpool2_idx_bwd, without launching: the R (Lin / 2) pooled positions of a window are cut into
// `chunks` runs of `chunk_pairs` (the last one shorter) so that windows x channel groups x chunks fills the chip; chunk p holds
// the window's pairs [p chunk_pairs, min((p + 1) chunk_pairs, R Lin / 2)).  workspace: bytes of the chunk partials.
int da_bn_maxpool2_idx_plan(int rows, int R, int Lin, int C, int* chunks, int* chunk_pairs, size_t* workspace) {
  if (!chunks || !chunk_pairs || !workspace || rows < 1 || !ae_pool_shape_ok(rows, R, Lin, C, C) ||
      (size_t)R * Lin >= 0x7fffffffull)
    return DA_EINVAL;
  const long W = rows / R, npw = (long)R * (Lin / 2), base = W * (C / AE_CG);
  long p = (1024 + base - 1) / base;
  const long maxp = (npw + 127) / 128;                               // at least 128 pairs (4 per slot) per chunk
  if (p > maxp) p = maxp;
  if (p < 1) p = 1;
  const long ch = ((npw + p - 1) / p + 31) / 32 * 32;
  const long P = (npw + ch - 1) / ch;
  if (P > 65535 || W > 0x7fffffffl) return DA_EINVAL;
  *chunks = (int)P;
  *chunk_pairs = (int)ch;
  *workspace = (size_t)W * P * 2 * (size_t)C * sizeof(float);
  return DA_OK;
}

size_t da_bn_maxpool2_idx_bwd_workspace(int rows, int R, int Lin, int C) {
  int P, ch;
  size_t ws;
  return da_bn_maxpool2_idx_plan(rows, R, Lin, C, &P, &ch, &ws) == DA_OK ? ws : 0;
}

// y [rows][Lin][ldy], statistics (W, C) -> out [rows][Lin / 2][C], sel: rows (Lin / 2) C / 32 words.  sel_in NULL: decide and
// write sel; else take sel_in's bits (sel NULL, or a destination for a copy)
int da_bn_maxpool2_idx_fwd(const float* y, int ldy, float* out, uint32_t* sel, const uint32_t* sel_in, int rows, int R, int Lin,
                           int C, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!y || !out || (!sel && !sel_in) || !mean || !invstd || !gamma || !beta || !ae_pool_shape_ok(rows, R, Lin, C, ldy))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  const int Lo = Lin / 2;
  const size_t npairs = (size_t)rows * Lo;
  hipLaunchKernelGGL(ae_pool_fwd_kernel, dim3(grid_stride_blocks(npairs * (C / 4))), dim3(256), 0, stream, y, ldy, out, sel, sel_in, npairs, Lo,
                     Lin, R, C, mean, invstd, gamma, beta);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// dout [rows][Lin / 2][C], sel, y [rows][Lin][ldy] -> dy [rows][Lin][C], ds [2][W][C] (sum dz, sum dz xhat: da_bn_param_grad_multi)
int da_bn_maxpool2_idx_bwd(const float* dout, const uint32_t* sel, const float* y, int ldy, float* dy, float* ds, float* workspace,
                           int rows, int R, int Lin, int C, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!dout || !sel || !y || !dy || !ds || !workspace || !mean || !invstd || !gamma || !beta || !ae_pool_shape_ok(rows, R, Lin, C, ldy))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  int P, chunk;
  size_t ws;
  if (da_bn_maxpool2_idx_plan(rows, R, Lin, C, &P, &chunk, &ws) != DA_OK) return DA_EINVAL;
  const int W = rows / R, Lo = Lin / 2;
  const dim3 grid(W, C / AE_CG, P);
  hipLaunchKernelGGL(ae_pool_bwd_partial_kernel, grid, dim3(256), 0, stream, dout, sel, y, ldy, workspace, R, Lin, Lo, C, chunk, mean,
                     invstd);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(ae_pool_bwd_merge_kernel, dim3(W, C / AE_CG), dim3(256), 0, stream, workspace, ds, W, P, C);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(ae_pool_bwd_apply_kernel, grid, dim3(256), 0, stream, dout, sel, y, ldy, dy, ds, W, R, Lin, Lo, C, chunk, mean,
                     invstd, gamma);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

static bool ae_unpool_shape_ok(int rows, int Lo, int C) {
  return rows >= 0 && Lo >= 1 && C >= 32 && C % 32 == 0 && fits32((size_t)rows, 2 * (size_t)Lo, (size_t)C);
}

// v [rows][Lo][C] (+ bias[C], or NULL) -> out [rows][2 Lo][C]: every element written
int da_unpool2_fwd(const float* v, const float* bias, const uint32_t* sel, float* out, int rows, int Lo, int C, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!v || !sel || !out || !ae_unpool_shape_ok(rows, Lo, C)) return DA_EINVAL;
  if (rows == 0) return DA_OK;
  const size_t npairs = (size_t)rows * Lo;
  hipLaunchKernelGGL(ae_unpool_fwd_kernel, dim3(grid_stride_blocks(npairs * (C / 4))), dim3(256), 0, stream, v, bias, sel, out, npairs, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// dout [rows][2 Lo][C] -> dv [rows][Lo][C] = dout[2j + sel]
int da_unpool2_bwd(const float* dout, const uint32_t* sel, float* dv, int rows, int Lo, int C, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!dout || !sel || !dv || !ae_unpool_shape_ok(rows, Lo, C)) return DA_EINVAL;
  if (rows == 0) return DA_OK;
  const size_t npairs = (size_t)rows * Lo;
  hipLaunchKernelGGL(ae_unpool_bwd_kernel, dim3(grid_stride_blocks(npairs * (C / 4))), dim3(256), 0, stream, dout, sel, dv, npairs, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

static bool ae_out_shape_ok(int rows, int L) {
  return rows >= 0 && L >= 2 && L % 2 == 0 && (size_t)rows * (size_t)L * (AE_OUT_C / 2) < 0x80000000ull;
}

static int ae_out_blocks(int rows, int L) {
  const size_t b = ((size_t)rows * (L / 2) + AE_OUT_POS - 1) / AE_OUT_POS;
  return (int)(b < AE_OUT_BLOCKS ? b : AE_OUT_BLOCKS);
}

// bytes of the loss partials of da_ae_out_fwd / of the block records of da_ae_out_bwd
size_t da_ae_out_fwd_workspace(int rows, int L) {
  return ae_out_shape_ok(rows, L) ? (size_t)ae_out_blocks(rows, L) * sizeof(float) : 0;
}
size_t da_ae_out_bwd_workspace(int rows, int L) {
  return ae_out_shape_ok(rows, L) ? (size_t)ae_out_blocks(rows, L) * AE_OUT_REC * sizeof(float) : 0;
}

// v [rows][L / 2][64], x [rows][L] -> recon, dr [rows][L], loss[1]
int da_ae_out_fwd(const float* v, const float* bias3, const uint32_t* sel1, const float* w4, const float* bias4, const float* x,
                  float* recon, float* dr, float* partials, float* loss, int rows, int L, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!v || !bias3 || !sel1 || !w4 || !bias4 || !x || !recon || !dr || !partials || !loss || !ae_out_shape_ok(rows, L) || rows < 1)
    return DA_EINVAL;
  const size_t npos = (size_t)rows * (L / 2);
  const int blocks = ae_out_blocks(rows, L);
  const float n = (float)rows * (float)L;
  hipLaunchKernelGGL(ae_out_fwd_kernel, dim3(blocks), dim3(256), 0, stream, v, bias3, sel1, w4, bias4, x, recon, dr, partials, npos,
                     L / 2, 2.0f / n);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_fold_kernel, dim3(1), dim3(256), 0, stream, partials, blocks, 1.0f / n, loss);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// dr [rows][L], v [rows][L / 2][64] -> dv [rows][L / 2][64] (the gradient at v + bias3), dw4 [64][1][3] and db4 [1] (+)=
int da_ae_out_bwd(const float* dr, const float* v, const float* bias3, const uint32_t* sel1, const float* w4, float* dv, float* dw4,
                  float* db4, float* workspace, int rows, int L, int accumulate, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!dr || !v || !bias3 || !sel1 || !w4 || !dv || !dw4 || !db4 || !workspace || !ae_out_shape_ok(rows, L) || rows < 1) return DA_EINVAL;
  const size_t npos = (size_t)rows * (L / 2);
  const int blocks = ae_out_blocks(rows, L);
  hipLaunchKernelGGL(ae_out_bwd_kernel, dim3(blocks), dim3(256), 0, stream, dr, v, bias3, sel1, w4, dv, workspace, npos, L / 2);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(ae_out_bwd_merge_kernel, dim3((AE_OUT_C * 3 + 1 + 7) / 8), dim3(256), 0, stream, workspace, blocks, dw4, db4,
                     accumulate ? 1 : 0);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
