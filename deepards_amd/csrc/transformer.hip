// One Block of the cnn_transformer head (reference models/transformer.py:13-88) as three fused fp32 kernels:
//
//   tfm_fwd_kernel     one workgroup per window: q/k/v projections, 4-head softmax attention, joint projection, dropout +
//                      residual + LayerNorm, feed-forward, dropout + residual (the block INPUT, :88) + LayerNorm.
//   tfm_bwd_kernel     one workgroup per window: dy -> dx and the per-token gradients the parameter pass reads.
//   tfm_pgrad_kernel   grid (D / 32 column slices, H / 8 row chunks): every workgroup walks all B T tokens in a fixed order
//                      and writes its slice of the sixteen parameter gradients (no atomics, no per-window slabs).
//
// Token rows live in LDS one wave at a time: a wave owns TPW tokens per pass, a lane the columns lane, lane + 64, ... of
// each; a whole (T, D) tile at the largest supported shape (64 x 2048 floats = 512 KB) does not fit the 160 KB LDS, so the
// tile is staged row-wise by the wave that works on the row.  Sums over D are lane partials in column order then one
// butterfly, sums over H and over tokens run in index order: nothing depends on timing, a replay is bit-identical.
// `attended` (the first LayerNorm's output) is not stored: it is rebuilt from the saved attention weights and v, a
// contraction over H <= 64, wherever the backward needs it.
#include "common.h"
#include <string.h>

#define TFM_NW 4                       // waves per workgroup (forward and data backward)
#define TFM_EPS 1e-5f                  // nn.LayerNorm default

struct TfmParams {                     // named_parameters() order of one Block
  const float *wq, *bq, *wk, *bk, *wv, *bv, *wj, *bj, *g1, *be1, *w0, *b0, *w2, *b2, *g2, *be2;
};
struct TfmGrads {
  float *wq, *bq, *wk, *bk, *wv, *bv, *wj, *bj, *g1, *be1, *w0, *b0, *w2, *b2, *g2, *be2;
};

struct TfmDrop {                       // the two dropout sites of a block: keys and threshold of da_dropout's mask
  uint32_t key1, key2, thr;
  float scale;
  __device__ __forceinline__ void init(const int64_t* seed_ptr, uint32_t salt1, uint32_t salt2, float p) {
    const int64_t s64 = seed_ptr ? seed_ptr[0] : 0;
    const uint32_t seed = (uint32_t)s64 ^ (uint32_t)(s64 >> 32);
    key1 = mix32(seed, salt1);
    key2 = mix32(seed, salt2);
    thr = (uint32_t)(p * 4294967296.0);
    scale = 1.0f / (1.0f - p);
  }
  __device__ __forceinline__ bool keep(uint32_t key, size_t i) const {
    return mix32(key, (uint32_t)i ^ (uint32_t)(i >> 32) * 0x27d4eb2fu) >= thr;
  }
  __device__ __forceinline__ float apply(uint32_t key, size_t i, float v) const { return keep(key, i) ? v * scale : 0.f; }
};

// acc[k][i] = sum_d rows[k * rstride + d] * W[(h0 + i) * D + d], i < 8 (weights [H][D]); every lane gets the sums
template <int TPW>
__device__ __forceinline__ void dot_d_hd(const float* __restrict__ W, int D, int h0, const float* rows, int rstride, int lane,
                                         float (&acc)[TPW][8]) {
#pragma unroll
  for (int k = 0; k < TPW; ++k)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[k][i] = 0.f;
  for (int d = lane; d < D; d += 64) {
    float xv[TPW];
#pragma unroll
    for (int k = 0; k < TPW; ++k) xv[k] = rows[k * rstride + d];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float w = W[(size_t)(h0 + i) * D + d];
#pragma unroll
      for (int k = 0; k < TPW; ++k) acc[k][i] = fmaf(xv[k], w, acc[k][i]);
    }
  }
#pragma unroll
  for (int k = 0; k < TPW; ++k)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[k][i] = wave_sum(acc[k][i]);
}

// the same with weights [D][H]: acc[k][i] = sum_d rows[k * rstride + d] * W[d * H + h0 + i]
template <int TPW>
__device__ __forceinline__ void dot_d_dh(const float* __restrict__ W, int D, int H, int h0, const float* rows, int rstride,
                                         int lane, float (&acc)[TPW][8]) {
#pragma unroll
  for (int k = 0; k < TPW; ++k)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[k][i] = 0.f;
  for (int d = lane; d < D; d += 64) {
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(W + (size_t)d * H + h0);
    const f32x4 w1 = *reinterpret_cast<const f32x4*>(W + (size_t)d * H + h0 + 4);
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      const float xv = rows[k * rstride + d];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[k][i] = fmaf(xv, w0[i], acc[k][i]);
        acc[k][i + 4] = fmaf(xv, w1[i], acc[k][i + 4]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < TPW; ++k)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[k][i] = wave_sum(acc[k][i]);
}

// bias + sum_h vec[h] * Wrow[h]: one output column of a Linear(H, D) (weights [D][H], Wrow = W + d * H), h in index order
__device__ __forceinline__ float dot_h_row(const float* __restrict__ Wrow, const float* vec, int H, float bias) {
  float s = bias;
  for (int h = 0; h < H; h += 4) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(Wrow + h);
    const f32x4 u = *reinterpret_cast<const f32x4*>(vec + h);
#pragma unroll
    for (int e = 0; e < 4; ++e) s = fmaf(u[e], w[e], s);
  }
  return s;
}

// sum_h vec[h] * W[h * D + d] (weights [H][D]), h in index order
__device__ __forceinline__ float dot_h_col(const float* __restrict__ W, int D, int d, const float* vec, int H, float s) {
  for (int h = 0; h < H; ++h) s = fmaf(vec[h], W[(size_t)h * D + d], s);
  return s;
}

// mean and 1 / sqrt(biased variance + eps) of one LDS row (two passes: the variance is taken around the mean)
__device__ __forceinline__ void row_stats(const float* row, int D, int lane, float& mean, float& rstd) {
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += row[d];
  mean = wave_sum(s) / (float)D;
  float v = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float t = row[d] - mean;
    v = fmaf(t, t, v);
  }
  rstd = 1.0f / sqrtf(wave_sum(v) / (float)D + TFM_EPS);
}

struct TfmFwdArgs {
  const float* x;
  TfmParams p;
  float *y, *q, *k, *v, *aw, *hid, *stats;
  int T, D, H;
  const int64_t* seed;
  uint32_t salt1, salt2;
  float drop_p;
};

// LDS floats: q | k | v [T][H] (q becomes the re-joined heads, k the ff hidden) | rows [TFM_NW][TPW][D]
template <int TPW>
__global__ __launch_bounds__(256) void tfm_fwd_kernel(TfmFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int T = a.T, D = a.D, H = a.H;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  float* sq = sm;
  float* sk = sq + T * H;
  float* sv = sk + T * H;
  float* rows = sv + T * H + (size_t)wave * TPW * D;
  const TfmParams& P = a.p;
  TfmDrop dr;
  dr.init(a.seed, a.salt1, a.salt2, a.drop_p);
  const int npass = ((T + TFM_NW - 1) / TFM_NW + TPW - 1) / TPW;
  const size_t tok0 = (size_t)b * T;

  // ---- q, k, v = x W^T + b
  for (int g = 0; g < npass; ++g) {
    int tok[TPW], tc[TPW];
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      tok[k] = wave + TFM_NW * (g * TPW + k);
      tc[k] = min(tok[k], T - 1);
      for (int d = lane; d < D; d += 64) rows[k * D + d] = a.x[(tok0 + tc[k]) * D + d];
    }
#pragma unroll 1
    for (int m = 0; m < 3; ++m) {
      const float* W = m == 0 ? P.wq : m == 1 ? P.wk : P.wv;
      const float* bias = m == 0 ? P.bq : m == 1 ? P.bk : P.bv;
      float* sdst = m == 0 ? sq : m == 1 ? sk : sv;
      float* gdst = m == 0 ? a.q : m == 1 ? a.k : a.v;
      for (int h0 = 0; h0 < H; h0 += 8) {
        float acc[TPW][8];
        dot_d_hd<TPW>(W, D, h0, rows, D, lane, acc);
#pragma unroll
        for (int k = 0; k < TPW; ++k)
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (lane == i && tok[k] < T) {
              const float val = acc[k][i] + bias[h0 + i];
              sdst[tok[k] * H + h0 + i] = val;
              gdst[(tok0 + tok[k]) * H + h0 + i] = val;
            }
      }
    }
  }
  __syncthreads();

  // ---- attention: thread (head, query i); softmax over the keys with the row maximum subtracted (transformer.py:42-47)
  if (tid < 4 * T) {
    const int head = tid / T, i = tid - head * T, hs = H >> 2;
    const float den = sqrtf((float)hs);
    float qv[16], acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      qv[e] = e < hs ? sq[i * H + head * hs + e] : 0.f;
      acc[e] = 0.f;
    }
    float mx = -INFINITY;
    for (int j = 0; j < T; ++j) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < hs) s = fmaf(qv[e], sk[j * H + head * hs + e], s);
      mx = fmaxf(mx, s / den);
    }
    float sum = 0.f;
    for (int j = 0; j < T; ++j) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < hs) s = fmaf(qv[e], sk[j * H + head * hs + e], s);
      sum += expf(s / den - mx);
    }
    float* awr = a.aw + (((size_t)b * 4 + head) * T + i) * T;
    for (int j = 0; j < T; ++j) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < hs) s = fmaf(qv[e], sk[j * H + head * hs + e], s);
      const float w = expf(s / den - mx) / sum;
      awr[j] = w;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < hs) acc[e] = fmaf(w, sv[j * H + head * hs + e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e < hs) sq[i * H + head * hs + e] = acc[e];          // only this thread read these q entries
  }
  __syncthreads();

  // ---- joint projection, dropout + x, LayerNorm, feed-forward, dropout + x, LayerNorm
  float* shid = sk;
  for (int g = 0; g < npass; ++g) {
    int tok[TPW], tc[TPW];
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      tok[k] = wave + TFM_NW * (g * TPW + k);
      tc[k] = min(tok[k], T - 1);
    }
    for (int d = lane; d < D; d += 64) {
      const float* wr = P.wj + (size_t)d * H;
      const float bias = P.bj[d];
#pragma unroll
      for (int k = 0; k < TPW; ++k) {
        const size_t idx = (tok0 + tc[k]) * D + d;
        rows[k * D + d] = dr.apply(dr.key1, idx, dot_h_row(wr, sq + tc[k] * H, H, bias)) + a.x[idx];
      }
    }
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      float mean, rstd;
      row_stats(rows + k * D, D, lane, mean, rstd);
      if (lane == 0 && tok[k] < T) {
        a.stats[(tok0 + tok[k]) * 4 + 0] = mean;
        a.stats[(tok0 + tok[k]) * 4 + 1] = rstd;
      }
      for (int d = lane; d < D; d += 64) rows[k * D + d] = fmaf((rows[k * D + d] - mean) * rstd, P.g1[d], P.be1[d]);
    }
    for (int h0 = 0; h0 < H; h0 += 8) {
      float acc[TPW][8];
      dot_d_hd<TPW>(P.w0, D, h0, rows, D, lane, acc);
#pragma unroll
      for (int k = 0; k < TPW; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (lane == i && tok[k] < T) {
            const float val = fmaxf(acc[k][i] + P.b0[h0 + i], 0.f);
            shid[tok[k] * H + h0 + i] = val;
            a.hid[(tok0 + tok[k]) * H + h0 + i] = val;
          }
    }
    __syncthreads();                                            // (npass is the same for every wave)
    for (int d = lane; d < D; d += 64) {
      const float* wr = P.w2 + (size_t)d * H;
      const float bias = P.b2[d];
#pragma unroll
      for (int k = 0; k < TPW; ++k) {
        const size_t idx = (tok0 + tc[k]) * D + d;
        rows[k * D + d] = dr.apply(dr.key2, idx, dot_h_row(wr, shid + tc[k] * H, H, bias)) + a.x[idx];
      }
    }
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      float mean, rstd;
      row_stats(rows + k * D, D, lane, mean, rstd);
      if (tok[k] < T) {
        if (lane == 0) {
          a.stats[(tok0 + tok[k]) * 4 + 2] = mean;
          a.stats[(tok0 + tok[k]) * 4 + 3] = rstd;
        }
        for (int d = lane; d < D; d += 64)
          a.y[(tok0 + tok[k]) * D + d] = fmaf((rows[k * D + d] - mean) * rstd, P.g2[d], P.be2[d]);
      }
    }
  }
}

struct TfmBwdArgs {
  const float *dy, *x;
  TfmParams p;
  const float *q, *k, *v, *aw, *hid, *stats;
  float *dx, *dq, *dk, *dv, *dhid, *da1, *da2, *wv;
  int T, D, H;
  const int64_t* seed;
  uint32_t salt1, salt2;
  float drop_p;
};

// LDS floats: q | k | v | wv | dp [T][H] (dp: d(ff pre-activation), later d(re-joined heads)) | dot [4][T] |
// rows [TFM_NW][TPW][2][D]
template <int TPW>
__global__ __launch_bounds__(256) void tfm_bwd_kernel(TfmBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int T = a.T, D = a.D, H = a.H, TH = T * H;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.x;
  float* sq = sm;
  float* sk = sq + TH;
  float* sv = sk + TH;
  float* swv = sv + TH;
  float* sdp = swv + TH;
  float* sdot = sdp + TH;
  float* rows = sdot + 4 * T + (size_t)wave * TPW * 2 * D;      // token k: row A at k * 2 D, row B at k * 2 D + D
  const TfmParams& P = a.p;
  TfmDrop dr;
  dr.init(a.seed, a.salt1, a.salt2, a.drop_p);
  const int npass = ((T + TFM_NW - 1) / TFM_NW + TPW - 1) / TPW;
  const size_t tok0 = (size_t)b * T;
  const int hs = H >> 2;
  const float den = sqrtf((float)hs);

  for (int i = tid; i < TH; i += 256) {
    sq[i] = a.q[tok0 * H + i];
    sk[i] = a.k[tok0 * H + i];
    sv[i] = a.v[tok0 * H + i];
  }
  __syncthreads();
  // ---- the re-joined heads wv = weights v (the forward did not keep them)
  if (tid < 4 * T) {
    const int head = tid / T, i = tid - head * T;
    const float* awr = a.aw + (((size_t)b * 4 + head) * T + i) * T;
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (int j = 0; j < T; ++j) {
      const float w = awr[j];
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < hs) acc[e] = fmaf(w, sv[j * H + head * hs + e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e < hs) {
        swv[i * H + head * hs + e] = acc[e];
        a.wv[(tok0 + i) * H + head * hs + e] = acc[e];
      }
  }
  __syncthreads();

  for (int g = 0; g < npass; ++g) {
    int tok[TPW], tc[TPW];
    float m1[TPW], r1[TPW], m2[TPW], r2[TPW];
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      tok[k] = wave + TFM_NW * (g * TPW + k);
      tc[k] = min(tok[k], T - 1);
      const float* st = a.stats + (tok0 + tc[k]) * 4;
      m1[k] = st[0]; r1[k] = st[1]; m2[k] = st[2]; r2[k] = st[3];
    }
    // second LayerNorm: rebuild its input from the ff hidden, then d(input)
    float s1[TPW], s2[TPW];
#pragma unroll
    for (int k = 0; k < TPW; ++k) s1[k] = s2[k] = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float* wr = P.w2 + (size_t)d * H;
      const float bias = P.b2[d], gam = P.g2[d];
#pragma unroll
      for (int k = 0; k < TPW; ++k) {
        const size_t idx = (tok0 + tc[k]) * D + d;
        const float a2 = dr.apply(dr.key2, idx, dot_h_row(wr, a.hid + (tok0 + tc[k]) * H, H, bias)) + a.x[idx];
        const float xh = (a2 - m2[k]) * r2[k], gg = a.dy[idx] * gam;
        s1[k] += gg;
        s2[k] = fmaf(gg, xh, s2[k]);
        rows[k * 2 * D + d] = xh;
        rows[k * 2 * D + D + d] = gg;
      }
    }
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      s1[k] = wave_sum(s1[k]) / (float)D;
      s2[k] = wave_sum(s2[k]) / (float)D;
    }
    for (int d = lane; d < D; d += 64)
#pragma unroll
      for (int k = 0; k < TPW; ++k) {
        const size_t idx = (tok0 + tc[k]) * D + d;
        const float da = r2[k] * (rows[k * 2 * D + D + d] - s1[k] - rows[k * 2 * D + d] * s2[k]);
        if (tok[k] < T) a.da2[idx] = da;
        rows[k * 2 * D + D + d] = dr.apply(dr.key2, idx, da);       // d(ff output)
      }
    for (int h0 = 0; h0 < H; h0 += 8) {
      float acc[TPW][8];
      dot_d_dh<TPW>(P.w2, D, H, h0, rows + D, 2 * D, lane, acc);
#pragma unroll
      for (int k = 0; k < TPW; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (lane == i && tok[k] < T) {
            const float val = a.hid[(tok0 + tok[k]) * H + h0 + i] > 0.f ? acc[k][i] : 0.f;
            sdp[tok[k] * H + h0 + i] = val;
            a.dhid[(tok0 + tok[k]) * H + h0 + i] = val;
          }
    }
    __syncthreads();                                            // (npass is the same for every wave)
    // first LayerNorm: its output feeds ff.0 only (the second residual adds the block input)
#pragma unroll
    for (int k = 0; k < TPW; ++k) s1[k] = s2[k] = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float* wr = P.wj + (size_t)d * H;
      const float bias = P.bj[d], gam = P.g1[d];
#pragma unroll
      for (int k = 0; k < TPW; ++k) {
        const size_t idx = (tok0 + tc[k]) * D + d;
        const float a1 = dr.apply(dr.key1, idx, dot_h_row(wr, swv + tc[k] * H, H, bias)) + a.x[idx];
        const float xh = (a1 - m1[k]) * r1[k];
        const float gg = dot_h_col(P.w0, D, d, sdp + tc[k] * H, H, 0.f) * gam;
        s1[k] += gg;
        s2[k] = fmaf(gg, xh, s2[k]);
        rows[k * 2 * D + d] = xh;
        rows[k * 2 * D + D + d] = gg;
      }
    }
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      s1[k] = wave_sum(s1[k]) / (float)D;
      s2[k] = wave_sum(s2[k]) / (float)D;
    }
    for (int d = lane; d < D; d += 64)
#pragma unroll
      for (int k = 0; k < TPW; ++k) {
        const size_t idx = (tok0 + tc[k]) * D + d;
        const float da = r1[k] * (rows[k * 2 * D + D + d] - s1[k] - rows[k * 2 * D + d] * s2[k]);
        if (tok[k] < T) a.da1[idx] = da;
        rows[k * 2 * D + D + d] = dr.apply(dr.key1, idx, da);       // d(joint projection output)
      }
    __syncthreads();                                            // every lane is done with this pass's sdp rows
    for (int h0 = 0; h0 < H; h0 += 8) {
      float acc[TPW][8];
      dot_d_dh<TPW>(P.wj, D, H, h0, rows + D, 2 * D, lane, acc);
#pragma unroll
      for (int k = 0; k < TPW; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (lane == i && tok[k] < T) sdp[tok[k] * H + h0 + i] = acc[k][i];         // d(re-joined heads)
    }
  }
  __syncthreads();

  // ---- attention backward.  As query i: dot_i = sum_j w_ij (dwv_i . v_j), dq_i = sum_j ds_ij k_j / sqrt(hs)
  const int head = tid < 4 * T ? tid / T : 0, qi = tid - head * T;
  if (tid < 4 * T) {
    const float* awr = a.aw + (((size_t)b * 4 + head) * T + qi) * T;
    float dw[16], acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      dw[e] = e < hs ? sdp[qi * H + head * hs + e] : 0.f;
      acc[e] = 0.f;
    }
    float dot = 0.f;
    for (int j = 0; j < T; ++j) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < hs) s = fmaf(dw[e], sv[j * H + head * hs + e], s);
      dot = fmaf(awr[j], s, dot);
    }
    sdot[head * T + qi] = dot;
    for (int j = 0; j < T; ++j) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < hs) s = fmaf(dw[e], sv[j * H + head * hs + e], s);
      const float ds = awr[j] * (s - dot);
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < hs) acc[e] = fmaf(ds, sk[j * H + head * hs + e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e < hs) a.dq[(tok0 + qi) * H + head * hs + e] = acc[e] / den;
  }
  __syncthreads();
  // as key j (= qi): dv_j = sum_t w_tj dwv_t, dk_j = sum_t ds_tj q_t / sqrt(hs)
  if (tid < 4 * T) {
    const float* awc = a.aw + ((size_t)b * 4 + head) * T * T + qi;
    float vv[16], ak[16], av[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      vv[e] = e < hs ? sv[qi * H + head * hs + e] : 0.f;
      ak[e] = av[e] = 0.f;
    }
    for (int t = 0; t < T; ++t) {
      const float w = awc[(size_t)t * T];
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < hs) s = fmaf(sdp[t * H + head * hs + e], vv[e], s);
      const float ds = w * (s - sdot[head * T + t]);
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < hs) {
          ak[e] = fmaf(ds, sq[t * H + head * hs + e], ak[e]);
          av[e] = fmaf(w, sdp[t * H + head * hs + e], av[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e < hs) {
        a.dk[(tok0 + qi) * H + head * hs + e] = ak[e] / den;
        a.dv[(tok0 + qi) * H + head * hs + e] = av[e];
      }
  }
  __syncthreads();                     // dq / dk / dv of the window are in memory for the whole workgroup

  // ---- dx = d(LayerNorm inputs) (both residuals add x) + the three projections' input gradients
  for (int g = 0; g < npass; ++g)
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
      const int t = wave + TFM_NW * (g * TPW + k);
      if (t >= T) continue;
      const float* gq = a.dq + (tok0 + t) * H;
      const float* gk = a.dk + (tok0 + t) * H;
      const float* gv = a.dv + (tok0 + t) * H;
      for (int d = lane; d < D; d += 64) {
        const size_t idx = (tok0 + t) * D + d;
        float s = a.da1[idx] + a.da2[idx];                      // this lane wrote both
        s = dot_h_col(P.wq, D, d, gq, H, s);
        s = dot_h_col(P.wk, D, d, gk, H, s);
        s = dot_h_col(P.wv, D, d, gv, H, s);
        a.dx[idx] = s;
      }
    }
}

struct TfmPgradArgs {
  const float *dy, *x;
  TfmParams p;
  const float *hid, *stats, *wv, *dq, *dk, *dv, *dhid, *da1, *da2;
  TfmGrads g;
  int accumulate, NT, D, H;            // NT = B T tokens
  const int64_t* seed;
  uint32_t salt1, salt2;
  float drop_p;
};

// the eight token slots' partial sums of eight accumulators -> thread (slot s, column c) gets the total of accumulator s
__device__ __forceinline__ float pgrad_fold(const float (&acc)[8], float (*red)[8][32], int slot, int c) {
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) red[slot][i][c] = acc[i];
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += red[k][slot][c];
  return s;
}

__device__ __forceinline__ void pgrad_store(float* p, float v, int accumulate) { *p = accumulate ? *p + v : v; }

// block (bx, hc): columns [32 bx, 32 bx + 32) of D, rows [8 hc, 8 hc + 8) of H.  Thread = (token slot, column): slot s
// walks the tokens s, s + 8, ...; the slots are folded in slot order.  The D-long vectors (LayerNorm, joint / ff.2 bias)
// come from the hc == 0 blocks, the H-long biases from the bx == 0 blocks.
__global__ __launch_bounds__(256) void tfm_pgrad_kernel(TfmPgradArgs a) {
  __shared__ float swj[64][32], sw2[64][32], sw0[64][32];
  __shared__ float red[8][8][32];
  const int D = a.D, H = a.H;
  const int tid = threadIdx.x, c = tid & 31, slot = tid >> 5;
  const int d = blockIdx.x * 32 + c, hc = blockIdx.y, hb = hc * 8;
  const TfmParams& P = a.p;
  TfmDrop dr;
  dr.init(a.seed, a.salt1, a.salt2, a.drop_p);
  for (int i = tid; i < H * 32; i += 256) {
    const int h = i >> 5, cc = i & 31, dd = blockIdx.x * 32 + cc;
    swj[h][cc] = P.wj[(size_t)dd * H + h];
    sw2[h][cc] = P.w2[(size_t)dd * H + h];
    sw0[h][cc] = P.w0[(size_t)h * D + dd];
  }
  __syncthreads();
  const bool vecs = hc == 0, hbias = blockIdx.x == 0;
  const float bj = P.bj[d], b2 = P.b2[d], g1 = P.g1[d], be1 = P.be1[d];
  float aq[8], ak[8], av[8], a0[8], aj[8], a2[8], vec[8], hq[8], hk[8], hv[8], h0[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) aq[i] = ak[i] = av[i] = a0[i] = aj[i] = a2[i] = vec[i] = hq[i] = hk[i] = hv[i] = h0[i] = 0.f;

  for (int n = slot; n < a.NT; n += 8) {
    const size_t idx = (size_t)n * D + d;
    const float* hidr = a.hid + (size_t)n * H;
    const float* wvr = a.wv + (size_t)n * H;
    const float* dhr = a.dhid + (size_t)n * H;
    const float* dqr = a.dq + (size_t)n * H + hb;
    const float* dkr = a.dk + (size_t)n * H + hb;
    const float* dvr = a.dv + (size_t)n * H + hb;
    const float* st = a.stats + (size_t)n * 4;
    const float xv = a.x[idx];
    float J = bj;
    for (int h = 0; h < H; ++h) J = fmaf(wvr[h], swj[h][c], J);
    const bool k1 = dr.keep(dr.key1, idx), k2 = dr.keep(dr.key2, idx);
    const float xh1 = ((k1 ? J * dr.scale : 0.f) + xv - st[0]) * st[1];
    const float att = fmaf(xh1, g1, be1);
    const float dJ = k1 ? a.da1[idx] * dr.scale : 0.f;
    const float dF = k2 ? a.da2[idx] * dr.scale : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      aq[i] = fmaf(dqr[i], xv, aq[i]);
      ak[i] = fmaf(dkr[i], xv, ak[i]);
      av[i] = fmaf(dvr[i], xv, av[i]);
      a0[i] = fmaf(dhr[hb + i], att, a0[i]);
      aj[i] = fmaf(dJ, wvr[hb + i], aj[i]);
      a2[i] = fmaf(dF, hidr[hb + i], a2[i]);
    }
    if (vecs) {                                                  // (block-uniform)
      float F = b2, dAtt = 0.f;
      for (int h = 0; h < H; ++h) {
        F = fmaf(hidr[h], sw2[h][c], F);
        dAtt = fmaf(dhr[h], sw0[h][c], dAtt);
      }
      const float xh2 = ((k2 ? F * dr.scale : 0.f) + xv - st[2]) * st[3];
      const float dyv = a.dy[idx];
      vec[0] = fmaf(dAtt, xh1, vec[0]);      // attention_norm.weight
      vec[1] += dAtt;                        // attention_norm.bias
      vec[2] = fmaf(dyv, xh2, vec[2]);       // ff_norm.weight
      vec[3] += dyv;                         // ff_norm.bias
      vec[4] += dJ;                          // joint_linear.bias
      vec[5] += dF;                          // ff.2.bias
    }
    if (hbias) {                                                 // (block-uniform)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        hq[i] += dqr[i];
        hk[i] += dkr[i];
        hv[i] += dvr[i];
        h0[i] += dhr[hb + i];
      }
    }
  }

  const int acc = a.accumulate;
  const size_t hd = (size_t)(hb + slot) * D + d, dh = (size_t)d * H + hb + slot;
  pgrad_store(a.g.wq + hd, pgrad_fold(aq, red, slot, c), acc);
  pgrad_store(a.g.wk + hd, pgrad_fold(ak, red, slot, c), acc);
  pgrad_store(a.g.wv + hd, pgrad_fold(av, red, slot, c), acc);
  pgrad_store(a.g.w0 + hd, pgrad_fold(a0, red, slot, c), acc);
  pgrad_store(a.g.wj + dh, pgrad_fold(aj, red, slot, c), acc);
  pgrad_store(a.g.w2 + dh, pgrad_fold(a2, red, slot, c), acc);
  if (vecs) {
    const float s = pgrad_fold(vec, red, slot, c);
    float* dst = slot == 0 ? a.g.g1 : slot == 1 ? a.g.be1 : slot == 2 ? a.g.g2 : slot == 3 ? a.g.be2 : slot == 4 ? a.g.bj : a.g.b2;
    if (slot < 6) pgrad_store(dst + d, s, acc);
  }
  if (hbias) {
    float s = pgrad_fold(hq, red, slot, c);
    if (c == 0) pgrad_store(a.g.bq + hb + slot, s, acc);
    s = pgrad_fold(hk, red, slot, c);
    if (c == 0) pgrad_store(a.g.bk + hb + slot, s, acc);
    s = pgrad_fold(hv, red, slot, c);
    if (c == 0) pgrad_store(a.g.bv + hb + slot, s, acc);
    s = pgrad_fold(h0, red, slot, c);
    if (c == 0) pgrad_store(a.g.b0 + hb + slot, s, acc);
  }
}

// ---- host entry points (include/deepards_hip.h) -------------------------------------------------------------------------
static bool tfm_shape_ok(int B, int T, int D, int H, float p) {
  return B >= 0 && T >= 1 && T <= 64 && D >= 64 && D <= 2048 && D % 64 == 0 && H >= 8 && H <= 64 && H % 8 == 0 && p >= 0.f &&
         p < 1.f && (long)B * T * D < (1l << 31);
}
static bool tfm_ptrs_ok(const void* const* ptrs, int n) {
  if (!ptrs) return false;
  for (int i = 0; i < n; ++i)
    if (!ptrs[i] || ((uintptr_t)ptrs[i] & 15)) return false;        // float4 loads of the weight rows
  return true;
}
#define TFM_FWD_TPW 5
#define TFM_BWD_TPW 3

// tokens a wave works on per pass: the weights it streams are shared by all of them; 1 where the rows would not fit LDS
static bool tfm_multi(int T, int D, int H) { return D <= 512 && T * H <= 1024; }
static int tfm_fwd_tokens(int T, int D, int H) { return tfm_multi(T, D, H) ? TFM_FWD_TPW : 1; }
static int tfm_bwd_tokens(int T, int D, int H) { return tfm_multi(T, D, H) ? TFM_BWD_TPW : 1; }
// dynamic LDS of the two kernels (their layouts are above each kernel), tpw = tokens per wave and pass
static size_t tfm_fwd_lds(int T, int D, int H, int tpw) {
  return ((size_t)3 * T * H + (size_t)TFM_NW * tpw * D) * sizeof(float);
}
static size_t tfm_bwd_lds(int T, int D, int H, int tpw) {
  return ((size_t)5 * T * H + 4 * T + (size_t)TFM_NW * tpw * 2 * D) * sizeof(float);
}

// dynamic LDS above the 64 KB default needs the attribute once per kernel AND device (the flag is a hint only: two threads
// racing here both set the same value)
#define TFM_MAX_DEVICES 64
template <typename K>
static int tfm_lds_attr(K kernel, size_t bytes, bool* done) {
  if (bytes > 160 * 1024) return DA_EINVAL;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return DA_EINVAL;
  if (dev >= TFM_MAX_DEVICES || !done[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess)
      return DA_EINVAL;
    if (dev < TFM_MAX_DEVICES) done[dev] = true;
  }
  return DA_OK;
}

extern "C" {

int da_tfm_block_form(int T, int D, int H, int* tokens_fwd, int* tokens_bwd, size_t* lds_fwd, size_t* lds_bwd) {
  if (!tfm_shape_ok(0, T, D, H, 0.f) || !tokens_fwd || !tokens_bwd || !lds_fwd || !lds_bwd) return DA_EINVAL;
  *tokens_fwd = tfm_fwd_tokens(T, D, H);
  *tokens_bwd = tfm_bwd_tokens(T, D, H);
  *lds_fwd = tfm_fwd_lds(T, D, H, *tokens_fwd);
  *lds_bwd = tfm_bwd_lds(T, D, H, *tokens_bwd);
  return DA_OK;
}

int da_tfm_block_fwd(const float* x, const float* const* params, float* y, float* q, float* k, float* v, float* aw, float* hid,
                     float* stats, int B, int T, int D, int H, const int64_t* seed, unsigned salt1, unsigned salt2, float p,
                     hipStream_t stream) {
  DA_ENTER();
  if (!tfm_shape_ok(B, T, D, H, p) || !tfm_ptrs_ok((const void* const*)params, 16) || (p > 0.f && !seed)) return DA_EINVAL;
  if (B == 0) return DA_OK;
  if (!x || !y || !q || !k || !v || !aw || !hid || !stats) return DA_EINVAL;
  TfmFwdArgs a;
  a.x = x;
  memcpy(&a.p, params, sizeof(a.p));
  a.y = y; a.q = q; a.k = k; a.v = v; a.aw = aw; a.hid = hid; a.stats = stats;
  a.T = T; a.D = D; a.H = H; a.seed = seed; a.salt1 = salt1; a.salt2 = salt2; a.drop_p = p;
  static bool attr[2][TFM_MAX_DEVICES];
  const int tpw = tfm_fwd_tokens(T, D, H);
  const size_t lds = tfm_fwd_lds(T, D, H, tpw);
  if (tpw == TFM_FWD_TPW) {
    if (tfm_lds_attr(tfm_fwd_kernel<TFM_FWD_TPW>, lds, attr[0]) != DA_OK) return DA_EINVAL;
    hipLaunchKernelGGL(tfm_fwd_kernel<TFM_FWD_TPW>, dim3(B), dim3(256), lds, stream, a);
  } else {
    if (tfm_lds_attr(tfm_fwd_kernel<1>, lds, attr[1]) != DA_OK) return DA_EINVAL;
    hipLaunchKernelGGL(tfm_fwd_kernel<1>, dim3(B), dim3(256), lds, stream, a);
  }
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_tfm_block_bwd(const float* dy, const float* x, const float* const* params, const float* q, const float* k, const float* v,
                     const float* aw, const float* hid, const float* stats, float* dx, float* dq, float* dk, float* dv,
                     float* dhid, float* da1, float* da2, float* wv, int B, int T, int D, int H, const int64_t* seed,
                     unsigned salt1, unsigned salt2, float p, hipStream_t stream) {
  DA_ENTER();
  if (!tfm_shape_ok(B, T, D, H, p) || !tfm_ptrs_ok((const void* const*)params, 16) || (p > 0.f && !seed)) return DA_EINVAL;
  if (B == 0) return DA_OK;
  if (!dy || !x || !q || !k || !v || !aw || !hid || !stats || !dx || !dq || !dk || !dv || !dhid || !da1 || !da2 || !wv)
    return DA_EINVAL;
  if (((uintptr_t)hid & 15)) return DA_EINVAL;
  TfmBwdArgs a;
  a.dy = dy; a.x = x;
  memcpy(&a.p, params, sizeof(a.p));
  a.q = q; a.k = k; a.v = v; a.aw = aw; a.hid = hid; a.stats = stats;
  a.dx = dx; a.dq = dq; a.dk = dk; a.dv = dv; a.dhid = dhid; a.da1 = da1; a.da2 = da2; a.wv = wv;
  a.T = T; a.D = D; a.H = H; a.seed = seed; a.salt1 = salt1; a.salt2 = salt2; a.drop_p = p;
  static bool attr[2][TFM_MAX_DEVICES];
  const int tpw = tfm_bwd_tokens(T, D, H);
  const size_t lds = tfm_bwd_lds(T, D, H, tpw);
  if (tpw == TFM_BWD_TPW) {
    if (tfm_lds_attr(tfm_bwd_kernel<TFM_BWD_TPW>, lds, attr[0]) != DA_OK) return DA_EINVAL;
    hipLaunchKernelGGL(tfm_bwd_kernel<TFM_BWD_TPW>, dim3(B), dim3(256), lds, stream, a);
  } else {
    if (tfm_lds_attr(tfm_bwd_kernel<1>, lds, attr[1]) != DA_OK) return DA_EINVAL;
    hipLaunchKernelGGL(tfm_bwd_kernel<1>, dim3(B), dim3(256), lds, stream, a);
  }
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_tfm_block_pgrad(const float* dy, const float* x, const float* const* params, const float* hid, const float* stats,
                       const float* wv, const float* dq, const float* dk, const float* dv, const float* dhid, const float* da1,
                       const float* da2, float* const* grads, int accumulate, int B, int T, int D, int H, const int64_t* seed,
                       unsigned salt1, unsigned salt2, float p, hipStream_t stream) {
  DA_ENTER();
  if (!tfm_shape_ok(B, T, D, H, p) || !tfm_ptrs_ok((const void* const*)params, 16) || !grads || (p > 0.f && !seed))
    return DA_EINVAL;
  for (int i = 0; i < 16; ++i)
    if (!grads[i]) return DA_EINVAL;
  if (B > 0 && (!dy || !x || !hid || !stats || !wv || !dq || !dk || !dv || !dhid || !da1 || !da2)) return DA_EINVAL;
  TfmPgradArgs a;
  a.dy = dy; a.x = x;
  memcpy(&a.p, params, sizeof(a.p));
  a.hid = hid; a.stats = stats; a.wv = wv; a.dq = dq; a.dk = dk; a.dv = dv; a.dhid = dhid; a.da1 = da1; a.da2 = da2;
  memcpy(&a.g, grads, sizeof(a.g));
  a.accumulate = accumulate ? 1 : 0;
  a.NT = B * T; a.D = D; a.H = H; a.seed = seed; a.salt1 = salt1; a.salt2 = salt2; a.drop_p = p;
  hipLaunchKernelGGL(tfm_pgrad_kernel, dim3(D / 32, H / 8), dim3(256), 0, stream, a);    // (B == 0: zeros, or nothing added)
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
