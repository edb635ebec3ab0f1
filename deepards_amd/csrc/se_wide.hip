// Squeeze-and-Excitation tail of an SE-ResNet Bottleneck (reference models/senet.py:15-34 SEModule, :71-95 Bottleneck.forward,
// :122-144 SEResNetBottleneck) at the bottleneck's width: the gate acts on 4 planes channels with reduction 16,
// (C, Cr) = (256, 16) ... (2048, 128).  Shapes: C % 64 == 0, C <= 2048, Cr % 16 == 0, Cr <= 128.
//
//     out = relu(z * s + res),   z = bn3(y3),   s = sigmoid(fc2(relu(fc1(mean_L z))))      per (row, channel)
//
// Same contract as se.hip: z = fmaf(y3, sc, sh) (bn_scale_shift) is NEVER stored, every sum runs in an order fixed by the shape
// alone, no atomics, `accumulate` is honoured.  What differs is how the work is laid out:
//
//   forward    da_se_wide_stats       one kernel over y3 (a block reads its row slice twice, the second time from the cache):
//                                     per-row channel sums (rows, C) and centred second moments, merged over a window's rows in
//                                     row order (Chan) -> mean, invstd.  The gate reads the row sums, not the map.
//              da_se_wide_gate_fwd    pool = fmaf(rowsum / L, sc, sh) elementwise, then per tile of 32 rows hid and s as two GEMM
//                                     launches on v_mfma_f32_32x32x2_f32; W1 and W2 are each read once per row tile
//              da_se_wide_scale_fwd   se_tail.h's elementwise kernel
//   backward   da_se_wide_bwd_reduce  g = dout . mask and dsum[row][c] = sum_l g z, blocks of (row, 64 channels)
//              da_se_wide_gate_bwd    dpre2 elementwise, per tile of 32 rows dhid, dpool (two GEMM launches); the parameter gradients as
//                                     GEMMs with K = rows, split over chunks of 256 rows, partials folded in chunk order
//              da_se_wide_bwd_scale   se_tail.h's elementwise kernel
//
// The MFMA fragments (as conv_wino.hip's weight gradient): lane = (frow = lane & 31, fh = lane >> 5) gives A[m = frow][k = fh]
// and B[k = fh][n = frow]; accumulator r of the lane is D[m = (r & 3) + 8 (r >> 2) + 4 fh][n = frow].  Where an operand is
// contiguous along K a lane loads the quad k = kb + 4 fh + e, e = 0..3, once and step e of the group of 8 multiplies the e-th
// elements: the order of the K terms is a permutation fixed by the shape.
#include "common.h"
#include "se_tail.h"

#define SEW_TR 32                     // rows per workgroup of the gate kernels
#define SEW_RC 256                    // rows per chunk of the parameter-gradient partials
#define SEW_MAXCR 128

__device__ __forceinline__ int sew_m(int r, int fh) { return (r & 3) + 8 * (r >> 2) + 4 * fh; }

// ---- the two GEMM shapes of a row tile -----------------------------------------------------------------------------------
// The narrow product: tile (32 rows x the 32 outputs j0 .. j0 + 32 of Cr) of A[32][C] B[C][Cr], K = C split over the block's four
// waves -- wave w takes the groups w, w + 4, ... of 8 channels -- and folded in wave order through LDS.  A: row-major (rows, C)
// in memory, rows [row0, row0 + nr): a lane reads its row's quad of a group as it lies; bquad(c, j) gives B[c .. c + 4][j].
// Four groups' operands are loaded before their products.  -> red[32][33] holds the tile (every thread may read it).
template <class BF>
__device__ __forceinline__ void sew_gemm_narrow(const float* __restrict__ A, int row0, int nr, int C, int Cr, int j0, BF bquad,
                                                float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, frow = lane & 31, fh = lane >> 5;
  const int NG = C >> 3, j = j0 + frow;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const bool arow = frow < nr, bcol = j < Cr;
  const float* ap = A + (size_t)(row0 + (arow ? frow : 0)) * C + 4 * fh;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int g0 = wave; g0 < NG; g0 += 16) {
    f32x4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = g0 + 4 * u;
      a[u] = zero;
      b[u] = zero;
      if (g < NG && arow) a[u] = *reinterpret_cast<const f32x4*>(ap + g * 8);
      if (g < NG && bcol) b[u] = bquad(g * 8 + 4 * fh, j);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (g0 + 4 * u < NG) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][e], b[u][e], acc, 0, 0, 0);
      }
  }
  for (int w = 0; w < 4; ++w) {                         // the four waves' partial sums, in wave order
    if (wave == w) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = sew_m(r, fh) * 33 + frow;
        red[i] = w == 0 ? acc[r] : red[i] + acc[r];
      }
    }
    __syncthreads();
  }
}

// hd[32][Cr + 1] = rows [row0, row0 + nr) of the row-major (rows, Cr) table T, zero beyond nr
__device__ __forceinline__ void sew_stage_rows(const float* __restrict__ T, int row0, int nr, int Cr, float* hd) {
  for (int i = threadIdx.x; i < SEW_TR * Cr; i += 256) {
    const int m = i / Cr, j = i - m * Cr;
    hd[m * (Cr + 1) + j] = m < nr ? T[(size_t)(row0 + m) * Cr + j] : 0.f;
  }
  __syncthreads();
}

// out[32][C] = hd[32][Cr] B[Cr][C]: the 32-channel tiles are dealt to the waves of the gridDim.y blocks of a row tile (block y,
// wave w: tiles 4 y + w, + 4 gridDim.y, ...); bquad(j, c) gives B[j .. j + 4][c]; emit(m, c, v) receives every element.  A
// tile's B quads (Cr / 8 <= 16 of them) are all loaded before its first product: one memory latency a tile, not one a K group.
template <class BF, class EF>
__device__ __forceinline__ void sew_gemm_wide(int C, int Cr, const float* hd, BF bquad, EF emit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, frow = lane & 31, fh = lane >> 5;
  const int hp = Cr + 1;
  for (int t = blockIdx.y * 4 + wave; t < C / 32; t += 4 * gridDim.y) {
    const int c = t * 32 + frow;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    f32x4 b[SEW_MAXCR / 8];
#pragma unroll
    for (int i = 0; i < SEW_MAXCR / 8; ++i)
      if (i * 8 < Cr) b[i] = bquad(i * 8 + 4 * fh, c);
#pragma unroll
    for (int i = 0; i < SEW_MAXCR / 8; ++i)
      if (i * 8 < Cr) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(hd[frow * hp + i * 8 + 4 * fh + e], b[i][e], acc, 0, 0, 0);
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) emit(sew_m(r, fh), c, acc[r]);
  }
}

// ---- forward ----------------------------------------------------------------------------------------------------------
// block = (row, 64 channels); thread = (channel quad, slot), slot s takes positions s, s + 16, ...; folded in slot order.
// The row's sums, then (the row's slice is at most L x 256 bytes: the second read comes from the cache) its centred second
// moments about the row's own mean.
__global__ __launch_bounds__(256) void sew_stats_rows_kernel(const float* __restrict__ y, int L, int C, float* __restrict__ rowsum,
                                                             float* __restrict__ rowm2) {
  __shared__ __attribute__((aligned(16))) float red[16 * 64];
  __shared__ float tot[64];
  const int row = blockIdx.x, cb = blockIdx.y * 64;
  const int q = threadIdx.x & 15, slot = threadIdx.x >> 4;
  const float* p = y + (size_t)row * L * C + cb + q * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int l = slot; l < L; l += 16) acc += *reinterpret_cast<const f32x4*>(p + (size_t)l * C);
  *reinterpret_cast<f32x4*>(red + slot * 64 + q * 4) = acc;
  __syncthreads();
  if (threadIdx.x < 64) {
    float t = 0.f;
    for (int k = 0; k < 16; ++k) t += red[k * 64 + threadIdx.x];
    tot[threadIdx.x] = t;
    rowsum[(size_t)row * C + cb + threadIdx.x] = t;
  }
  __syncthreads();
  const float fl = (float)L;
  f32x4 m2 = {0.f, 0.f, 0.f, 0.f};
  float mu[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) mu[e] = tot[q * 4 + e] / fl;
  for (int l = slot; l < L; l += 16) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + (size_t)l * C);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = v[e] - mu[e];
      m2[e] = fmaf(d, d, m2[e]);
    }
  }
  *reinterpret_cast<f32x4*>(red + slot * 64 + q * 4) = m2;
  __syncthreads();
  if (threadIdx.x < 64) {
    float t = 0.f;
    for (int k = 0; k < 16; ++k) t += red[k * 64 + threadIdx.x];
    rowm2[(size_t)row * C + cb + threadIdx.x] = t;
  }
}

// thread = (window, channel): Chan's update over the window's R rows (L positions each) in row order -> mean, invstd
__global__ __launch_bounds__(256) void sew_stats_merge_kernel(const float* __restrict__ rowsum, const float* __restrict__ rowm2,
                                                              int W, int R, int L, int C, float eps, float* __restrict__ mean,
                                                              float* __restrict__ invstd) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= W * C) return;
  const int w = idx / C, c = idx - w * C;
  const float fl = (float)L;
  float mu = 0.f, m2 = 0.f, n = 0.f;
  for (int r = 0; r < R; ++r) {
    const size_t k = ((size_t)w * R + r) * C + c;
    const float mb = rowsum[k] / fl, d = mb - mu, nn = n + fl;
    mu = fmaf(d, fl / nn, mu);
    m2 = m2 + rowm2[k] + d * d * (n * fl / nn);
    n = nn;
  }
  mean[idx] = mu;
  invstd[idx] = 1.0f / sqrtf(m2 / n + eps);
}

// thread = (row, channel quad): pool = fmaf(rowsum / L, sc, sh) with the statistics of the row's own window
__global__ __launch_bounds__(256) void sew_pool_kernel(const float* __restrict__ rowsum, int rows, int R, int L, int C,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ pool) {
  const int nq = C >> 2;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * nq) return;
  const int row = (int)(idx / nq), c0 = (int)(idx - (size_t)row * nq) * 4;
  Bn4 bn;
  bn.load(mean, invstd, gamma, beta, (size_t)(row / R), C, c0);
  const f32x4 rs = *reinterpret_cast<const f32x4*>(rowsum + (size_t)row * C + c0);
  const float fl = (float)L;
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = fmaf(rs[e] / fl, bn.sc[e], bn.sh[e]);
  *reinterpret_cast<f32x4*>(pool + (size_t)row * C + c0) = o;
}

// block = (SEW_TR consecutive rows, 32 hidden units), 4 waves: hid = relu(pool W1^T + b1).  W1 is read once per row tile.
__global__ __launch_bounds__(256) void sew_hid_fwd_kernel(const float* __restrict__ pool, int rows, int C, int Cr,
                                                          const float* __restrict__ w1, const float* __restrict__ b1,
                                                          float* __restrict__ hid) {
  __shared__ float red[SEW_TR * 33];
  const int row0 = blockIdx.x * SEW_TR, nr = min(SEW_TR, rows - row0), j0 = blockIdx.y * 32;
  sew_gemm_narrow(pool, row0, nr, C, Cr, j0, [&](int c, int j) -> f32x4 { return *reinterpret_cast<const f32x4*>(w1 + (size_t)j * C + c); },
                  red);
  for (int i = threadIdx.x; i < SEW_TR * 32; i += 256) {
    const int m = i >> 5, j = j0 + (i & 31);
    if (m < nr && j < Cr) hid[(size_t)(row0 + m) * Cr + j] = fmaxf(red[m * 33 + (i & 31)] + b1[j], 0.f);
  }
}

// block = (SEW_TR consecutive rows, a share of the output channels), 4 waves: s = sigmoid(hid W2^T + b2), the 32-channel tiles
// dealt over the gridDim.y blocks of the row tile.  LDS: hd[32][Cr + 1]
__global__ __launch_bounds__(256) void sew_gate_fwd_kernel(const float* __restrict__ hid, int rows, int C, int Cr,
                                                           const float* __restrict__ w2, const float* __restrict__ b2,
                                                           float* __restrict__ s) {
  __shared__ float hd[SEW_TR * (SEW_MAXCR + 1)];
  const int row0 = blockIdx.x * SEW_TR, nr = min(SEW_TR, rows - row0);
  sew_stage_rows(hid, row0, nr, Cr, hd);
  sew_gemm_wide(
      C, Cr, hd, [&](int j, int c) -> f32x4 { return *reinterpret_cast<const f32x4*>(w2 + (size_t)c * Cr + j); },
      [&](int m, int c, float v) {
        if (m < nr) s[(size_t)(row0 + m) * C + c] = 1.0f / (1.0f + expf(-(v + b2[c])));
      });
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// block = (row, 64 channels); thread = (channel quad, slot), slot s takes positions s, s + 16, ...; dsum folded in slot order
__global__ __launch_bounds__(256) void sew_bwd_reduce_kernel(const float* __restrict__ dout, const unsigned char* __restrict__ mask,
                                                             const float* __restrict__ y, float* __restrict__ g,
                                                             float* __restrict__ dsum, int R, int L, int C,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta) {
  __shared__ __attribute__((aligned(16))) float red[16 * 64];
  const int row = blockIdx.x, cb = blockIdx.y * 64;
  const int q = threadIdx.x & 15, slot = threadIdx.x >> 4, c0 = cb + q * 4;
  Bn4 bn;
  bn.load(mean, invstd, gamma, beta, (size_t)(row / R), C, c0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int l = slot; l < L; l += 16) {
    const size_t el = ((size_t)row * L + l) * C + c0;
    const f32x4 d = *reinterpret_cast<const f32x4*>(dout + el);
    const unsigned m = (unsigned)mask[el >> 3] >> (c0 & 4);
    const f32x4 z = bn.z(*reinterpret_cast<const f32x4*>(y + el));
    f32x4 gv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      gv[e] = (m >> e) & 1u ? d[e] : 0.f;
      acc[e] = fmaf(gv[e], z[e], acc[e]);
    }
    *reinterpret_cast<f32x4*>(g + el) = gv;
  }
  *reinterpret_cast<f32x4*>(red + slot * 64 + q * 4) = acc;
  __syncthreads();
  if (threadIdx.x < 64) {
    float t = 0.f;
    for (int k = 0; k < 16; ++k) t += red[k * 64 + threadIdx.x];
    dsum[(size_t)row * C + cb + threadIdx.x] = t;
  }
}

// thread = 4 elements: dpre2 = dsum s (1 - s)
__global__ __launch_bounds__(256) void sew_dpre2_kernel(const float* __restrict__ dsum, const float* __restrict__ s,
                                                        float* __restrict__ dpre2, size_t nquads) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nquads) return;
  const f32x4 d = reinterpret_cast<const f32x4*>(dsum)[idx], sv = reinterpret_cast<const f32x4*>(s)[idx];
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = d[e] * sv[e] * (1.0f - sv[e]);
  reinterpret_cast<f32x4*>(dpre2)[idx] = o;
}

// block = (SEW_TR consecutive rows, 32 hidden units): dhid = (dpre2 W2) . (hid > 0).  W2 is read once per row tile.
__global__ __launch_bounds__(256) void sew_hid_bwd_kernel(const float* __restrict__ dpre2, const float* __restrict__ hid,
                                                          const float* __restrict__ w2, float* __restrict__ dhid, int rows, int C,
                                                          int Cr) {
  __shared__ float red[SEW_TR * 33];
  const int row0 = blockIdx.x * SEW_TR, nr = min(SEW_TR, rows - row0), j0 = blockIdx.y * 32;
  sew_gemm_narrow(
      dpre2, row0, nr, C, Cr, j0,
      [&](int c, int j) -> f32x4 {
        f32x4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = w2[(size_t)(c + e) * Cr + j];
        return b;
      },
      red);
  for (int i = threadIdx.x; i < SEW_TR * 32; i += 256) {
    const int m = i >> 5, j = j0 + (i & 31);
    if (m < nr && j < Cr) {
      const size_t k = (size_t)(row0 + m) * Cr + j;
      dhid[k] = hid[k] > 0.f ? red[m * 33 + (i & 31)] : 0.f;
    }
  }
}

// block = (SEW_TR consecutive rows, a share of dpool's channels): dpool = dhid W1, dealt over the gridDim.y blocks
__global__ __launch_bounds__(256) void sew_gate_bwd_kernel(const float* __restrict__ dhid, const float* __restrict__ w1,
                                                           float* __restrict__ dpool, int rows, int C, int Cr) {
  __shared__ float hd[SEW_TR * (SEW_MAXCR + 1)];
  const int row0 = blockIdx.x * SEW_TR, nr = min(SEW_TR, rows - row0);
  sew_stage_rows(dhid, row0, nr, Cr, hd);
  sew_gemm_wide(
      C, Cr, hd,
      [&](int j, int c) -> f32x4 {
        f32x4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = w1[(size_t)(j + e) * C + c];
        return b;
      },
      [&](int m, int c, float v) {
        if (m < nr) dpool[(size_t)(row0 + m) * C + c] = v;
      });
}

// The parameter gradients of chunk blockIdx.y (SEW_RC consecutive rows) into part[chunk][dW2 (C, Cr) | db2 (C) | dW1 (Cr, C) |
// db1 (Cr)].  Blocks [0, nbt): one 32 x 32 tile per wave, K = the chunk's rows in row order --
//     dW2[c][j] = sum_r dpre2[r][c] hid[r][j]   tiles (C / 32) x NT,       dW1[j][c] = sum_r dhid[r][j] pool[r][c]   tiles NT x (C / 32)
// (both operands are read as they lie in memory: 32 consecutive floats of row r per half wave).  Blocks [nbt, ..): the
// column sums db2 | db1, one thread per column in row order.
__global__ __launch_bounds__(256) void sew_pgrad_partial_kernel(const float* __restrict__ dpre2, const float* __restrict__ dhid,
                                                                const float* __restrict__ hid, const float* __restrict__ pool,
                                                                float* __restrict__ part, int rows, int C, int Cr, int nbt) {
  const int P = 2 * C * Cr + C + Cr;
  const int r0 = blockIdx.y * SEW_RC, r1 = min(rows, r0 + SEW_RC);
  float* out = part + (size_t)blockIdx.y * P;
  if ((int)blockIdx.x >= nbt) {
    const int i = ((int)blockIdx.x - nbt) * 256 + threadIdx.x;
    if (i >= C + Cr) return;
    const float* b = i < C ? dpre2 + i : dhid + (i - C);
    const int ld = i < C ? C : Cr;
    float t = 0.f;
    for (int r = r0; r < r1; ++r) t += b[(size_t)r * ld];
    out[i < C ? C * Cr + i : 2 * C * Cr + C + (i - C)] = t;
    return;
  }
  const int lane = threadIdx.x & 63, frow = lane & 31, fh = lane >> 5;
  const int NT = (Cr + 31) >> 5, CT = C / 32, T = CT * NT;
  int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= 2 * T) return;
  const bool second = tile >= T;                        // dW1
  if (second) tile -= T;
  // narrow index j (the Cr side, may be padded), wide index c
  const int jt = second ? tile / CT : tile % NT, ct = second ? tile % CT : tile / NT;
  const int j = jt * 32 + frow, c = ct * 32 + frow;
  const float* nar = second ? dhid : hid;               // (rows, Cr)
  const float* wid = second ? pool : dpre2;             // (rows, C)
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int rb = r0; rb < r1; rb += 16) {                // 8 K steps' operands loaded before their products
    float nv[8], wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = rb + 2 * u + fh;
      nv[u] = 0.f;
      wv[u] = 0.f;
      if (r < r1) {
        wv[u] = wid[(size_t)r * C + c];
        if (j < Cr) nv[u] = nar[(size_t)r * Cr + j];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(second ? nv[u] : wv[u], second ? wv[u] : nv[u], acc, 0, 0, 0);
  }
  if (second) {                                         // D[m = j][n = c]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jm = jt * 32 + sew_m(r, fh);
      if (jm < Cr) out[(size_t)C * Cr + C + (size_t)jm * C + c] = acc[r];
    }
  } else if (j < Cr) {                                  // D[m = c][n = j]
#pragma unroll
    for (int r = 0; r < 16; ++r) out[(size_t)(ct * 32 + sew_m(r, fh)) * Cr + j] = acc[r];
  }
}

// blocks a row tile of the wide products (s, dpool) is dealt over: enough of them to fill the machine when there are few row
// tiles (B = 64: 40), at most one 32-channel tile per wave; a function of the shape alone (and the results do not depend on it)
static inline int sew_col_blocks(int rows, int C) {
  const int tiles = (rows + SEW_TR - 1) / SEW_TR, most = C / 128 > 0 ? C / 128 : 1;
  int ns = (512 + tiles - 1) / tiles;
  if (ns > 8) ns = 8;
  return ns < most ? ns : most;
}

static bool sew_shape_ok(int rows, int L, int C, int Cr) {
  return rows >= 0 && L >= 1 && C >= 64 && C <= 2048 && C % 64 == 0 && Cr >= 16 && Cr <= SEW_MAXCR && Cr % 16 == 0 &&
         (size_t)rows * L < 0x7fffffffull && (size_t)rows * C < 0x7fffffffull;      // (int indices of (rows, C) and (W, C) tables)
}

extern "C" {

// 1 if the wide family takes (C, Cr)
int da_se_wide_shape_ok(int C, int Cr) { return sew_shape_ok(0, 1, C, Cr) ? 1 : 0; }

// y (rows, L, C), windows of R rows -> mean, invstd (rows / R, C), rowsum (rows, C); workspace: rows * C floats
int da_se_wide_stats(const float* y, int rows, int R, int L, int C, float eps, float* mean, float* invstd, float* rowsum,
                     float* workspace, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!y || !mean || !invstd || !rowsum || !workspace || R < 1 || rows % R || !sew_shape_ok(rows, L, C, 16))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  hipLaunchKernelGGL(sew_stats_rows_kernel, dim3(rows, C / 64), dim3(256), 0, stream, y, L, C, rowsum, workspace);
  DA_CHECK_LAUNCH();
  const int W = rows / R;
  hipLaunchKernelGGL(sew_stats_merge_kernel, dim3(((size_t)W * C + 255) / 256), dim3(256), 0, stream, rowsum, workspace, W, R, L, C,
                     eps, mean, invstd);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_se_wide_gate_fwd(const float* rowsum, int rows, int R, int L, int C, int Cr, const float* mean, const float* invstd,
                        const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2, const float* b2,
                        float* pool, float* hid, float* s, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!rowsum || !mean || !invstd || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !pool || !hid || !s || R < 1 || rows % R ||
      !sew_shape_ok(rows, L, C, Cr))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  hipLaunchKernelGGL(sew_pool_kernel, dim3((unsigned)(((size_t)rows * (C / 4) + 255) / 256)), dim3(256), 0, stream, rowsum, rows, R, L,
                     C, mean, invstd, gamma, beta, pool);
  DA_CHECK_LAUNCH();
  const int tiles = (rows + SEW_TR - 1) / SEW_TR;
  hipLaunchKernelGGL(sew_hid_fwd_kernel, dim3(tiles, (Cr + 31) / 32), dim3(256), 0, stream, pool, rows, C, Cr, w1, b1, hid);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(sew_gate_fwd_kernel, dim3(tiles, sew_col_blocks(rows, C)), dim3(256), 0, stream, hid, rows, C, Cr, w2, b2, s);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_se_wide_scale_fwd(const float* y, const float* res, float* out, void* mask, int rows, int R, int L, int C, const float* mean,
                         const float* invstd, const float* gamma, const float* beta, const float* s, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!y || !res || !out || !mask || !mean || !invstd || !gamma || !beta || !s || R < 1 || rows % R || !sew_shape_ok(rows, L, C, 16))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  const size_t npos = (size_t)rows * L;
  hipLaunchKernelGGL(se_scale_fwd_kernel, dim3(grid_stride_blocks(npos * (C / 8))), dim3(256), 0, stream, y, res, out, (unsigned char*)mask,
                     npos, L, R * L, C, mean, invstd, gamma, beta, s);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_se_wide_bwd_reduce(const float* dout, const void* mask, const float* y, float* g, float* dsum, int rows, int R, int L, int C,
                          const float* mean, const float* invstd, const float* gamma, const float* beta, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!dout || !mask || !y || !g || !dsum || !mean || !invstd || !gamma || !beta || R < 1 || rows % R ||
      !sew_shape_ok(rows, L, C, 16))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  hipLaunchKernelGGL(sew_bwd_reduce_kernel, dim3(rows, C / 64), dim3(256), 0, stream, dout, (const unsigned char*)mask, y, g, dsum, R,
                     L, C, mean, invstd, gamma, beta);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// rows per chunk of the parameter-gradient partials (tests reach past one chunk with it)
int da_se_wide_chunk_rows(void) { return SEW_RC; }

// bytes of scratch da_se_wide_gate_bwd needs: dpre2 (rows, C), dhid (rows, Cr) and the parameter-gradient partials
size_t da_se_wide_gate_bwd_workspace(int rows, int C, int Cr) {
  if (rows < 0 || C < 2 || Cr < 1) return 0;
  const int nchunks = (rows + SEW_RC - 1) / SEW_RC;
  return ((size_t)rows * C + (size_t)rows * Cr + (size_t)nchunks * (2 * (size_t)C * Cr + C + Cr)) * sizeof(float);
}

// dsum, s, pool (rows, C), hid (rows, Cr), w1 (Cr, C), w2 (C, Cr) -> dpool (rows, C) and dw1 / db1 / dw2 / db2 (+= when accumulate)
int da_se_wide_gate_bwd(const float* dsum, const float* s, const float* hid, const float* pool, const float* w1, const float* w2,
                        float* dpool, float* dw1, float* db1, float* dw2, float* db2, int accumulate, float* workspace, int rows,
                        int C, int Cr, hipStream_t stream) {
  DA_ENTER();
  if (!dsum || !s || !hid || !pool || !w1 || !w2 || !dpool || !dw1 || !db1 || !dw2 || !db2 || !workspace ||
      !sew_shape_ok(rows, 1, C, Cr))
    return DA_EINVAL;
  const int P = 2 * C * Cr + C + Cr;
  const int nchunks = (rows + SEW_RC - 1) / SEW_RC;
  float* dpre2 = workspace;
  float* dhid = dpre2 + (size_t)rows * C;
  float* part = dhid + (size_t)rows * Cr;
  if (rows > 0) {
    if (nchunks > 65535) return DA_EINVAL;
    hipLaunchKernelGGL(sew_dpre2_kernel, dim3((unsigned)(((size_t)rows * (C / 4) + 255) / 256)), dim3(256), 0, stream, dsum, s, dpre2,
                       (size_t)rows * (C / 4));
    DA_CHECK_LAUNCH();
    const int tiles = (rows + SEW_TR - 1) / SEW_TR;
    hipLaunchKernelGGL(sew_hid_bwd_kernel, dim3(tiles, (Cr + 31) / 32), dim3(256), 0, stream, dpre2, hid, w2, dhid, rows, C, Cr);
    DA_CHECK_LAUNCH();
    hipLaunchKernelGGL(sew_gate_bwd_kernel, dim3(tiles, sew_col_blocks(rows, C)), dim3(256), 0, stream, dhid, w1, dpool, rows, C, Cr);
    DA_CHECK_LAUNCH();
    const int T = (C / 32) * ((Cr + 31) / 32), nbt = (2 * T + 3) / 4, nbb = (C + Cr + 255) / 256;
    hipLaunchKernelGGL(sew_pgrad_partial_kernel, dim3(nbt + nbb, nchunks), dim3(256), 0, stream, dpre2, dhid, hid, pool, part, rows, C,
                       Cr, nbt);
    DA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(se_pgrad_fold_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, part, nchunks, C, Cr, dw2, db2, dw1, db1,
                     accumulate);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_se_wide_bwd_scale(const float* g, const float* s, const float* dpool, float* dz, int rows, int L, int C, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!g || !s || !dpool || !dz || !sew_shape_ok(rows, L, C, 16)) return DA_EINVAL;
  if (rows == 0) return DA_OK;
  const size_t npos = (size_t)rows * L;
  hipLaunchKernelGGL(se_bwd_scale_kernel, dim3(grid_stride_blocks(npos * (C / 4))), dim3(256), 0, stream, g, s, dpool, dz, npos, L, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
