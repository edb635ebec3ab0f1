// Squeeze-and-Excitation tail of an SE-ResNet BasicBlock (reference models/senet.py:15-34 SEModule, :52-68 SEBasicBlock.forward):
//
//     out = relu(z * s + res),   z = bn2(y2),   s = sigmoid(fc2(relu(fc1(mean_L z))))      per (row, channel)
//
// float activations (rows, L, C) channels-last, BatchNorm windows of R rows, statistics (W, C).  With sc = gamma invstd and
// sh = beta - mean sc (bn_scale_shift, common.h) z = fmaf(y2, sc, sh) is NEVER stored: every kernel here that needs it
// recomputes it from y2 with that one fused multiply-add, so forward and backward see the same floats.
//
//   forward    da_se_gate_fwd    per row tile: pool = sc mean_L(y2) + sh (the affine commutes with the mean), hid, s
//              da_se_scale_fwd   out = max(fmaf(z, s, res), 0) and the ReLU decisions as one bit per element
//   backward   da_se_bwd_reduce  g = dout . mask (the residual's gradient) and dsum[row][c] = sum_l g z
//              da_se_gate_bwd    the gate's backward per row tile -> dpool, and the four parameter gradients
//              da_se_bwd_scale   dz = fmaf(g, s, dpool / L): the gradient bn2's backward (mask_mode 0) takes
//
// Every sum runs in an order fixed by the shape alone (thread-private chains, LDS folds in slot order, partials folded in
// chunk order): no atomics, the same bits every call.
#include "common.h"
#include "se_tail.h"      // Bn4, the elementwise scale kernels and the partials' fold: shared with se_wide.hip

#define SE_TR 4                       // rows per workgroup of the gate kernels: W1 / W2 are read once for all of them (8 rows a
                                      // workgroup measured slower at every stage but the last: too few workgroups at B = 64)

// ---- forward ----------------------------------------------------------------------------------------------------------
// block = SE_TR consecutive rows, 256 threads.  LDS: pl[SE_TR][C] | hd[SE_TR][Cr] | red[SE_TR * 1024]
__global__ __launch_bounds__(256) void se_gate_fwd_kernel(const float* __restrict__ y2, int rows, int R, int L, int C, int Cr,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ w2, const float* __restrict__ b2,
                                                          float* __restrict__ pool, float* __restrict__ hid, float* __restrict__ s) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* pl = sm;
  float* hd = pl + SE_TR * C;
  float* red = hd + SE_TR * Cr;
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * SE_TR, nr = min(SE_TR, rows - row0);
  const int nq = C >> 2, slots = 256 / nq;
  // 1. the row sums of y2: thread = (channel quad, slot), slot s takes positions s, s + slots, ...; folded in slot order
  {
    const int q = tid % nq, slot = tid / nq, c0 = q * 4;
    if (slot < slots) {
      for (int r = 0; r < SE_TR; ++r) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (r < nr) {
          const float* p = y2 + (size_t)(row0 + r) * L * C + c0;
          for (int l = slot; l < L; l += slots) acc += *reinterpret_cast<const f32x4*>(p + (size_t)l * C);
        }
        *reinterpret_cast<f32x4*>(red + (size_t)(r * slots + slot) * C + c0) = acc;
      }
    }
  }
  __syncthreads();
  const float inv_l = 1.0f / (float)L;
  for (int i = tid; i < SE_TR * C; i += 256) {
    const int r = i / C, c = i - r * C;
    float v = 0.f;
    if (r < nr) {
      float t = 0.f;
      for (int k = 0; k < slots; ++k) t += red[(size_t)(r * slots + k) * C + c];
      const int w = (row0 + r) / R;
      float sc, sh;
      bn_scale_shift(mean[(size_t)w * C + c], invstd[(size_t)w * C + c], gamma[c], beta[c], sc, sh);
      v = fmaf(t * inv_l, sc, sh);
      pool[(size_t)(row0 + r) * C + c] = v;
    }
    pl[i] = v;
  }
  __syncthreads();
  // 2. hid = relu(W1 pool + b1): output j by tpo = 256 / Cr threads, part p takes the quads p, p + tpo, ...; folded in part order
  const int tpo = 256 / Cr;
  {
    const int j = tid / tpo, part = tid - j * tpo;
    float acc[SE_TR];
#pragma unroll
    for (int r = 0; r < SE_TR; ++r) acc[r] = 0.f;
    const float* wr = w1 + (size_t)j * C;
    for (int qq = part; qq < nq; qq += tpo) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + 4 * qq);
#pragma unroll
      for (int r = 0; r < SE_TR; ++r) {
        const f32x4 pv = *reinterpret_cast<const f32x4*>(pl + r * C + 4 * qq);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r] = fmaf(wv[e], pv[e], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < SE_TR; ++r) red[(r * Cr + j) * tpo + part] = acc[r];
  }
  __syncthreads();
  for (int i = tid; i < SE_TR * Cr; i += 256) {
    const int r = i / Cr, j = i - r * Cr;
    float t = 0.f;
    for (int k = 0; k < tpo; ++k) t += red[i * tpo + k];
    t = fmaxf(t + b1[j], 0.f);
    hd[i] = t;
    if (r < nr) hid[(size_t)(row0 + r) * Cr + j] = t;
  }
  __syncthreads();
  // 3. s = sigmoid(W2 hid + b2): one thread per output channel
  for (int c = tid; c < C; c += 256) {
    float acc[SE_TR];
#pragma unroll
    for (int r = 0; r < SE_TR; ++r) acc[r] = 0.f;
    const float* wr = w2 + (size_t)c * Cr;
    for (int jq = 0; jq < Cr; jq += 4) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + jq);
#pragma unroll
      for (int r = 0; r < SE_TR; ++r) {
        const f32x4 hv = *reinterpret_cast<const f32x4*>(hd + r * Cr + jq);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r] = fmaf(wv[e], hv[e], acc[r]);
      }
    }
    const float bias = b2[c];
#pragma unroll
    for (int r = 0; r < SE_TR; ++r)
      if (r < nr) s[(size_t)(row0 + r) * C + c] = 1.0f / (1.0f + expf(-(acc[r] + bias)));
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// block = one row; thread = (channel quad, slot), slot s takes positions s, s + slots, ...; dsum folded in slot order
__global__ __launch_bounds__(256) void se_bwd_reduce_kernel(const float* __restrict__ dout, const unsigned char* __restrict__ mask,
                                                            const float* __restrict__ y2, float* __restrict__ g,
                                                            float* __restrict__ dsum, int R, int L, int C,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta) {
  __shared__ __attribute__((aligned(16))) float red[1024];
  const int row = blockIdx.x, nq = C >> 2, slots = 256 / nq;
  const int q = threadIdx.x % nq, slot = threadIdx.x / nq, c0 = q * 4;
  if (slot < slots) {
    Bn4 bn;
    bn.load(mean, invstd, gamma, beta, (size_t)(row / R), C, c0);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int l = slot; l < L; l += slots) {
      const size_t el = ((size_t)row * L + l) * C + c0;
      const f32x4 d = *reinterpret_cast<const f32x4*>(dout + el);
      const unsigned m = (unsigned)mask[el >> 3] >> (c0 & 4);
      const f32x4 z = bn.z(*reinterpret_cast<const f32x4*>(y2 + el));
      f32x4 gv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        gv[e] = (m >> e) & 1u ? d[e] : 0.f;
        acc[e] = fmaf(gv[e], z[e], acc[e]);
      }
      *reinterpret_cast<f32x4*>(g + el) = gv;
    }
    *reinterpret_cast<f32x4*>(red + slot * C + c0) = acc;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float t = 0.f;
    for (int k = 0; k < slots; ++k) t += red[k * C + c];
    dsum[(size_t)row * C + c] = t;
  }
}

// block = SE_TR consecutive rows.  LDS: dp[SE_TR][C] | dh[SE_TR][Cr] | red[SE_TR * 256]
__global__ __launch_bounds__(256) void se_gate_bwd_kernel(const float* __restrict__ dsum, const float* __restrict__ s,
                                                          const float* __restrict__ hid, const float* __restrict__ w1,
                                                          const float* __restrict__ w2, float* __restrict__ dpre2,
                                                          float* __restrict__ dhid, float* __restrict__ dpool, int rows, int C, int Cr) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* dp = sm;
  float* dh = dp + SE_TR * C;
  float* red = dh + SE_TR * Cr;
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * SE_TR, nr = min(SE_TR, rows - row0);
  for (int i = tid; i < SE_TR * C; i += 256) {                     // dpre2 = dsum s (1 - s)
    const int r = i / C, c = i - r * C;
    float v = 0.f;
    if (r < nr) {
      const size_t k = (size_t)(row0 + r) * C + c;
      const float sv = s[k];
      v = dsum[k] * sv * (1.0f - sv);
      dpre2[k] = v;
    }
    dp[i] = v;
  }
  __syncthreads();
  const int tpo = 256 / Cr;
  {                                                                 // dhid = (W2^T dpre2) . (hid > 0): part p takes channels p, p + tpo, ...
    const int part = tid / Cr, j = tid - part * Cr;
    float acc[SE_TR];
#pragma unroll
    for (int r = 0; r < SE_TR; ++r) acc[r] = 0.f;
    for (int c = part; c < C; c += tpo) {
      const float wv = w2[(size_t)c * Cr + j];
#pragma unroll
      for (int r = 0; r < SE_TR; ++r) acc[r] = fmaf(wv, dp[r * C + c], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < SE_TR; ++r) red[(r * Cr + j) * tpo + part] = acc[r];
  }
  __syncthreads();
  for (int i = tid; i < SE_TR * Cr; i += 256) {
    const int r = i / Cr, j = i - r * Cr;
    float v = 0.f;
    if (r < nr) {
      float t = 0.f;
      for (int k = 0; k < tpo; ++k) t += red[i * tpo + k];
      const size_t k2 = (size_t)(row0 + r) * Cr + j;
      v = hid[k2] > 0.f ? t : 0.f;
      dhid[k2] = v;
    }
    dh[i] = v;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {                              // dpool = W1^T dhid
    float acc[SE_TR];
#pragma unroll
    for (int r = 0; r < SE_TR; ++r) acc[r] = 0.f;
    for (int j = 0; j < Cr; ++j) {
      const float wv = w1[(size_t)j * C + c];
#pragma unroll
      for (int r = 0; r < SE_TR; ++r) acc[r] = fmaf(wv, dh[r * Cr + j], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < SE_TR; ++r)
      if (r < nr) dpool[(size_t)(row0 + r) * C + c] = acc[r];
  }
}

// The parameter gradients as partials over chunks of `rc` consecutive rows: elements [4 i, 4 i + 4) of [dW2 (C, Cr) | db2 (C) |
// dW1 (Cr, C) | db1 (Cr)] of chunk blockIdx.y, each summed over the chunk's rows in row order by one thread (the four share
// their left operand; every section's size is a multiple of 4, so a quad never straddles two).
__global__ __launch_bounds__(256) void se_pgrad_partial_kernel(const float* __restrict__ dpre2, const float* __restrict__ dhid,
                                                               const float* __restrict__ hid, const float* __restrict__ pool,
                                                               float* __restrict__ part, int rows, int rc, int C, int Cr) {
  const int P = 2 * C * Cr + C + Cr;
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= P) return;
  const int r0 = blockIdx.y * rc, r1 = min(rows, r0 + rc);
  const float* a = nullptr;            // one float per row (the outer product's left factor), or none (a bias: sums of b)
  const float* b;                      // four consecutive floats per row
  int lda = 0, ldb;
  if (i < C * Cr) {                                   // dW2[c][j] = sum dpre2[r][c] hid[r][j]
    a = dpre2 + i / Cr; lda = C; b = hid + i % Cr; ldb = Cr;
  } else if (i < C * Cr + C) {                        // db2[c] = sum dpre2[r][c]
    b = dpre2 + (i - C * Cr); ldb = C;
  } else if (i < 2 * C * Cr + C) {                    // dW1[j][c] = sum dhid[r][j] pool[r][c]
    const int k = i - C * Cr - C;
    a = dhid + k / C; lda = Cr; b = pool + k % C; ldb = C;
  } else {                                            // db1[j] = sum dhid[r][j]
    b = dhid + (i - 2 * C * Cr - C); ldb = Cr;
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (a) {
    for (int r = r0; r < r1; ++r) {
      const float av = a[(size_t)r * lda];
      const f32x4 bv = *reinterpret_cast<const f32x4*>(b + (size_t)r * ldb);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(av, bv[e], acc[e]);
    }
  } else {
    for (int r = r0; r < r1; ++r) acc += *reinterpret_cast<const f32x4*>(b + (size_t)r * ldb);
  }
  *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.y * P + i) = acc;
}

// shapes the kernels tile: C a multiple of 64 up to 512 (the four stages) whose quads divide a block, Cr a multiple of 16 that
// divides 256
static bool se_shape_ok(int rows, int L, int C, int Cr) {
  return rows >= 0 && L >= 1 && C >= 64 && C <= 512 && C % 64 == 0 && 256 % (C / 4) == 0 && Cr >= 16 && Cr % 16 == 0 &&
         Cr <= 256 && 256 % Cr == 0 && (C / 4) % (256 / Cr) == 0 && (size_t)rows * L < 0x7fffffffull;
}
// rows per chunk of the parameter-gradient partials: C / 2, so that a call's partials hold about rows x C floats
static inline int se_chunk_rows(int C) { return C / 2; }

extern "C" {

int da_se_gate_fwd(const float* y2, int rows, int R, int L, int C, int Cr, const float* mean, const float* invstd,
                   const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2, const float* b2,
                   float* pool, float* hid, float* s, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!y2 || !mean || !invstd || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !pool || !hid || !s || R < 1 || rows % R ||
      !se_shape_ok(rows, L, C, Cr))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  const size_t shm = ((size_t)SE_TR * C + (size_t)SE_TR * Cr + (size_t)SE_TR * 1024) * sizeof(float);
  hipLaunchKernelGGL(se_gate_fwd_kernel, dim3((rows + SE_TR - 1) / SE_TR), dim3(256), shm, stream, y2, rows, R, L, C, Cr, mean,
                     invstd, gamma, beta, w1, b1, w2, b2, pool, hid, s);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_se_scale_fwd(const float* y2, const float* res, float* out, void* mask, int rows, int R, int L, int C, const float* mean,
                    const float* invstd, const float* gamma, const float* beta, const float* s, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!y2 || !res || !out || !mask || !mean || !invstd || !gamma || !beta || !s || R < 1 || rows % R || !se_shape_ok(rows, L, C, 16))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  const size_t npos = (size_t)rows * L;
  hipLaunchKernelGGL(se_scale_fwd_kernel, dim3(grid_stride_blocks(npos * (C / 8))), dim3(256), 0, stream, y2, res, out, (unsigned char*)mask,
                     npos, L, R * L, C, mean, invstd, gamma, beta, s);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_se_bwd_reduce(const float* dout, const void* mask, const float* y2, float* g, float* dsum, int rows, int R, int L, int C,
                     const float* mean, const float* invstd, const float* gamma, const float* beta, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!dout || !mask || !y2 || !g || !dsum || !mean || !invstd || !gamma || !beta || R < 1 || rows % R || !se_shape_ok(rows, L, C, 16))
    return DA_EINVAL;
  if (rows == 0) return DA_OK;
  hipLaunchKernelGGL(se_bwd_reduce_kernel, dim3(rows), dim3(256), 0, stream, dout, (const unsigned char*)mask, y2, g, dsum, R, L, C,
                     mean, invstd, gamma, beta);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// bytes of scratch da_se_gate_bwd needs: dpre2 (rows, C), dhid (rows, Cr) and the parameter-gradient partials
size_t da_se_gate_bwd_workspace(int rows, int C, int Cr) {
  if (rows < 0 || C < 2 || Cr < 1) return 0;
  const int rc = se_chunk_rows(C), nchunks = (rows + rc - 1) / rc;
  return ((size_t)rows * C + (size_t)rows * Cr + (size_t)nchunks * (2 * (size_t)C * Cr + C + Cr)) * sizeof(float);
}

// dsum, s, pool (rows, C), hid (rows, Cr), w1 (Cr, C), w2 (C, Cr) -> dpool (rows, C) and dw1 / db1 / dw2 / db2 (+= when accumulate)
int da_se_gate_bwd(const float* dsum, const float* s, const float* hid, const float* pool, const float* w1, const float* w2,
                   float* dpool, float* dw1, float* db1, float* dw2, float* db2, int accumulate, float* workspace, int rows, int C,
                   int Cr, hipStream_t stream) {
  DA_ENTER();
  if (!dsum || !s || !hid || !pool || !w1 || !w2 || !dpool || !dw1 || !db1 || !dw2 || !db2 || !workspace ||
      !se_shape_ok(rows, 1, C, Cr))
    return DA_EINVAL;
  const int P = 2 * C * Cr + C + Cr;
  const int rc = se_chunk_rows(C), nchunks = (rows + rc - 1) / rc;
  float* dpre2 = workspace;
  float* dhid = dpre2 + (size_t)rows * C;
  float* part = dhid + (size_t)rows * Cr;
  if (rows > 0) {
    if (nchunks > 65535) return DA_EINVAL;
    const size_t shm = ((size_t)SE_TR * C + (size_t)SE_TR * Cr + (size_t)SE_TR * 256) * sizeof(float);
    hipLaunchKernelGGL(se_gate_bwd_kernel, dim3((rows + SE_TR - 1) / SE_TR), dim3(256), shm, stream, dsum, s, hid, w1, w2, dpre2,
                       dhid, dpool, rows, C, Cr);
    DA_CHECK_LAUNCH();
    hipLaunchKernelGGL(se_pgrad_partial_kernel, dim3((P / 4 + 255) / 256, nchunks), dim3(256), 0, stream, dpre2, dhid, hid, pool, part,
                       rows, rc, C, Cr);
    DA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(se_pgrad_fold_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, part, nchunks, C, Cr, dw2, db2, dw1, db1,
                     accumulate);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_se_bwd_scale(const float* g, const float* s, const float* dpool, float* dz, int rows, int L, int C, hipStream_t stream) {
  DA_ENTER();
  if (g_act_bf16) return DA_EINVAL;
  if (!g || !s || !dpool || !dz || !se_shape_ok(rows, L, C, 16)) return DA_EINVAL;
  if (rows == 0) return DA_OK;
  const size_t npos = (size_t)rows * L;
  hipLaunchKernelGGL(se_bwd_scale_kernel, dim3(grid_stride_blocks(npos * (C / 4))), dim3(256), 0, stream, g, s, dpool, dz, npos, L, C);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
