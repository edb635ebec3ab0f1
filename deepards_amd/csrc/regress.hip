// Breath-metadata regression (reference models/torch_cnn_bm_regressor.py, train_ards_detector.py:1081-1099): the head of
// CNNRegressor -- AvgPool1d(7) of the breath block's last map (or its flat features), linear_final, MSELoss -- and its backward.
//
// Per breath row r (R rows: the whole batch), feature c (F) and output m (M <= 16):
//     feat[r][c] = (sum_{p = 0..6} x[r][p][c]) / 7   (map form, p rising)   |   x[r][c]   (flat form)
//     out[r][m]  = bias[m] + sum_c W[m][c] feat[r][c]
//     loss       = sum_{r,m} (out - target)^2 / (R M)
//     d[r][m]    = 2 (out - target) gscale / (R M)
//     dfeat[r][c] = sum_m d[r][m] W[m][c] (m rising)   -> dx[r][p][c] = dfeat / 7 for the seven positions | dflat[r][c]
//     dW[m][c]   = sum_r d[r][m] feat[r][c],   db[m] = sum_r d[r][m]
//
// Decomposition (two launches forward, two backward):
//   regress_rows_fwd_kernel    RG_ROWS rows per block, one wave per row at a time: a lane pools its columns c = 4 lane + 256 i
//                              (16-byte loads; c = lane + 64 i on the scalar path), writes feat once (map form: the backward
//                              reads R F floats instead of the map's 7 R F; flat form: nothing is written, feat IS x) and runs
//                              one fmaf chain per output over them, then an xor-shuffle tree over the 64 lanes per output.
//   regress_finish_fwd_kernel  one block: the squared errors as a strided per-thread chain and a fixed LDS tree.
//   regress_rows_bwd_kernel    the same row blocks; d of the block's rows in LDS (prologue); a thread owns 4 (1) columns, holds
//                              W's M values of them in registers and walks the block's rows in order: dfeat (m rising), the
//                              seven (one) stores, and the block's share of dW in registers, written as ONE partial row.
//   regress_finish_bwd_kernel  dW = the partial rows folded in block order (one thread per element); one more block for db
//                              (per-thread strided chains over r + the same LDS tree, per output).
//
// No float atomics anywhere: every sum's order is a function of (R, F, M, form) and of the path (16-byte or scalar, which the
// alignment of the operands selects), so two runs give the same bits.
#include "common.h"

constexpr int RG_ROWS = 8;             // rows of one block of the two row kernels (da_regress_rows_per_block)
constexpr int RG_BT = 256;
constexpr int RG_MAXM = 16;
constexpr int RG_POOL = 7;

// x: row r's first element at x + r rstride; position p of the map form at + p ld
template <bool VEC, bool MAP>
__global__ __launch_bounds__(RG_BT) void regress_rows_fwd_kernel(const float* __restrict__ x, int ld, const float* __restrict__ W,
                                                                 const float* __restrict__ bias, float* __restrict__ feat,
                                                                 float* __restrict__ out, int R, int F, int M) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = wave; k < RG_ROWS; k += RG_BT / 64) {
    const int r = blockIdx.x * RG_ROWS + k;
    if (r >= R) break;                                                      // (wave-uniform)
    const float* xr = x + (size_t)r * (MAP ? RG_POOL : 1) * ld;
    float acc[RG_MAXM];
#pragma unroll
    for (int m = 0; m < RG_MAXM; ++m) acc[m] = 0.f;
    if constexpr (VEC) {
      for (int c = lane * 4; c < F; c += 256) {
        f32x4 f = *reinterpret_cast<const f32x4*>(xr + c);
        if constexpr (MAP) {
#pragma unroll
          for (int p = 1; p < RG_POOL; ++p) f += *reinterpret_cast<const f32x4*>(xr + (size_t)p * ld + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) f[e] = f[e] / 7.0f;
          *reinterpret_cast<f32x4*>(feat + (size_t)r * F + c) = f;
        }
#pragma unroll
        for (int m = 0; m < RG_MAXM; ++m) {
          if (m < M) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(W + (size_t)m * F + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[m] = fmaf(w[e], f[e], acc[m]);
          }
        }
      }
    } else {
      for (int c = lane; c < F; c += 64) {
        float f = xr[c];
        if constexpr (MAP) {
#pragma unroll
          for (int p = 1; p < RG_POOL; ++p) f += xr[(size_t)p * ld + c];
          f = f / 7.0f;
          feat[(size_t)r * F + c] = f;
        }
#pragma unroll
        for (int m = 0; m < RG_MAXM; ++m)
          if (m < M) acc[m] = fmaf(W[(size_t)m * F + c], f, acc[m]);
      }
    }
#pragma unroll
    for (int m = 0; m < RG_MAXM; ++m) {
      if (m < M) {                                                          // (M is uniform: every lane shuffles)
        const float s = wave_sum(acc[m]);
        if (lane == 0) out[(size_t)r * M + m] = bias[m] + s;
      }
    }
  }
}

__global__ __launch_bounds__(RG_BT) void regress_finish_fwd_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                                   float* __restrict__ loss, int n) {
  __shared__ float red[RG_BT];
  float local = 0.f;
  for (int i = threadIdx.x; i < n; i += RG_BT) {
    const float e = out[i] - target[i];
    local = fmaf(e, e, local);
  }
  const float s = block_tree_sum<RG_BT>(local, red);
  if (threadIdx.x == 0) loss[0] = s / (float)n;
}

// feat: row r at feat + r ldf (the forward's pooled features, ldf = F, or the flat operand itself with its pitch)
// dx:   row r at dx + r (MAP ? 7 : 1) ldg, position p at + p ldg
template <bool VEC, bool MAP>
__global__ __launch_bounds__(RG_BT) void regress_rows_bwd_kernel(const float* __restrict__ feat, int ldf,
                                                                 const float* __restrict__ W, const float* __restrict__ out,
                                                                 const float* __restrict__ target, float* __restrict__ dx, int ldg,
                                                                 float* __restrict__ part, int R, int F, int M, float gs) {
  __shared__ float d_s[RG_ROWS][RG_MAXM];
  constexpr int V = VEC ? 4 : 1;
  const int tid = threadIdx.x, r0 = blockIdx.x * RG_ROWS;
  if (tid < RG_ROWS * RG_MAXM) {
    const int k = tid / RG_MAXM, m = tid % RG_MAXM, r = r0 + k;
    float d = 0.f;
    if (r < R && m < M) d = 2.0f * (out[(size_t)r * M + m] - target[(size_t)r * M + m]) * gs;
    d_s[k][m] = d;
  }
  __syncthreads();
  const int rows = min(RG_ROWS, R - r0);
  for (int c = tid * V; c < F; c += blockDim.x * V) {
    float w[RG_MAXM][V], acc[RG_MAXM][V];
#pragma unroll
    for (int m = 0; m < RG_MAXM; ++m) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        w[m][e] = m < M ? W[(size_t)m * F + c + e] : 0.f;
        acc[m][e] = 0.f;
      }
    }
    for (int k = 0; k < rows; ++k) {
      const int r = r0 + k;
      alignas(16) float f[V], g[V];
      if constexpr (VEC) *reinterpret_cast<f32x4*>(f) = *reinterpret_cast<const f32x4*>(feat + (size_t)r * ldf + c);
      else f[0] = feat[(size_t)r * ldf + c];
#pragma unroll
      for (int e = 0; e < V; ++e) g[e] = 0.f;
#pragma unroll
      for (int m = 0; m < RG_MAXM; ++m) {
        if (m < M) {
          const float d = d_s[k][m];
#pragma unroll
          for (int e = 0; e < V; ++e) {
            g[e] = fmaf(d, w[m][e], g[e]);
            acc[m][e] = fmaf(d, f[e], acc[m][e]);
          }
        }
      }
      float* dr = dx + (size_t)r * (MAP ? RG_POOL : 1) * ldg + c;
      if constexpr (MAP) {
#pragma unroll
        for (int e = 0; e < V; ++e) g[e] = g[e] / 7.0f;
#pragma unroll
        for (int p = 0; p < RG_POOL; ++p) {
          if constexpr (VEC) *reinterpret_cast<f32x4*>(dr + (size_t)p * ldg) = *reinterpret_cast<const f32x4*>(g);
          else dr[(size_t)p * ldg] = g[0];
        }
      } else {
        if constexpr (VEC) *reinterpret_cast<f32x4*>(dr) = *reinterpret_cast<const f32x4*>(g);
        else dr[0] = g[0];
      }
    }
    float* pr = part + (size_t)blockIdx.x * M * F + c;
#pragma unroll
    for (int m = 0; m < RG_MAXM; ++m) {
      if (m < M) {
#pragma unroll
        for (int e = 0; e < V; ++e) pr[(size_t)m * F + e] = acc[m][e];
      }
    }
  }
}

// blocks 0 .. gridDim.x - 2: dW; the last block: db
__global__ __launch_bounds__(RG_BT) void regress_finish_bwd_kernel(const float* __restrict__ part, int G,
                                                                   const float* __restrict__ out, const float* __restrict__ target,
                                                                   float* __restrict__ dW, float* __restrict__ db, int R, int F,
                                                                   int M, float gs, int accumulate) {
  __shared__ float red[RG_BT];
  const int tid = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    const int i = blockIdx.x * RG_BT + tid, n = M * F;
    if (i < n) {
      float s = 0.f;
      for (int g = 0; g < G; ++g) s += part[(size_t)g * n + i];
      dW[i] = accumulate ? dW[i] + s : s;
    }
    return;
  }
  for (int m = 0; m < M; ++m) {
    float local = 0.f;
    for (int r = tid; r < R; r += RG_BT) local += 2.0f * (out[(size_t)r * M + m] - target[(size_t)r * M + m]) * gs;
    const float s = block_tree_sum<RG_BT>(local, red);
    if (tid == 0) db[m] = accumulate ? db[m] + s : s;
  }
}


// form 0: flat features (R, F); form 1: the map (R, 7, F)
static inline bool rg_shape_ok(int R, int F, int M, int form) {
  return (form == 0 || form == 1) && R >= 1 && F >= 1 && M >= 1 && M <= RG_MAXM && R <= (1 << 24) && F <= (1 << 20) &&
         (long long)R * RG_POOL * F < (1ll << 40);
}

extern "C" {

int da_regress_rows_per_block(void) { return RG_ROWS; }

int da_regress_shape_ok(int R, int F, int M, int form) { return rg_shape_ok(R, F, M, form) ? 1 : 0; }

size_t da_regress_workspace(int R, int F, int M) {
  if (!rg_shape_ok(R, F, M, 0)) return 0;
  const size_t G = ((size_t)R + RG_ROWS - 1) / RG_ROWS;
  return G * (size_t)M * F * sizeof(float);
}

int da_regress_fwd(const float* x, int ld, int form, const float* W, const float* bias, const float* target, float* feat,
                   float* out, float* loss, int R, int F, int M, hipStream_t stream) {
  DA_ENTER();
  if (!rg_shape_ok(R, F, M, form) || ld < F || !x || !W || !bias || !target || !out || !loss || (form == 1 && !feat))
    return DA_EINVAL;
  const int G = (R + RG_ROWS - 1) / RG_ROWS;
  const bool vec = F % 4 == 0 && ld % 4 == 0 && aligned16(x) && aligned16(W) && (form == 0 || aligned16(feat));
  if (form == 1) {
    if (vec)
      hipLaunchKernelGGL((regress_rows_fwd_kernel<true, true>), dim3(G), dim3(RG_BT), 0, stream, x, ld, W, bias, feat, out, R, F, M);
    else
      hipLaunchKernelGGL((regress_rows_fwd_kernel<false, true>), dim3(G), dim3(RG_BT), 0, stream, x, ld, W, bias, feat, out, R, F, M);
  } else {
    if (vec)
      hipLaunchKernelGGL((regress_rows_fwd_kernel<true, false>), dim3(G), dim3(RG_BT), 0, stream, x, ld, W, bias, feat, out, R, F, M);
    else
      hipLaunchKernelGGL((regress_rows_fwd_kernel<false, false>), dim3(G), dim3(RG_BT), 0, stream, x, ld, W, bias, feat, out, R, F, M);
  }
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(regress_finish_fwd_kernel, dim3(1), dim3(RG_BT), 0, stream, out, target, loss, R * M);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_regress_bwd(const float* feat, int ldf, const float* W, const float* out, const float* target, float* dx, int ldg, int form,
                   float* dW, float* db, float* workspace, float gscale, int accumulate, int R, int F, int M, hipStream_t stream) {
  DA_ENTER();
  if (!rg_shape_ok(R, F, M, form) || ldf < F || ldg < F || !feat || !W || !out || !target || !dx || !dW || !db || !workspace)
    return DA_EINVAL;
  const int G = (R + RG_ROWS - 1) / RG_ROWS;
  const float gs = gscale / (float)(R * M);
  const bool vec = F % 4 == 0 && ldf % 4 == 0 && ldg % 4 == 0 && aligned16(feat) && aligned16(W) && aligned16(dx) &&
                   aligned16(workspace);
  const int per = vec ? 256 : 64, waves = (F + per - 1) / per;
  const int bt = 64 * (waves < 2 ? 2 : (waves > 4 ? 4 : waves));            // (>= RG_ROWS * RG_MAXM threads for the prologue)
  if (form == 1) {
    if (vec)
      hipLaunchKernelGGL((regress_rows_bwd_kernel<true, true>), dim3(G), dim3(bt), 0, stream, feat, ldf, W, out, target, dx, ldg,
                         workspace, R, F, M, gs);
    else
      hipLaunchKernelGGL((regress_rows_bwd_kernel<false, true>), dim3(G), dim3(bt), 0, stream, feat, ldf, W, out, target, dx, ldg,
                         workspace, R, F, M, gs);
  } else {
    if (vec)
      hipLaunchKernelGGL((regress_rows_bwd_kernel<true, false>), dim3(G), dim3(bt), 0, stream, feat, ldf, W, out, target, dx, ldg,
                         workspace, R, F, M, gs);
    else
      hipLaunchKernelGGL((regress_rows_bwd_kernel<false, false>), dim3(G), dim3(bt), 0, stream, feat, ldf, W, out, target, dx, ldg,
                         workspace, R, F, M, gs);
  }
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(regress_finish_bwd_kernel, dim3((M * F + RG_BT - 1) / RG_BT + 1), dim3(RG_BT), 0, stream, workspace, G, out,
                     target, dW, db, R, F, M, gs, accumulate);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
