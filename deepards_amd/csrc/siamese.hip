// Siamese pretraining (reference models/siamese.py, dataset.py SiameseNetworkDataset): the triplet draw and the |a - c| head.
//
// Head, per pair p (0: anchor / positive, target [0, 1]; 1: anchor / negative, target [1, 0]) and breath row r = b NB + k:
//     u[p][r][c] = b1[c] + sum_d W1[c][d] |fc_p[r][d] - fa_p[r][d]|                      c = 0, 1      (linear_intermediate)
//     z[p][b][o] = b2[o] + sum_j W2[o][j] u[p][b NB ..][j]                               j = 2 k + c   (linear_final)
//     loss       = (1 / 2B) sum_{p,b,o} max(z, 0) - z t + log1p(exp(-|z|))               = mean BCE(pos) + mean BCE(neg)
//
// These are streaming kernels: the forward reads the four (three with a shared anchor) [B NB][D] operands once, the backward
// reads them once more and writes as many gradients.  Decomposition:
//
//   siamese_rows_fwd_kernel   SH_ROWS rows per block, one wave per row at a time (both pairs, so a shared anchor is loaded
//                             once): every lane runs one fmaf chain per (pair, c) over its columns d = 4 lane + 256 i (16-byte
//                             loads; d = lane + 64 i on the scalar path), then an xor-shuffle tree over the 64 lanes.
//   siamese_finish_fwd_kernel one block: z (one thread per logit, an fmaf chain j = 0 .. 2 NB - 1 from the bias), the BCE terms,
//                             their sum as a strided per-thread chain and a fixed LDS tree.
//   siamese_rows_bwd_kernel   the same row blocks; a thread owns 4 (1) columns and walks the block's rows in order: du from z and
//                             W2 (block prologue, LDS), dfc = sign(fc - fa) (W1[0][d] du0 + W1[1][d] du1), dfa = -dfc -- with a
//                             shared anchor (-dfc_pos) + (-dfc_neg), formed here -- and the block's share of dW1 in registers
//                             (row order, pos before neg), written as ONE partial row per block.
//   siamese_finish_bwd_kernel dW1 = the partial rows folded in block order (one thread per element); one more block for dW2,
//                             db2, db1 (per-thread strided chains + the same LDS tree).
//
// No float atomics anywhere: every sum's order is a function of (B, NB, D) only, so two runs give the same bits.
#include "common.h"

constexpr int SH_ROWS = 8;             // rows of one block of the two row kernels (da_siamese_head_rows_per_block)
constexpr int SH_BT = 256;

// dz = (sigmoid(z) - t) gs of logit o of pair p: t = o for the positive pair ([0, 1]), 1 - o for the negative one ([1, 0])
__device__ __forceinline__ float siamese_dz(float z, int p, int o, float gs) {
  const float t = (float)(p == 0 ? o : 1 - o);
  return (1.0f / (1.0f + expf(-z)) - t) * gs;
}

template <bool VEC>
__global__ __launch_bounds__(SH_BT) void siamese_rows_fwd_kernel(const float* __restrict__ fa_p, const float* __restrict__ fc_p,
                                                                 const float* __restrict__ fa_n, const float* __restrict__ fc_n,
                                                                 int ld, const float* __restrict__ W1, const float* __restrict__ b1,
                                                                 float* __restrict__ u, int R, int D) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool shared = fa_p == fa_n;
  for (int k = wave; k < SH_ROWS; k += SH_BT / 64) {
    const int r = blockIdx.x * SH_ROWS + k;
    if (r >= R) break;
    const size_t off = (size_t)r * ld;
    float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;                       // [pair][c]
    if constexpr (VEC) {
      for (int d = lane * 4; d < D; d += 256) {
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(W1 + d), w1 = *reinterpret_cast<const f32x4*>(W1 + D + d);
        const f32x4 ap = *reinterpret_cast<const f32x4*>(fa_p + off + d), cp = *reinterpret_cast<const f32x4*>(fc_p + off + d);
        const f32x4 an = shared ? ap : *reinterpret_cast<const f32x4*>(fa_n + off + d);
        const f32x4 cn = *reinterpret_cast<const f32x4*>(fc_n + off + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xp = fabsf(cp[e] - ap[e]), xn = fabsf(cn[e] - an[e]);
          a00 = fmaf(w0[e], xp, a00);
          a01 = fmaf(w1[e], xp, a01);
          a10 = fmaf(w0[e], xn, a10);
          a11 = fmaf(w1[e], xn, a11);
        }
      }
    } else {
      for (int d = lane; d < D; d += 64) {
        const float w0 = W1[d], w1 = W1[D + d];
        const float ap = fa_p[off + d], an = shared ? ap : fa_n[off + d];
        const float xp = fabsf(fc_p[off + d] - ap), xn = fabsf(fc_n[off + d] - an);
        a00 = fmaf(w0, xp, a00);
        a01 = fmaf(w1, xp, a01);
        a10 = fmaf(w0, xn, a10);
        a11 = fmaf(w1, xn, a11);
      }
    }
    a00 = wave_sum(a00);
    a01 = wave_sum(a01);
    a10 = wave_sum(a10);
    a11 = wave_sum(a11);
    if (lane == 0) {
      const float c0 = b1[0], c1 = b1[1];
      u[(size_t)r * 2] = a00 + c0;
      u[(size_t)r * 2 + 1] = a01 + c1;
      u[((size_t)R + r) * 2] = a10 + c0;
      u[((size_t)R + r) * 2 + 1] = a11 + c1;
    }
  }
}

__global__ __launch_bounds__(SH_BT) void siamese_finish_fwd_kernel(const float* __restrict__ u, const float* __restrict__ W2,
                                                                   const float* __restrict__ b2, float* __restrict__ z,
                                                                   float* __restrict__ loss, int B, int NB) {
  __shared__ float red[SH_BT];
  const int n = 4 * B, J = 2 * NB;
  float local = 0.f;
  for (int i = threadIdx.x; i < n; i += SH_BT) {
    const int p = i / (2 * B), b = (i >> 1) % B, o = i & 1;
    const float* uu = u + ((size_t)p * B + b) * J;                          // u[p][b NB ..][.]: J consecutive floats
    const float* w = W2 + (size_t)o * J;
    float acc = b2[o];
    for (int j = 0; j < J; ++j) acc = fmaf(w[j], uu[j], acc);
    z[i] = acc;
    const float t = (float)(p == 0 ? o : 1 - o);
    local += fmaxf(acc, 0.f) - acc * t + log1pf(expf(-fabsf(acc)));
  }
  const float s = block_tree_sum<SH_BT>(local, red);
  if (threadIdx.x == 0) loss[0] = s / (float)(2 * B);
}

template <bool VEC>
__global__ __launch_bounds__(SH_BT) void siamese_rows_bwd_kernel(
    const float* __restrict__ fa_p, const float* __restrict__ fc_p, const float* __restrict__ fa_n, const float* __restrict__ fc_n,
    int ld, const float* __restrict__ W1, const float* __restrict__ W2, const float* __restrict__ z, float* __restrict__ dfa_p,
    float* __restrict__ dfc_p, float* __restrict__ dfa_n, float* __restrict__ dfc_n, int ldg, float* __restrict__ part, int R,
    int NB, int B, int D, float gs) {
  __shared__ float du_s[SH_ROWS][2][2];                                     // [row][pair][c]
  constexpr int W = VEC ? 4 : 1;
  const int tid = threadIdx.x, r0 = blockIdx.x * SH_ROWS;
  const bool shared = fa_p == fa_n;
  if (tid < SH_ROWS * 4) {
    const int k = tid >> 2, p = (tid >> 1) & 1, c = tid & 1, r = r0 + k;
    float du = 0.f;
    if (r < R) {
      const int b = r / NB, j = (r - b * NB) * 2 + c;
      const float z0 = z[((size_t)p * B + b) * 2], z1 = z[((size_t)p * B + b) * 2 + 1];
      du = fmaf(W2[j], siamese_dz(z0, p, 0, gs), W2[2 * NB + j] * siamese_dz(z1, p, 1, gs));
    }
    du_s[k][p][c] = du;
  }
  __syncthreads();
  const int rows = min(SH_ROWS, R - r0);
  for (int d = tid * W; d < D; d += blockDim.x * W) {
    float w0[W], w1[W], acc0[W], acc1[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      w0[e] = W1[d + e];
      w1[e] = W1[D + d + e];
      acc0[e] = acc1[e] = 0.f;
    }
    for (int k = 0; k < rows; ++k) {
      const size_t off = (size_t)(r0 + k) * ld + d, goff = (size_t)(r0 + k) * ldg + d;
      const float dp0 = du_s[k][0][0], dp1 = du_s[k][0][1], dn0 = du_s[k][1][0], dn1 = du_s[k][1][1];
      alignas(16) float ap[W], cp[W], an[W], cn[W], gp[W], gn[W], ga[W];
      if constexpr (VEC) {
        *reinterpret_cast<f32x4*>(ap) = *reinterpret_cast<const f32x4*>(fa_p + off);
        *reinterpret_cast<f32x4*>(cp) = *reinterpret_cast<const f32x4*>(fc_p + off);
        *reinterpret_cast<f32x4*>(cn) = *reinterpret_cast<const f32x4*>(fc_n + off);
        if (!shared) *reinterpret_cast<f32x4*>(an) = *reinterpret_cast<const f32x4*>(fa_n + off);
      } else {
        ap[0] = fa_p[off];
        cp[0] = fc_p[off];
        cn[0] = fc_n[off];
        if (!shared) an[0] = fa_n[off];
      }
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const float xp = cp[e] - ap[e], xn = cn[e] - (shared ? ap[e] : an[e]);
        const float sp = (float)((xp > 0.f) - (xp < 0.f)), sn = (float)((xn > 0.f) - (xn < 0.f));       // sign(0) = 0
        gp[e] = sp * fmaf(w0[e], dp0, w1[e] * dp1);
        gn[e] = sn * fmaf(w0[e], dn0, w1[e] * dn1);
        ga[e] = (-gp[e]) + (-gn[e]);                                        // shared anchor: pos then neg
        acc0[e] = fmaf(dp0, fabsf(xp), acc0[e]);
        acc1[e] = fmaf(dp1, fabsf(xp), acc1[e]);
        acc0[e] = fmaf(dn0, fabsf(xn), acc0[e]);
        acc1[e] = fmaf(dn1, fabsf(xn), acc1[e]);
      }
      if constexpr (VEC) {
        *reinterpret_cast<f32x4*>(dfc_p + goff) = *reinterpret_cast<const f32x4*>(gp);
        *reinterpret_cast<f32x4*>(dfc_n + goff) = *reinterpret_cast<const f32x4*>(gn);
        if (shared) {
          *reinterpret_cast<f32x4*>(dfa_p + goff) = *reinterpret_cast<const f32x4*>(ga);
        } else {
          *reinterpret_cast<f32x4*>(dfa_p + goff) = f32x4{-gp[0], -gp[1], -gp[2], -gp[3]};
          *reinterpret_cast<f32x4*>(dfa_n + goff) = f32x4{-gn[0], -gn[1], -gn[2], -gn[3]};
        }
      } else {
        dfc_p[goff] = gp[0];
        dfc_n[goff] = gn[0];
        if (shared) {
          dfa_p[goff] = ga[0];
        } else {
          dfa_p[goff] = -gp[0];
          dfa_n[goff] = -gn[0];
        }
      }
    }
    float* pr = part + (size_t)blockIdx.x * 2 * D + d;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      pr[e] = acc0[e];
      pr[D + e] = acc1[e];
    }
  }
}

// blocks 0 .. gridDim.x - 2: dW1; the last block: dW2, db2, db1 (dzs: 4 B floats of workspace, written then read here)
__global__ __launch_bounds__(SH_BT) void siamese_finish_bwd_kernel(const float* __restrict__ part, int G, const float* __restrict__ u,
                                                                   const float* __restrict__ z, const float* __restrict__ W2,
                                                                   float* __restrict__ dzs, float* __restrict__ dW1,
                                                                   float* __restrict__ db1, float* __restrict__ dW2,
                                                                   float* __restrict__ db2, int B, int NB, int D, float gs,
                                                                   int accumulate) {
  __shared__ float red[SH_BT];
  const int tid = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    const int i = blockIdx.x * SH_BT + tid;
    if (i < 2 * D) {
      float s = 0.f;
      for (int g = 0; g < G; ++g) s += part[(size_t)g * 2 * D + i];
      dW1[i] = accumulate ? dW1[i] + s : s;
    }
    return;
  }
  const int R = B * NB, J = 2 * NB;
  for (int i = tid; i < 4 * B; i += SH_BT) dzs[i] = siamese_dz(z[i], i / (2 * B), i & 1, gs);
  __syncthreads();
  for (int i = tid; i < 2 * J; i += SH_BT) {
    const int o = i / J, j = i - o * J;
    float s = 0.f;
    for (int pb = 0; pb < 2 * B; ++pb) s = fmaf(dzs[pb * 2 + o], u[(size_t)pb * J + j], s);
    dW2[i] = accumulate ? dW2[i] + s : s;
  }
  for (int o = 0; o < 2; ++o) {
    float local = 0.f;
    for (int pb = tid; pb < 2 * B; pb += SH_BT) local += dzs[pb * 2 + o];
    const float s = block_tree_sum<SH_BT>(local, red);
    if (tid == 0) db2[o] = accumulate ? db2[o] + s : s;
  }
  for (int c = 0; c < 2; ++c) {
    float local = 0.f;
    for (int i = tid; i < 2 * R; i += SH_BT) {
      const int p = i / R, r = i - p * R, b = r / NB, j = (r - b * NB) * 2 + c;
      local += fmaf(W2[j], dzs[(p * B + b) * 2], W2[J + j] * dzs[(p * B + b) * 2 + 1]);
    }
    const float s = block_tree_sum<SH_BT>(local, red);
    if (tid == 0) db1[c] = accumulate ? db1[c] + s : s;
  }
}

// One thread per batch slot.  pos: the patient's next window, the previous one behind the patient's last.  neg: uniform over the
// M = N - pat_count windows of other patients, off = (r M) >> 32 with r a 32-bit hash of (seed, step, slot): a window's
// probability differs from 1 / M by at most 2^-32, a relative bias of M / 2^32 -- below 1e-4 for any store under 400 000 windows.
// Every index is clamped into [0, N): the gather behind this reads tiles[idx] unchecked, and an anchor the host never saw must
// not carry it out of the store.
__global__ void siamese_draw_kernel(const int64_t* __restrict__ anchor, const int* __restrict__ pat_start,
                                    const int* __restrict__ pat_count, int64_t* __restrict__ out, int B, int N, uint32_t seed,
                                    uint32_t step, int literal) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int64_t a = anchor[i];
  a = a < 0 ? 0 : (a >= N ? N - 1 : a);
  const int64_t ps = pat_start[a], pc = pat_count[a];
  int64_t pos = a + 1 < ps + pc ? a + 1 : a - 1;
  const uint32_t r = mix32(mix32(seed, step), (uint32_t)i);
  const uint64_t M = (uint64_t)(N - pc > 0 ? N - pc : 1);
  const int64_t off = (int64_t)(((uint64_t)r * M) >> 32);
  int64_t neg = off < ps ? off : off + pc;
  pos = pos < 0 ? 0 : (pos >= N ? N - 1 : pos);
  neg = neg < 0 ? 0 : (neg >= N ? N - 1 : neg);
  out[i] = a;
  out[B + i] = pos;
  if (literal) {
    out[2 * B + i] = a;
    out[3 * B + i] = neg;
  } else {
    out[2 * B + i] = neg;
  }
}


static inline bool head_shape_ok(int B, int NB, int D, int ld) {
  return B >= 1 && NB >= 1 && D >= 1 && ld >= D && (long long)B * NB <= (1 << 24) && (long long)B * NB * 2 * D < (1ll << 40);
}

extern "C" {

int da_siamese_head_rows_per_block(void) { return SH_ROWS; }

int da_siamese_draw(const int64_t* anchor, const int* pat_start, const int* pat_count, int64_t* out, int B, int N, unsigned seed,
                    unsigned step, int literal, hipStream_t stream) {
  DA_ENTER();
  if (!anchor || !pat_start || !pat_count || !out || N < 2 || B < 1) return DA_EINVAL;
  hipLaunchKernelGGL(siamese_draw_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, anchor, pat_start, pat_count, out, B, N, seed,
                     step, literal);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_siamese_head_fwd(const float* fa_pos, const float* fc_pos, const float* fa_neg, const float* fc_neg, int ld, const float* W1,
                        const float* b1, const float* W2, const float* b2, float* u, float* z, float* loss, int B, int NB, int D,
                        hipStream_t stream) {
  DA_ENTER();
  if (!fa_pos || !fc_pos || !fa_neg || !fc_neg || !W1 || !b1 || !W2 || !b2 || !u || !z || !loss || !head_shape_ok(B, NB, D, ld))
    return DA_EINVAL;
  const int R = B * NB, G = (R + SH_ROWS - 1) / SH_ROWS;
  const bool vec = D % 4 == 0 && ld % 4 == 0 && aligned16(fa_pos) && aligned16(fc_pos) && aligned16(fa_neg) && aligned16(fc_neg) &&
                   aligned16(W1);
  if (vec)
    hipLaunchKernelGGL(siamese_rows_fwd_kernel<true>, dim3(G), dim3(SH_BT), 0, stream, fa_pos, fc_pos, fa_neg, fc_neg, ld, W1, b1,
                       u, R, D);
  else
    hipLaunchKernelGGL(siamese_rows_fwd_kernel<false>, dim3(G), dim3(SH_BT), 0, stream, fa_pos, fc_pos, fa_neg, fc_neg, ld, W1, b1,
                       u, R, D);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(siamese_finish_fwd_kernel, dim3(1), dim3(SH_BT), 0, stream, u, W2, b2, z, loss, B, NB);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

size_t da_siamese_head_bwd_workspace(int B, int NB, int D) {
  if (!head_shape_ok(B, NB, D, D)) return 0;
  const size_t G = ((size_t)B * NB + SH_ROWS - 1) / SH_ROWS;
  return (G * 2 * D + 4 * (size_t)B) * sizeof(float);
}

int da_siamese_head_bwd(const float* fa_pos, const float* fc_pos, const float* fa_neg, const float* fc_neg, int ld, const float* W1,
                        const float* W2, const float* u, const float* z, float* dfa_pos, float* dfc_pos, float* dfa_neg,
                        float* dfc_neg, int ldg, float* dW1, float* db1, float* dW2, float* db2, float* workspace, float gscale,
                        int accumulate, int B, int NB, int D, hipStream_t stream) {
  DA_ENTER();
  if (!fa_pos || !fc_pos || !fa_neg || !fc_neg || !W1 || !W2 || !u || !z || !dfa_pos || !dfc_pos || !dfc_neg || !dW1 || !db1 ||
      !dW2 || !db2 || !workspace || !head_shape_ok(B, NB, D, ld) || ldg < D)
    return DA_EINVAL;
  const bool shared = fa_pos == fa_neg;
  if (!shared && !dfa_neg) return DA_EINVAL;
  const int R = B * NB, G = (R + SH_ROWS - 1) / SH_ROWS;
  float* part = workspace;
  float* dzs = workspace + (size_t)G * 2 * D;
  const float gs = gscale / (float)(2 * B);
  const bool vec = D % 4 == 0 && ld % 4 == 0 && ldg % 4 == 0 && aligned16(fa_pos) && aligned16(fc_pos) && aligned16(fa_neg) &&
                   aligned16(fc_neg) && aligned16(W1) && aligned16(dfa_pos) && aligned16(dfc_pos) && aligned16(dfc_neg) &&
                   (shared || aligned16(dfa_neg)) && aligned16(part);
  const int per = vec ? 256 : 64, waves = (D + per - 1) / per;
  const int bt = 64 * (waves < 1 ? 1 : (waves > 4 ? 4 : waves));
  if (vec)
    hipLaunchKernelGGL(siamese_rows_bwd_kernel<true>, dim3(G), dim3(bt), 0, stream, fa_pos, fc_pos, fa_neg, fc_neg, ld, W1, W2, z,
                       dfa_pos, dfc_pos, dfa_neg, dfc_neg, ldg, part, R, NB, B, D, gs);
  else
    hipLaunchKernelGGL(siamese_rows_bwd_kernel<false>, dim3(G), dim3(bt), 0, stream, fa_pos, fc_pos, fa_neg, fc_neg, ld, W1, W2, z,
                       dfa_pos, dfc_pos, dfa_neg, dfc_neg, ldg, part, R, NB, B, D, gs);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(siamese_finish_bwd_kernel, dim3((2 * D + SH_BT - 1) / SH_BT + 1), dim3(SH_BT), 0, stream, part, G, u, z, W2,
                     dzs, dW1, db1, dW2, db2, B, NB, D, gs, accumulate);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
