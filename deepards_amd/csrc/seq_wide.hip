// Whole-patient recurrences of the nested networks (reference models/cnn_to_nested_layer.py: nn.RNN(128, 128) /
// nn.LSTM(128, 128), batch_first, zero initial state, over the W window vectors of ONE patient).
//
// The workload is the opposite of da_lstm_fwd's and lstm_seq.hip's: S = 1 sequence, H = 128, T = W in the hundreds or
// thousands, every step waiting for the last.  A sequence is one workgroup of 512 lanes (8 waves, two per SIMD: 256 of the
// SIMD lane's 512 unified registers each), and NOTHING that is constant over time is read from memory inside the T loop:
// w_hh (64 KiB RNN, 256 KiB LSTM -- more than the CU's 160 KiB LDS) lives in the registers of the 512 lanes, loaded once.
// The input projection gx = x W_ih^T (all steps at once) and every parameter / input gradient are GEMMs outside these kernels;
// the backward kernels only produce the pre-activation gradient dz [S][T][G].
//
// Lane mapping (tid = 4 j + q, j = 0 .. 127 the hidden unit; a unit's four lanes are one DPP quad):
//   LSTM forward   q = gate g (i, f, g, o): the lane owns row g H + j of w_hh, 128 registers; z is one fmaf chain k = 0 .. 127
//                  over h_{t-1} (LDS broadcast reads, ds_read_b128); the four activated gates meet by quad broadcasts.
//   LSTM backward  the lane owns the COLUMN slice w_hh[g H + k][j], k = 0 .. 127 (128 registers, loaded once, strided);
//                  its share of dh_{t-1}[j] = sum_k w_hh[g H + k][j] dz[g][k]; the four shares are added in the quad as
//                  (g0 + g1) + (g2 + g3).  dz of a step travels through an LDS tile [4][H + 4] (the pad keeps the four gate
//                  rows a wave reads at once on different banks).
//   RNN forward    the row j is split over the quad: lane q owns the float4 chunks q, q + 4, .. q + 28 of w_hh[j][.]
//                  (32 registers, one fmaf chain in chunk order), z = (p0 + p1) + (p2 + p3) by quad broadcasts.
//   RNN backward   the same split of COLUMN j: lane q owns w_hh[4 (q + 4 c) + e][j], c = 0 .. 7, e = 0 .. 3.
// h (forward) / dz (backward) of one step go round through a double-buffered LDS tile and ONE workgroup barrier per step.
// The per-step operands that do change (gx_t; dhs_t, gates_t, c_t) are prefetched SEQW_PF steps ahead into registers.
//
// Saved for the backward.  RNN: nothing but the output hs.  LSTM: the ACTIVATED gates [T][H][4] (unit-major, the lane
// order) and cs [T][H]: 2 048 + 512 = 2 560 bytes per step.  Recomputing the gates from cs as lstm_seq.hip does would need
// the row AND the column slice of w_hh in one lane (256 registers for the weights alone): it does not fit without scratch,
// so the gates are stored -- 5 MiB at T = 2 048, and the backward needs one set of 128 weight registers instead of two.
// Against da_lstm_bwd's form this saves, per step, the 256 KiB re-read of w_hh (64 KiB for the RNN) in each direction and
// the 256 KiB read-modify-write of the per-lane dw_hh accumulators: dW_hh = dz^T h_prev is one GEMM afterwards.
//
// Registers (hipcc -O3 --offload-arch=gfx950 --save-temps, .vgpr_count / .private_segment_fixed_size of the four kernels):
//   seqw_lstm_fwd 160 / 0   seqw_lstm_bwd 184 / 0   seqw_rnn_fwd 64 / 0   seqw_rnn_bwd 78 / 0      (budget 256; no spill,
//   no scratch: a spilled weight row would silently turn this into the kernel that re-reads w_hh every step)
//
// Arithmetic: tanhf, expf and a true division (lstm_seq.hip's gate_act, for the same reason: long dependent chains judged
// against stock float32 torch).  Every sum runs in an order fixed by H alone; no atomics; a sequence is worked on by one
// block that reads nothing of its neighbours: its bits do not depend on S or on its position.
#include "common.h"

#define SEQW_H 128
#define SEQW_BT 512
#define SEQW_PF 4                       // steps the changing operands are loaded ahead

__device__ __forceinline__ float seqw_quad_sum(float p) {               // the same bits in all four lanes
  return (quad_bcast<0>(p) + quad_bcast<1>(p)) + (quad_bcast<2>(p) + quad_bcast<3>(p));
}

// ---- tanh RNN ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SEQW_BT) void seqw_rnn_fwd_kernel(const float* __restrict__ gx, const float* __restrict__ whh,
                                                               const float* __restrict__ bih, const float* __restrict__ bhh,
                                                               float* __restrict__ hs, int T) {
  constexpr int H = SEQW_H;
  __shared__ __attribute__((aligned(16))) float hbuf[2][H];
  const int tid = threadIdx.x, j = tid >> 2, q = tid & 3;
  float w[32];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(whh + (size_t)j * H + 4 * (q + 4 * c));
    w[4 * c] = v[0]; w[4 * c + 1] = v[1]; w[4 * c + 2] = v[2]; w[4 * c + 3] = v[3];
  }
  const float b = bih[j] + bhh[j];
  const float* g = gx + (size_t)blockIdx.x * T * H + j;
  float* out = hs + (size_t)blockIdx.x * T * H + j;
  if (q == 0) hbuf[0][j] = 0.f;
  float pre[SEQW_PF];
#pragma unroll
  for (int u = 0; u < SEQW_PF; ++u) pre[u] = u < T ? g[(size_t)u * H] : 0.f;
  __syncthreads();
  for (int t0 = 0; t0 < T; t0 += SEQW_PF) {
#pragma unroll
    for (int u = 0; u < SEQW_PF; ++u) {
      const int t = t0 + u;
      if (t < T) {                                        // block-uniform
        const float gxt = pre[u];
        pre[u] = t + SEQW_PF < T ? g[(size_t)(t + SEQW_PF) * H] : 0.f;
        const float* hp = hbuf[t & 1];
        float p = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(hp + 4 * (q + 4 * c));
          p = fmaf(w[4 * c], v[0], p);
          p = fmaf(w[4 * c + 1], v[1], p);
          p = fmaf(w[4 * c + 2], v[2], p);
          p = fmaf(w[4 * c + 3], v[3], p);
        }
        const float h = tanhf((gxt + b) + seqw_quad_sum(p));
        if (q == 0) {
          out[(size_t)t * H] = h;
          hbuf[(t + 1) & 1][j] = h;
        }
        __syncthreads();
      }
    }
  }
}

__global__ __launch_bounds__(SEQW_BT) void seqw_rnn_bwd_kernel(const float* __restrict__ dhs, const float* __restrict__ whh,
                                                               const float* __restrict__ hs, float* __restrict__ dz, int T) {
  constexpr int H = SEQW_H;
  __shared__ __attribute__((aligned(16))) float dzbuf[2][H];
  const int tid = threadIdx.x, j = tid >> 2, q = tid & 3;
  float wc[32];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) wc[4 * c + e] = whh[(size_t)(4 * (q + 4 * c) + e) * H + j];
  const size_t base = (size_t)blockIdx.x * T * H + j;
  const float* dh_in = dhs + base;
  const float* h_in = hs + base;
  float* out = dz + base;
  float pd[SEQW_PF], ph[SEQW_PF];
#pragma unroll
  for (int u = 0; u < SEQW_PF; ++u) {
    const int t = T - 1 - u;
    pd[u] = t >= 0 ? dh_in[(size_t)t * H] : 0.f;
    ph[u] = t >= 0 ? h_in[(size_t)t * H] : 0.f;
  }
  float dh_rec = 0.f;
  for (int i0 = 0; i0 < T; i0 += SEQW_PF) {
#pragma unroll
    for (int u = 0; u < SEQW_PF; ++u) {
      const int it = i0 + u, t = T - 1 - it;
      if (t >= 0) {                                       // block-uniform
        const float h = ph[u];
        const float d = (pd[u] + dh_rec) * (1.f - h * h);
        const int tn = t - SEQW_PF;
        pd[u] = tn >= 0 ? dh_in[(size_t)tn * H] : 0.f;
        ph[u] = tn >= 0 ? h_in[(size_t)tn * H] : 0.f;
        if (q == 0) {
          out[(size_t)t * H] = d;
          dzbuf[it & 1][j] = d;
        }
        __syncthreads();
        if (t > 0) {                                      // (there is no gradient into the initial state)
          const float* dp = dzbuf[it & 1];
          float p = 0.f;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(dp + 4 * (q + 4 * c));
            p = fmaf(wc[4 * c], v[0], p);
            p = fmaf(wc[4 * c + 1], v[1], p);
            p = fmaf(wc[4 * c + 2], v[2], p);
            p = fmaf(wc[4 * c + 3], v[3], p);
          }
          dh_rec = seqw_quad_sum(p);
        }
      }
    }
  }
}

// ---- LSTM ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SEQW_BT) void seqw_lstm_fwd_kernel(const float* __restrict__ gx, const float* __restrict__ whh,
                                                                const float* __restrict__ bih, const float* __restrict__ bhh,
                                                                float* __restrict__ hs, float* __restrict__ cs,
                                                                float* __restrict__ gates, int T) {
  constexpr int H = SEQW_H;
  __shared__ __attribute__((aligned(16))) float hbuf[2][H];
  const int tid = threadIdx.x, j = tid >> 2, g = tid & 3, row = g * H + j;
  float w[H];
#pragma unroll
  for (int k = 0; k < H; k += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(whh + (size_t)row * H + k);
    w[k] = v[0]; w[k + 1] = v[1]; w[k + 2] = v[2]; w[k + 3] = v[3];
  }
  const float b = bih[row] + bhh[row];
  const size_t s = blockIdx.x;
  const float* gin = gx + s * T * 4 * H + row;
  float* hout = hs + s * T * H + j;
  float* cout = cs + s * T * H + j;
  float* gout = gates + s * T * 4 * H + tid;
  if (g == 0) hbuf[0][j] = 0.f;
  float pre[SEQW_PF];
#pragma unroll
  for (int u = 0; u < SEQW_PF; ++u) pre[u] = u < T ? gin[(size_t)u * 4 * H] : 0.f;
  float c = 0.f;
  __syncthreads();
  for (int t0 = 0; t0 < T; t0 += SEQW_PF) {
#pragma unroll
    for (int u = 0; u < SEQW_PF; ++u) {
      const int t = t0 + u;
      if (t < T) {                                        // block-uniform
        float z = pre[u] + b;
        pre[u] = t + SEQW_PF < T ? gin[(size_t)(t + SEQW_PF) * 4 * H] : 0.f;
        const float* hp = hbuf[t & 1];
#pragma unroll
        for (int k = 0; k < H; k += 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(hp + k);
          z = fmaf(w[k], v[0], z);
          z = fmaf(w[k + 1], v[1], z);
          z = fmaf(w[k + 2], v[2], z);
          z = fmaf(w[k + 3], v[3], z);
        }
        const float a = g == 2 ? tanhf(z) : sigmoidf_(z);
        const float ai = quad_bcast<0>(a), af = quad_bcast<1>(a), ag = quad_bcast<2>(a), ao = quad_bcast<3>(a);
        c = fmaf(af, c, ai * ag);
        const float h = ao * tanhf(c);
        gout[(size_t)t * 4 * H] = a;
        if (g == 0) {
          hout[(size_t)t * H] = h;
          hbuf[(t + 1) & 1][j] = h;
        } else if (g == 1) {
          cout[(size_t)t * H] = c;
        }
        __syncthreads();
      }
    }
  }
}

__global__ __launch_bounds__(SEQW_BT) void seqw_lstm_bwd_kernel(const float* __restrict__ dhs, const float* __restrict__ whh,
                                                                const float* __restrict__ cs, const float* __restrict__ gates,
                                                                float* __restrict__ dz, int T) {
  constexpr int H = SEQW_H, LD = H + 4;
  __shared__ __attribute__((aligned(16))) float dzbuf[2][4][LD];
  const int tid = threadIdx.x, j = tid >> 2, g = tid & 3, row = g * H + j;
  float wc[H];
#pragma unroll
  for (int k = 0; k < H; ++k) wc[k] = whh[(size_t)(g * H + k) * H + j];
  const size_t s = blockIdx.x;
  const float* dh_in = dhs + s * T * H + j;
  const float* c_in = cs + s * T * H + j;
  const float* g_in = gates + s * T * 4 * H + tid;
  float* out = dz + s * T * 4 * H + row;
  // operands of step t: dhs_t, the lane's gate a_t and c_{t-1} (c_t is the previous step's c_{t-1})
  float pd[SEQW_PF], pa[SEQW_PF], pc[SEQW_PF];
#pragma unroll
  for (int u = 0; u < SEQW_PF; ++u) {
    const int t = T - 1 - u;
    pd[u] = t >= 0 ? dh_in[(size_t)t * H] : 0.f;
    pa[u] = t >= 0 ? g_in[(size_t)t * 4 * H] : 0.f;
    pc[u] = t >= 1 ? c_in[(size_t)(t - 1) * H] : 0.f;
  }
  float ct = c_in[(size_t)(T - 1) * H];
  float dh_rec = 0.f, dc_next = 0.f;
  for (int i0 = 0; i0 < T; i0 += SEQW_PF) {
#pragma unroll
    for (int u = 0; u < SEQW_PF; ++u) {
      const int it = i0 + u, t = T - 1 - it;
      if (t >= 0) {                                       // block-uniform
        const float a = pa[u], cp = pc[u], dh = pd[u] + dh_rec;
        const int tn = t - SEQW_PF;
        pd[u] = tn >= 0 ? dh_in[(size_t)tn * H] : 0.f;
        pa[u] = tn >= 0 ? g_in[(size_t)tn * 4 * H] : 0.f;
        pc[u] = tn >= 1 ? c_in[(size_t)(tn - 1) * H] : 0.f;
        const float ai = quad_bcast<0>(a), af = quad_bcast<1>(a), ag = quad_bcast<2>(a), ao = quad_bcast<3>(a);
        const float tc = tanhf(ct);
        const float dc = fmaf(dh * ao, 1.f - tc * tc, dc_next);
        const float d = g == 0 ? dc * ag * ai * (1.f - ai)
                      : g == 1 ? dc * cp * af * (1.f - af)
                      : g == 2 ? dc * ai * (1.f - ag * ag)
                               : dh * tc * ao * (1.f - ao);
        dc_next = dc * af;
        ct = cp;
        out[(size_t)t * 4 * H] = d;
        dzbuf[it & 1][g][j] = d;
        __syncthreads();
        if (t > 0) {                                      // (there is no gradient into the initial state)
          const float* dp = dzbuf[it & 1][g];
          float p = 0.f;
#pragma unroll
          for (int k = 0; k < H; k += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(dp + k);
            p = fmaf(wc[k], v[0], p);
            p = fmaf(wc[k + 1], v[1], p);
            p = fmaf(wc[k + 2], v[2], p);
            p = fmaf(wc[k + 3], v[3], p);
          }
          dh_rec = seqw_quad_sum(p);
        }
      }
    }
  }
}

static inline bool seqw_ok(int kind, int S, int T, int H) { return (kind == 0 || kind == 1) && S >= 0 && T >= 1 && H == SEQW_H; }

extern "C" {

// kind 0: tanh RNN, 1: LSTM.  1 if the four kernels run (H, T), else 0; launches nothing.
int da_seqw_shape_ok(int kind, int H, int T) { return seqw_ok(kind, 1, T, H) ? 1 : 0; }

int da_seqw_rnn_fwd(const float* gx, const float* w_hh, const float* b_ih, const float* b_hh, float* hs, int S, int T, int H,
                    hipStream_t stream) {
  DA_ENTER();
  if (!gx || !w_hh || !b_ih || !b_hh || !hs || !seqw_ok(0, S, T, H)) return DA_EINVAL;
  if (S == 0) return DA_OK;
  hipLaunchKernelGGL(seqw_rnn_fwd_kernel, dim3(S), dim3(SEQW_BT), 0, stream, gx, w_hh, b_ih, b_hh, hs, T);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_seqw_rnn_bwd(const float* dhs, const float* w_hh, const float* hs, float* dz, int S, int T, int H, hipStream_t stream) {
  DA_ENTER();
  if (!dhs || !w_hh || !hs || !dz || !seqw_ok(0, S, T, H)) return DA_EINVAL;
  if (S == 0) return DA_OK;
  hipLaunchKernelGGL(seqw_rnn_bwd_kernel, dim3(S), dim3(SEQW_BT), 0, stream, dhs, w_hh, hs, dz, T);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_seqw_lstm_fwd(const float* gx, const float* w_hh, const float* b_ih, const float* b_hh, float* hs, float* cs, float* gates,
                     int S, int T, int H, hipStream_t stream) {
  DA_ENTER();
  if (!gx || !w_hh || !b_ih || !b_hh || !hs || !cs || !gates || !seqw_ok(1, S, T, H)) return DA_EINVAL;
  if (S == 0) return DA_OK;
  hipLaunchKernelGGL(seqw_lstm_fwd_kernel, dim3(S), dim3(SEQW_BT), 0, stream, gx, w_hh, b_ih, b_hh, hs, cs, gates, T);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_seqw_lstm_bwd(const float* dhs, const float* w_hh, const float* cs, const float* gates, float* dz, int S, int T, int H,
                     hipStream_t stream) {
  DA_ENTER();
  if (!dhs || !w_hh || !cs || !gates || !dz || !seqw_ok(1, S, T, H)) return DA_EINVAL;
  if (S == 0) return DA_OK;
  hipLaunchKernelGGL(seqw_lstm_bwd_kernel, dim3(S), dim3(SEQW_BT), 0, stream, dhs, w_hh, cs, gates, dz, T);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
