// Waveform LSTM of the lstm_only networks (reference models/lstm_only.py: nn.LSTM(1, H, batch_first=True) over the 224 raw
// samples of every breath row, zero initial state) and the per-breath projection Linear(T H -> F) behind it.
//
// The workload: N = B NB independent sequences (1 280 at B = 64, NB = 20), T = 224 dependent steps, an input of size ONE.  There
// is no gx tensor: z_row = w_ih[row] x_t + (b_ih + b_hh)[row] + sum_k w_hh[row][k] h_k, the sum an fmaf chain k = 0 .. H - 1.
//
// Form of the two recurrence kernels (SeqCfg): a sequence is worked on by 4H lanes, lane r = 4 j + g owning gate row g H + j
// (g = 0 .. 3: i, f, g, o) with that row of w_hh in H registers for all T steps.  The four gates of a unit sit in one quad and
// are exchanged by DPP quad broadcasts; h goes round through a double-buffered LDS tile of H floats and ONE barrier per step.
// 4H <= 64: the block is a single wave (two sequences at H = 8, one at H = 16), the barrier stays inside it.  Larger H: one
// sequence per block of 4H lanes rounded up to whole waves (the spare lanes idle).
//
// Saved for the backward, per sequence: cs [T][H] floats and one int (the length) -- 14 340 bytes at T = 224, H = 16, beside
// the output hs itself; activated gates [T][4H] would be 57 344.  The backward recomputes the gates from (x_t, h_{t-1}) with
// the forward's own fmaf chain, so they are the forward's bits.
//
// Backward: reverse time; per lane the row of w_hh (gate recompute), the column slice w_hh[g H + .][j] (for W^T dz), H
// accumulators of dw_hh[row][.] and the prefetched h_{t-1}: 4H + 2H registers, sized by H (a template parameter).  dz travels
// through a double-buffered LDS tile [4][H]; the four gate-block shares of dh_{t-1}[j] meet in the quad.  A block writes ONE
// partial row (dw_hh, dw_ih, db of its `Q` consecutive sequences, in sequence order); the rows are folded by da_reduce_rows:
// every sum in an order fixed by (N, T, H), the same bits every call.
//
// packed (LSTMOnlyWithPacking: len = index of the first exact zero + 1, a row starting with a zero runs whole): step t runs
// iff x[0] == 0 or no sample among x[0 .. t - 1] equals zero -- evaluated on the fly from x; hs at t >= len is +0.0, the
// backward starts at len - 1 and never reads dhs behind it.
#include "common.h"

extern "C" int da_reduce_rows(const float* m, int rows, int n, float* out, int accumulate, hipStream_t stream);   // head_optim.hip

template <int H>
struct SeqCfg {
  static constexpr int TPS = 4 * H;                                   // lanes of one sequence
  static constexpr int BT = TPS <= 64 ? 64 : (TPS + 63) / 64 * 64;     // block threads
  static constexpr int SPB = BT / TPS;                                // sequences per block: 2 at H = 8, else 1
};

// tanh(z) or sigmoid(z) from the library's expf / tanhf and a true division, as da_lstm_fwd takes them: the errors of 224
// dependent steps are judged against stock float32 torch, so the fast v_exp_f32 / v_rcp_f32 forms (and tanh as
// 2 sigmoid(2 z) - 1, which loses the small arguments) stay out.  exp overflow gives 1 / inf = 0, never a NaN.
__device__ __forceinline__ float gate_act(float z, bool is_tanh) {
  return is_tanh ? tanhf(z) : sigmoidf_(z);
}

template <int H>
__device__ __forceinline__ float gate_z(const float (&w)[H], const float* __restrict__ h, float wx, float x, float b) {
  float z = fmaf(wx, x, b);
#pragma unroll
  for (int k = 0; k < H; k += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(h + k);
    z = fmaf(w[k], v[0], z);
    z = fmaf(w[k + 1], v[1], z);
    z = fmaf(w[k + 2], v[2], z);
    z = fmaf(w[k + 3], v[3], z);
  }
  return z;
}

template <int H>
__global__ __launch_bounds__(SeqCfg<H>::BT) void lstm_seq_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wih,
                                                                     const float* __restrict__ whh, const float* __restrict__ bih,
                                                                     const float* __restrict__ bhh, float* __restrict__ hs,
                                                                     float* __restrict__ cs, int* __restrict__ lens, int N, int T,
                                                                     int packed) {
  constexpr int TPS = SeqCfg<H>::TPS, SPB = SeqCfg<H>::SPB;
  __shared__ __attribute__((aligned(16))) float hbuf[2][SPB][H];
  const int tid = threadIdx.x;
  const bool lane_ok = tid < SPB * TPS;                 // spare lanes of the last wave: compute along, touch no memory
  const int sub = lane_ok ? tid / TPS : 0, r = tid % TPS;
  const int j = r >> 2, g = r & 3, row = g * H + j;
  const int n = blockIdx.x * SPB + sub;
  const bool live = lane_ok && n < N;
  const int nn = n < N ? n : N - 1;
  float w[H];
#pragma unroll
  for (int k = 0; k < H; k += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(whh + (size_t)row * H + k);
    w[k] = v[0]; w[k + 1] = v[1]; w[k + 2] = v[2]; w[k + 3] = v[3];
  }
  const float wx = wih[row], b = bih[row] + bhh[row];
  if (lane_ok && g == 0) hbuf[0][sub][j] = 0.f;
  __syncthreads();
  const float* xr = x + (size_t)nn * T;
  float xt = xr[0], c = 0.f;
  const bool first_zero = xt == 0.f;                    // (-0.0 == 0)
  bool seen = false;
  int len = 0;
  for (int t = 0; t < T; ++t) {
    const float xn = t + 1 < T ? xr[t + 1] : 0.f;
    const bool run = !packed || first_zero || !seen;    // uniform over the sequence's lanes
    seen = seen || xt == 0.f;
    float h = 0.f, cv = 0.f;
    if (run) {
      const float a = gate_act(gate_z<H>(w, hbuf[t & 1][sub], wx, xt, b), g == 2);
      const float ai = quad_bcast<0>(a), af = quad_bcast<1>(a), ag = quad_bcast<2>(a), ao = quad_bcast<3>(a);
      c = fmaf(af, c, ai * ag);
      h = ao * gate_act(c, true);
      cv = c;
      len = t + 1;
    }
    if (live) {
      const size_t o = ((size_t)n * T + t) * H + j;
      if (g == 0) {
        hs[o] = h;
        hbuf[(t + 1) & 1][sub][j] = h;
      } else if (g == 1) {
        cs[o] = cv;
      }
    }
    __syncthreads();
    xt = xn;
  }
  if (live && r == 0) lens[n] = len;
}

template <int H>
__global__ __launch_bounds__(SeqCfg<H>::BT) void lstm_seq_bwd_kernel(const float* __restrict__ x, const float* __restrict__ wih,
                                                                     const float* __restrict__ whh, const float* __restrict__ bih,
                                                                     const float* __restrict__ bhh, const float* __restrict__ hs,
                                                                     const float* __restrict__ cs, const int* __restrict__ lens,
                                                                     const float* __restrict__ dhs, float* __restrict__ part_hh,
                                                                     float* __restrict__ part_ih, float* __restrict__ part_b, int N,
                                                                     int T, int Q, int groups) {
  constexpr int TPS = SeqCfg<H>::TPS, SPB = SeqCfg<H>::SPB;
  __shared__ __attribute__((aligned(16))) float dzbuf[2][SPB][4][H];
  const int tid = threadIdx.x;
  const bool lane_ok = tid < SPB * TPS;
  const int sub = lane_ok ? tid / TPS : 0, r = tid % TPS;
  const int j = r >> 2, g = r & 3, row = g * H + j;
  const int grp = blockIdx.x * SPB + sub;
  float w[H], wc[H], acc[H];
#pragma unroll
  for (int k = 0; k < H; k += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(whh + (size_t)row * H + k);
    w[k] = v[0]; w[k + 1] = v[1]; w[k + 2] = v[2]; w[k + 3] = v[3];
  }
#pragma unroll
  for (int k = 0; k < H; ++k) {
    wc[k] = whh[(size_t)(g * H + k) * H + j];
    acc[k] = 0.f;
  }
  const float wx = wih[row], b = bih[row] + bhh[row];
  float aih = 0.f, ab = 0.f;
  int it = 0;
  for (int q = 0; q < Q; ++q) {
    const int n = grp * Q + q;
    const bool seq_ok = grp < groups && n < N;          // uniform over the sequence's lanes (spare lanes included)
    const int nn = seq_ok ? n : 0;
    const int len = seq_ok ? min(max(lens[nn], 0), T) : 0;
    const int tstart = SPB == 1 ? len - 1 : T - 1;        // block-uniform trip count
    const float* xr = x + (size_t)nn * T;
    const float* hr = hs + (size_t)nn * T * H;
    const float* cr = cs + (size_t)nn * T * H + j;
    const float* dr = dhs + (size_t)nn * T * H + j;
    float dh_rec = 0.f, dc_next = 0.f;
    // operands of step t, loaded one step ahead
    float hp[H], xt = 0.f, ct = 0.f, dht = 0.f;
    auto load_h = [&](int t) {
#pragma unroll
      for (int k = 0; k < H; k += 4) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t > 0) v = *reinterpret_cast<const f32x4*>(hr + (size_t)(t - 1) * H + k);
        hp[k] = v[0]; hp[k + 1] = v[1]; hp[k + 2] = v[2]; hp[k + 3] = v[3];
      }
    };
    const int t0 = len - 1;
    if (t0 >= 0) {
      load_h(t0);
      xt = xr[t0];
      ct = cr[(size_t)t0 * H];
      dht = dr[(size_t)t0 * H];
    }
    for (int t = tstart; t >= 0; --t) {
      const bool run = t < len;
      if (run) {
        const float cp = t > 0 ? cr[(size_t)(t - 1) * H] : 0.f;
        const float a = gate_act(gate_z<H>(w, hp, wx, xt, b), g == 2);
        const float ai = quad_bcast<0>(a), af = quad_bcast<1>(a), ag = quad_bcast<2>(a), ao = quad_bcast<3>(a);
        const float tc = gate_act(ct, true);
        const float dh = dht + dh_rec;
        const float dc = fmaf(dh * ao, 1.f - tc * tc, dc_next);
        const float dz = g == 0 ? dc * ag * ai * (1.f - ai)
                       : g == 1 ? dc * cp * af * (1.f - af)
                       : g == 2 ? dc * ai * (1.f - ag * ag)
                                : dh * tc * ao * (1.f - ao);
        dc_next = dc * af;
#pragma unroll
        for (int k = 0; k < H; ++k) acc[k] = fmaf(dz, hp[k], acc[k]);
        aih = fmaf(dz, xt, aih);
        ab += dz;
        if (lane_ok) dzbuf[it & 1][sub][g][j] = dz;
        // the next step's operands
        ct = cp;
        if (t > 0) {
          load_h(t - 1);
          xt = xr[t - 1];
          dht = dr[(size_t)(t - 1) * H];
        }
      }
      __syncthreads();
      if (run) {
        const float* dzv = dzbuf[it & 1][sub][g];
        float p = 0.f;
#pragma unroll
        for (int k = 0; k < H; k += 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(dzv + k);
          p = fmaf(wc[k], v[0], p);
          p = fmaf(wc[k + 1], v[1], p);
          p = fmaf(wc[k + 2], v[2], p);
          p = fmaf(wc[k + 3], v[3], p);
        }
        dh_rec = (quad_bcast<0>(p) + quad_bcast<1>(p)) + (quad_bcast<2>(p) + quad_bcast<3>(p));
      }
      ++it;
    }
  }
  if (lane_ok && grp < groups) {
    float* o = part_hh + ((size_t)grp * 4 * H + row) * H;
#pragma unroll
    for (int k = 0; k < H; k += 4) *reinterpret_cast<f32x4*>(o + k) = f32x4{acc[k], acc[k + 1], acc[k + 2], acc[k + 3]};
    part_ih[(size_t)grp * 4 * H + row] = aih;
    part_b[(size_t)grp * 4 * H + row] = ab;
  }
}

// ---- breath projection Linear(K = T H -> F) over the N rows: a skinny-N GEMM (F = 16 or 64 outputs) --------------------------
// forward: a block takes PROJ_RT rows and 16 outputs; thread `tid` walks the float4 columns tid, tid + 256, ...; the 64 sums
// are folded over the wave (wave_sum) and over the four waves in wave order.
#define PROJ_RT 4
__global__ __launch_bounds__(256) void seq_proj_fwd_kernel(const float* __restrict__ hs, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ y, int N, int K,
                                                           int F) {
  __shared__ float red[4][PROJ_RT * 16];
  const int n0 = blockIdx.x * PROJ_RT, f0 = blockIdx.y * 16;
  float acc[PROJ_RT][16];
#pragma unroll
  for (int i = 0; i < PROJ_RT; ++i)
#pragma unroll
    for (int f = 0; f < 16; ++f) acc[i][f] = 0.f;
  const int K4 = K >> 2;
  for (int k4 = threadIdx.x; k4 < K4; k4 += 256) {
    f32x4 a[PROJ_RT];
#pragma unroll
    for (int i = 0; i < PROJ_RT; ++i) {
      const int n = n0 + i < N ? n0 + i : N - 1;
      a[i] = *reinterpret_cast<const f32x4*>(hs + (size_t)n * K + 4 * k4);
    }
#pragma unroll
    for (int f = 0; f < 16; ++f) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(W + (size_t)(f0 + f) * K + 4 * k4);
#pragma unroll
      for (int i = 0; i < PROJ_RT; ++i)
        acc[i][f] = fmaf(a[i][3], wv[3], fmaf(a[i][2], wv[2], fmaf(a[i][1], wv[1], fmaf(a[i][0], wv[0], acc[i][f]))));
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < PROJ_RT; ++i)
#pragma unroll
    for (int f = 0; f < 16; ++f) {
      const float s = wave_sum(acc[i][f]);
      if (lane == 0) red[wave][i * 16 + f] = s;
    }
  __syncthreads();
  if (threadIdx.x < PROJ_RT * 16) {
    const int i = threadIdx.x >> 4, f = threadIdx.x & 15;
    if (n0 + i < N)
      y[(size_t)(n0 + i) * F + f0 + f] =
          ((red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x])) + bias[f0 + f];
  }
}

// dhs[n][k] = sum_f dy[n][f] W[f][k], f in order
__global__ __launch_bounds__(256) void seq_proj_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ W,
                                                             float* __restrict__ dhs, int K, int F) {
  const int k4 = blockIdx.y * 256 + threadIdx.x, n = blockIdx.x;
  if (k4 >= (K >> 2)) return;
  const float* d = dy + (size_t)n * F;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int f = 0; f < F; ++f) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(W + (size_t)f * K + 4 * k4);
    const float v = d[f];
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = fmaf(v, wv[e], s[e]);
  }
  *reinterpret_cast<f32x4*>(dhs + (size_t)n * K + 4 * k4) = s;
}

// dW partials: part[chunk][f][k] = sum over the chunk's PROJ_RC rows (in row order) of dy[n][f] hs[n][k]
#define PROJ_RC 32
__global__ __launch_bounds__(256) void seq_proj_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ hs,
                                                             float* __restrict__ part, int N, int K, int F) {
  const int k4 = blockIdx.x * 256 + threadIdx.x, chunk = blockIdx.y, f0 = blockIdx.z * 16;
  if (k4 >= (K >> 2)) return;
  f32x4 acc[16];
#pragma unroll
  for (int f = 0; f < 16; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int n1 = min(N, (chunk + 1) * PROJ_RC);
  for (int n = chunk * PROJ_RC; n < n1; ++n) {
    const f32x4 hv = *reinterpret_cast<const f32x4*>(hs + (size_t)n * K + 4 * k4);
    const float* d = dy + (size_t)n * F + f0;
#pragma unroll
    for (int f = 0; f < 16; ++f) {
      const float v = d[f];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[f][e] = fmaf(v, hv[e], acc[f][e]);
    }
  }
#pragma unroll
  for (int f = 0; f < 16; ++f)
    *reinterpret_cast<f32x4*>(part + ((size_t)chunk * F + f0 + f) * K + 4 * k4) = acc[f];
}

static inline bool seq_shape_ok(int N, int T, int H) { return N >= 0 && T >= 1 && H >= 8 && H <= 64 && H % 8 == 0; }
static inline bool proj_shape_ok(int N, int K, int F) { return N >= 0 && K >= 4 && K % 4 == 0 && F >= 16 && F <= 64 && F % 16 == 0; }
// sequences one backward block runs one after the other: keeps the partial rows near 2 048 however large N is
static inline int seq_bwd_q(int N) { return N <= 2048 ? 1 : (N + 2047) / 2048; }

#define SEQ_DISPATCH(STMT)              \
  switch (H) {                          \
    case 8: { constexpr int HH = 8; STMT; } break;    \
    case 16: { constexpr int HH = 16; STMT; } break;  \
    case 24: { constexpr int HH = 24; STMT; } break;  \
    case 32: { constexpr int HH = 32; STMT; } break;  \
    case 40: { constexpr int HH = 40; STMT; } break;  \
    case 48: { constexpr int HH = 48; STMT; } break;  \
    case 56: { constexpr int HH = 56; STMT; } break;  \
    default: { constexpr int HH = 64; STMT; } break;  \
  }

extern "C" {

// sequences a forward block works on at hidden size H (2 at H = 8, else 1); -1 for a refused H
int da_lstm_seq_block_seqs(int H) {
  if (!seq_shape_ok(0, 1, H)) return DA_EINVAL;
  return H == 8 ? 2 : 1;
}

int da_lstm_seq_fwd(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int packed,
                    float* hs, float* cs, int* lens, int N, int T, int H, hipStream_t stream) {
  DA_ENTER();
  if (!x || !w_ih || !w_hh || !b_ih || !b_hh || !hs || !cs || !lens || !seq_shape_ok(N, T, H) || (packed != 0 && packed != 1))
    return DA_EINVAL;
  if (N == 0) return DA_OK;
  SEQ_DISPATCH(hipLaunchKernelGGL(lstm_seq_fwd_kernel<HH>, dim3((N + SeqCfg<HH>::SPB - 1) / SeqCfg<HH>::SPB),
                                  dim3(SeqCfg<HH>::BT), 0, stream, x, w_ih, w_hh, b_ih, b_hh, hs, cs, lens, N, T, packed));
  DA_CHECK_LAUNCH();
  return DA_OK;
}

size_t da_lstm_seq_bwd_workspace(int N, int H) {
  if (!seq_shape_ok(N, 1, H)) return 0;
  const int q = seq_bwd_q(N), groups = (N + q - 1) / q;
  return (size_t)groups * 4 * H * (H + 2) * sizeof(float);
}

int da_lstm_seq_bwd(const float* dhs, const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                    const float* hs, const float* cs, const int* lens, float* dw_ih, float* dw_hh, float* db, float* db2,
                    float* workspace, int accumulate, int N, int T, int H, hipStream_t stream) {
  DA_ENTER();
  if (!dhs || !x || !w_ih || !w_hh || !b_ih || !b_hh || !hs || !cs || !lens || !dw_ih || !dw_hh || !db || !seq_shape_ok(N, T, H) ||
      (N > 0 && !workspace))
    return DA_EINVAL;
  const int G4 = 4 * H;
  if (N == 0) {
    if (!accumulate) {
      hipError_t e = hipMemsetAsync(dw_ih, 0, G4 * sizeof(float), stream);
      if (e == hipSuccess) e = hipMemsetAsync(dw_hh, 0, (size_t)G4 * H * sizeof(float), stream);
      if (e == hipSuccess) e = hipMemsetAsync(db, 0, G4 * sizeof(float), stream);
      if (e == hipSuccess && db2) e = hipMemsetAsync(db2, 0, G4 * sizeof(float), stream);
      if (e != hipSuccess) return (int)e;
    }
    return DA_OK;
  }
  const int q = seq_bwd_q(N), groups = (N + q - 1) / q;
  float* part_hh = workspace;
  float* part_ih = part_hh + (size_t)groups * G4 * H;
  float* part_b = part_ih + (size_t)groups * G4;
  SEQ_DISPATCH(hipLaunchKernelGGL(lstm_seq_bwd_kernel<HH>, dim3((groups + SeqCfg<HH>::SPB - 1) / SeqCfg<HH>::SPB),
                                  dim3(SeqCfg<HH>::BT), 0, stream, x, w_ih, w_hh, b_ih, b_hh, hs, cs, lens, dhs, part_hh, part_ih,
                                  part_b, N, T, q, groups));
  DA_CHECK_LAUNCH();
  int rc = da_reduce_rows(part_hh, groups, G4 * H, dw_hh, accumulate, stream);
  if (rc == DA_OK) rc = da_reduce_rows(part_ih, groups, G4, dw_ih, accumulate, stream);
  if (rc == DA_OK) rc = da_reduce_rows(part_b, groups, G4, db, accumulate, stream);
  if (rc == DA_OK && db2) rc = da_reduce_rows(part_b, groups, G4, db2, accumulate, stream);
  return rc;
}

int da_lstm_seq_proj_fwd(const float* hs, const float* W, const float* bias, float* y, int N, int K, int F, hipStream_t stream) {
  DA_ENTER();
  if (!hs || !W || !bias || !y || !proj_shape_ok(N, K, F)) return DA_EINVAL;
  if (N == 0) return DA_OK;
  hipLaunchKernelGGL(seq_proj_fwd_kernel, dim3((N + PROJ_RT - 1) / PROJ_RT, F / 16), dim3(256), 0, stream, hs, W, bias, y, N, K, F);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

size_t da_lstm_seq_proj_bwd_workspace(int N, int K, int F) {
  if (!proj_shape_ok(N, K, F)) return 0;
  return (size_t)((N + PROJ_RC - 1) / PROJ_RC) * F * K * sizeof(float);
}

int da_lstm_seq_proj_bwd(const float* dy, const float* hs, const float* W, float* dhs, float* dW, float* dbias, float* workspace,
                         int accumulate, int N, int K, int F, hipStream_t stream) {
  DA_ENTER();
  if (!dy || !hs || !W || !dhs || !dW || !dbias || !proj_shape_ok(N, K, F) || (N > 0 && !workspace)) return DA_EINVAL;
  if (N == 0) {
    if (!accumulate) {
      hipError_t e = hipMemsetAsync(dW, 0, (size_t)F * K * sizeof(float), stream);
      if (e == hipSuccess) e = hipMemsetAsync(dbias, 0, F * sizeof(float), stream);
      if (e != hipSuccess) return (int)e;
    }
    return DA_OK;
  }
  const int kb = ((K >> 2) + 255) / 256, chunks = (N + PROJ_RC - 1) / PROJ_RC;
  hipLaunchKernelGGL(seq_proj_dgrad_kernel, dim3(N, kb), dim3(256), 0, stream, dy, W, dhs, K, F);
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(seq_proj_wgrad_kernel, dim3(kb, chunks, F / 16), dim3(256), 0, stream, dy, hs, workspace, N, K, F);
  DA_CHECK_LAUNCH();
  int rc = da_reduce_rows(workspace, chunks, F * K, dW, accumulate, stream);
  if (rc == DA_OK) rc = da_reduce_rows(dy, N, F, dbias, accumulate, stream);
  return rc;
}

}  // extern "C"
