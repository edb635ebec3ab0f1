// The head of the 1-D ProtoPNet (reference models/protopnet1d/model.py:113-354 PPNet; train_ards_detector.py:1194-1247
// ProtoPNetModel.calc_loss) behind the breath block's map z [rows][L][C] (channels innermost, rows = B NB):
//
//   add-on layers   Conv1d(k = 1) + bias -> ReLU | Sigmoid (:159-185).  The 1x1 convolutions run on the GEMM conv path
//                   (conv_gemm.hip); da_bias_act_fwd / da_bias_act_bwd are the bias, the activation and their backward.
//   prototype layer da_proto_fwd: d[row][p][l] = sum_c (z[row][l][c] - protos[p][c])^2 (:217-242 _l2_convolution), the global
//                   min-pool over l with its arg-min (:263) and sim = log((min_d + 1) / (min_d + 1e-4)) (:254);
//                   da_proto_bwd: the gradients on z and on the prototypes.
//   loss            da_ppnet_loss: cross entropy + cluster + separation cost and their gradients in one launch.
//
// The distance is taken in the DIRECT form.  The reference expands it, relu(sum z^2 - 2 sum z p + sum p^2); the two agree in
// exact arithmetic, but the direct form is a sum of squares -- never negative (the ReLU is vacuous), and EXACTLY 0 where a
// prototype is bitwise a patch of the map (every pushed prototype on its source window), where the expanded form leaves
// rounding noise that the log similarity amplifies by 1 / (d + 1e-4).
//
// Summation order (no atomics anywhere: the same operands give the same bits on every run, and a row's outputs do not depend
// on the rows around it):
//   d        four chains, chain e over the channels e, e + 4, e + 8, ... ascending (fmaf from zero), then (a0 + a1) + (a2 + a3)
//   db       rows m = s, s + 8, ... of a tile of 64 positions in slot s, the 8 slots in order, the tiles in order (da_reduce_rows)
//   dz       the prototypes p = 0, 1, ... whose arg-min is this position, ascending (fmaf from zero)
//   dprotos  rows r = s, s + 8, ... of a chunk of 64 rows in slot s, the 8 slots in order, the chunks in order (da_reduce_rows)
//   loss     a wave per window b = w, w + 16, ...; the maxima by a butterfly on (value, lowest index); the 16 waves in order
#include "common.h"

extern "C" int da_reduce_rows(const float* m, int rows, int n, float* out, int accumulate, hipStream_t stream);   // head_optim.hip

#define PP_RELU 0
#define PP_SIGMOID 1
#define PP_EPS 1e-4                 // PPNet.epsilon (model.py:124)

#define BA_ROWS 64                  // positions of one block of the bias / activation backward
#define BA_CC 128                   // its channels (32 lanes x 4)
#define BA_MAX_N 4096

#define PF_DC 64                    // channels staged per pass of the distance kernel
#define PF_LDQ (PF_DC / 4 + 1)      // quads of one staged row (+ 1: rows of different prototypes fall on different banks)
#define PF_MAX_P 64
#define PF_MAX_L 64
#define PF_MAX_D 512
#define PF_ZPOS 128                 // map positions (rows of the tile x L) staged per pass
#define PF_ITEMS 16                 // (row, p, l) distances of one thread
#define PF_RT 4                     // rows of a tile at the small shapes
#define PB_ROWS 64                  // rows of one chunk of the prototype gradient

// ---------------------------------------------------------------------------------------------------------------------
// y[m][n] = act(x[m][n] + b[n])
// ---------------------------------------------------------------------------------------------------------------------
template <int ACT>
__global__ __launch_bounds__(256) void bias_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ b,
                                                           float* __restrict__ y, size_t nquad, int nq) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nquad) return;
  const int q = (int)(i % (size_t)nq);
  const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
  const f32x4 bb = *reinterpret_cast<const f32x4*>(b + (size_t)q * 4);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float s = v[e] + bb[e];
    o[e] = ACT == PP_RELU ? (s < 0.f ? 0.f : s) : 1.0f / (1.0f + expf(-s));     // (a NaN stays a NaN)
  }
  *reinterpret_cast<f32x4*>(y + i * 4) = o;
}

// dx = dy act'(y) from the stored output; the block's column sums of dx -> part[tile][n] (the bias gradient's partials)
template <int ACT>
__global__ __launch_bounds__(256) void bias_act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                           float* __restrict__ dx, float* __restrict__ part, int M, int N) {
  __shared__ f32x4 red[8][32];
  const int ql = threadIdx.x & 31, slot = threadIdx.x >> 5;
  const int c = blockIdx.y * BA_CC + ql * 4;
  const bool live = c < N;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (live) {
#pragma unroll
    for (int i = 0; i < BA_ROWS / 8; ++i) {
      const int m = blockIdx.x * BA_ROWS + slot + 8 * i;
      if (m < M) {
        const size_t o = (size_t)m * N + c;
        const f32x4 g = *reinterpret_cast<const f32x4*>(dy + o);
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + o);
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = ACT == PP_RELU ? (v[e] > 0.f ? g[e] : 0.f) : g[e] * (v[e] * (1.0f - v[e]));
        if (dx) *reinterpret_cast<f32x4*>(dx + o) = d;
        acc += d;
      }
    }
  }
  if (!part) return;                                     // (uniform: a kernel argument)
  red[slot][ql] = acc;
  __syncthreads();
  if (slot == 0 && live) {
    for (int k = 1; k < 8; ++k) acc += red[k][ql];
    *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * N + c) = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The prototype layer, forward.  A block takes a tile of RT rows: per pass it stages PF_DC channels of the P prototypes and
// of the tile's positions in LDS, and thread i adds that pass's share to its distances i, i + 256, ... (item = (r P + p) L + l,
// the order of dist).  Then a thread per (row, p) takes the minimum over l (the lowest l attaining it) and the similarity.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ static inline int pf_row_tile(int L, int P) {
  int rt = PF_RT;
  if (rt > PF_ZPOS / L) rt = PF_ZPOS / L;
  if (rt > 256 * PF_ITEMS / (L * P)) rt = 256 * PF_ITEMS / (L * P);
  return rt < 1 ? 1 : rt;                                // L <= 64, L P <= 4096: one row always fits
}

__global__ __launch_bounds__(256) void proto_fwd_kernel(const float* __restrict__ z, const float* __restrict__ protos,
                                                        float* __restrict__ dist, float* __restrict__ min_d,
                                                        int* __restrict__ arg, float* __restrict__ sim, int rows, int L, int D,
                                                        int P, int RT) {
  __shared__ f32x4 sP[PF_MAX_P * PF_LDQ];                // 17 408 B
  __shared__ f32x4 sZ[PF_ZPOS * PF_LDQ];                 // 34 816 B; the finished distances of the tile afterwards
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * RT;
  const int nr = min(RT, rows - row0);
  const int npos = nr * L, nitems = nr * P * L;
  int zo[PF_ITEMS], po[PF_ITEMS];
  f32x4 acc[PF_ITEMS];
#pragma unroll
  for (int it = 0; it < PF_ITEMS; ++it) {
    const int item = tid + it * 256;
    zo[it] = po[it] = 0;
    acc[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (item < nitems) {
      const int r = item / (P * L), rem = item - r * P * L;
      const int p = rem / L, l = rem - p * L;
      zo[it] = (r * L + l) * PF_LDQ;
      po[it] = p * PF_LDQ;
    }
  }
  for (int c0 = 0; c0 < D; c0 += PF_DC) {
    const int nq = min(PF_DC, D - c0) >> 2;              // 8 or 16 quads (D % 32 == 0)
    for (int i = tid; i < P * nq; i += 256) {
      const int p = i / nq, q = i - p * nq;
      sP[p * PF_LDQ + q] = *reinterpret_cast<const f32x4*>(protos + (size_t)p * D + c0 + q * 4);
    }
    for (int i = tid; i < npos * nq; i += 256) {
      const int pos = i / nq, q = i - pos * nq;
      sZ[pos * PF_LDQ + q] = *reinterpret_cast<const f32x4*>(z + ((size_t)row0 * L + pos) * D + c0 + q * 4);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < PF_ITEMS; ++it) {
      if (tid + it * 256 < nitems) {
#pragma unroll 8
        for (int q = 0; q < nq; ++q) {
          const f32x4 d = sZ[zo[it] + q] - sP[po[it] + q];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[it][e] = fmaf(d[e], d[e], acc[it][e]);
        }
      }
    }
    __syncthreads();
  }
  float* sD = reinterpret_cast<float*>(sZ);              // nitems <= 4096 floats (every read of sZ is behind the last barrier)
#pragma unroll
  for (int it = 0; it < PF_ITEMS; ++it) {
    const int item = tid + it * 256;
    if (item < nitems) {
      const float d = (acc[it][0] + acc[it][1]) + (acc[it][2] + acc[it][3]);
      sD[item] = d;
      if (dist) dist[(size_t)row0 * P * L + item] = d;
    }
  }
  __syncthreads();
  for (int rp = tid; rp < nr * P; rp += 256) {
    const float* d = sD + (size_t)rp * L;
    float best = d[0];
    int at = 0;
    for (int l = 1; l < L; ++l) {
      const float v = d[l];
      if (v < best || (v != v && best == best)) {        // strict: the lowest l of a tie stays; a NaN wins, as in max_pool1d
        best = v;
        at = l;
      }
    }
    const size_t o = (size_t)row0 * P + rp;
    min_d[o] = best;
    arg[o] = at;
    // in double: rows P values, and log(1 / 1e-4) of a pushed prototype comes out correctly rounded
    sim[o] = (float)log(((double)best + 1.0) / ((double)best + PP_EPS));
  }
}

// g[row][p] = d loss / d min_d: the caller's gradient on min_d plus its gradient on sim through
// d sim / d min_d = 1 / (m + 1) - 1 / (m + eps) = -(1 - eps) / ((m + 1) (m + eps))
__device__ __forceinline__ float proto_g(const float* __restrict__ dsim, const float* __restrict__ dmin,
                                         const float* __restrict__ min_d, size_t o) {
  float g = dmin ? dmin[o] : 0.f;
  if (dsim) {
    const float m = min_d[o], eps = (float)PP_EPS;
    g = fmaf(dsim[o], -(1.0f - eps) / ((m + 1.0f) * (m + eps)), g);
  }
  return g;
}

// dz[row][l][c] = sum over the prototypes p with arg[row][p] == l of 2 g[row][p] (z - protos[p]); block = one row
__global__ __launch_bounds__(256) void proto_bwd_dz_kernel(const float* __restrict__ dsim, const float* __restrict__ dmin,
                                                           const float* __restrict__ min_d, const int* __restrict__ arg,
                                                           const float* __restrict__ z, const float* __restrict__ protos,
                                                           float* __restrict__ dz, int L, int D, int P) {
  __shared__ float sg[PF_MAX_P];
  __shared__ int sa[PF_MAX_P];
  const int row = blockIdx.x, tid = threadIdx.x;
  if (tid < P) {
    const size_t o = (size_t)row * P + tid;
    sg[tid] = 2.0f * proto_g(dsim, dmin, min_d, o);
    sa[tid] = arg[o];
  }
  __syncthreads();
  const int nq = D >> 2;
  for (int i = tid; i < L * nq; i += 256) {
    const int l = i / nq, q = i - l * nq;
    const size_t o = ((size_t)row * L + l) * D + q * 4;
    const f32x4 zv = *reinterpret_cast<const f32x4*>(z + o);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < P; ++p) {
      if (sa[p] == l) {
        const f32x4 pv = *reinterpret_cast<const f32x4*>(protos + (size_t)p * D + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(sg[p], zv[e] - pv[e], acc[e]);
      }
    }
    *reinterpret_cast<f32x4*>(dz + o) = acc;
  }
}

// part[chunk][p][c] = sum over the chunk's rows of 2 g[row][p] (protos[p][c] - z[row][arg[row][p]][c]);
// block = (prototype, chunk of PB_ROWS rows, 128 channels)
__global__ __launch_bounds__(256) void proto_bwd_dp_kernel(const float* __restrict__ dsim, const float* __restrict__ dmin,
                                                           const float* __restrict__ min_d, const int* __restrict__ arg,
                                                           const float* __restrict__ z, const float* __restrict__ protos,
                                                           float* __restrict__ part, int rows, int L, int D, int P) {
  __shared__ f32x4 red[8][32];
  const int p = blockIdx.x, chunk = blockIdx.y;
  const int ql = threadIdx.x & 31, slot = threadIdx.x >> 5;
  const int c = blockIdx.z * BA_CC + ql * 4;
  const bool live = c < D;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const f32x4 pv = *reinterpret_cast<const f32x4*>(protos + (size_t)p * D + c);
#pragma unroll
    for (int i = 0; i < PB_ROWS / 8; ++i) {
      const int r = chunk * PB_ROWS + slot + 8 * i;
      if (r < rows) {
        const size_t o = (size_t)r * P + p;
        const int a = arg[o];
        if ((unsigned)a < (unsigned)L) {                 // (an arg-min this library wrote always is)
          const float g2 = 2.0f * proto_g(dsim, dmin, min_d, o);
          const f32x4 zv = *reinterpret_cast<const f32x4*>(z + ((size_t)r * L + a) * D + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(g2, pv[e] - zv[e], acc[e]);
        }
      }
    }
  }
  red[slot][ql] = acc;
  __syncthreads();
  if (slot == 0 && live) {
    for (int k = 1; k < 8; ++k) acc += red[k][ql];
    *reinterpret_cast<f32x4*>(part + ((size_t)chunk * P + p) * D + c) = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// ProtoPNetModel.calc_loss (train_ards_detector.py:1194-1247) without the l1 term, and its gradients, in one launch of one
// block: wave w takes the windows w, w + 16, ..., its lanes the NB P distances of the window.  With s = softmax(logits):
//   cls        mean over [B][2] of -(t log s + (1 - t) log(1 - s)), the logs as a log-softmax (1 - s_c = s_{1-c}: no
//              cancellation) clamped at -100 as F.binary_cross_entropy clamps them;  with a_c = t_c + 1 - t_{1-c}
//              d cls / d logits[b][c] = (2 s_c - a_c) / (2 B)
//   label      argmax(target) (class 0 on a tie); correct[j] = ((j mod P) / (P / 2) == label)
//   cluster    mean_b(max_dist - max_j((max_dist - min_d[b][j]) correct[j])): the masked-out entries take part as zeros, so
//              a window whose correct entries are all negative (min_d > max_dist) has the maximum 0 and no gradient; the
//              maximum's gradient goes to the lowest index attaining it:  d / d min_d[b][j*] = correct[j*] / B
//   separation the same with 1 - correct;   total = cls + clust_lambda cluster + sep_lambda separation (a plus sign, as written)
// gscale multiplies the gradients only.  out[5] = total, cls, cluster, separation, 0 (the caller's l1 slot).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (v2 > v || (v2 == v && i2 < i)) {
      v = v2;
      i = i2;
    }
  }
}

__global__ __launch_bounds__(1024) void ppnet_loss_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                          const float* __restrict__ min_d, int B, int NB, int P,
                                                          float max_dist, float clust_lambda, float sep_lambda, float gscale,
                                                          float* __restrict__ out, float* __restrict__ dlogits,
                                                          float* __restrict__ dmin) {
  __shared__ float red[3][16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int K = NB * P, half = P >> 1;
  const float inv_b = 1.0f / (float)B;
  float s_cls = 0.f, s_clu = 0.f, s_sep = 0.f;             // lane 0 of the wave holds them
  for (int b = wave; b < B; b += 16) {
    const float t0 = target[(size_t)b * 2], t1 = target[(size_t)b * 2 + 1];
    const int label = t1 > t0 ? 1 : 0;
    const float* md = min_d + (size_t)b * K;
    float vc = -INFINITY, vs = -INFINITY;
    int ic = 0x7fffffff, is = 0x7fffffff;
    for (int j = lane; j < K; j += 64) {
      const bool corr = (j % P) / half == label;
      const float v = max_dist - md[j];
      const float c = corr ? v : 0.f, s = corr ? 0.f : v;
      if (c > vc) {
        vc = c;
        ic = j;
      }
      if (s > vs) {
        vs = s;
        is = j;
      }
    }
    wave_argmax(vc, ic);
    wave_argmax(vs, is);
    if (dmin) {
      float* dm = dmin + (size_t)b * K;
      for (int j = lane; j < K; j += 64) {
        const bool corr = (j % P) / half == label;
        float g = 0.f;
        if (j == ic && corr) g += clust_lambda;
        if (j == is && !corr) g += sep_lambda;
        dm[j] = g * inv_b * gscale;
      }
    }
    if (lane == 0) {
      s_clu += max_dist - vc;
      s_sep += max_dist - vs;
      const float x0 = logits[(size_t)b * 2], x1 = logits[(size_t)b * 2 + 1];
      const float d = x1 - x0, e = expf(-fabsf(d)), sp = log1pf(e);
      const bool up = d >= 0.f;                            // class 1 holds the larger logit
      const float ls_hi = fmaxf(-sp, -100.f), ls_lo = fmaxf(-fabsf(d) - sp, -100.f);
      const float p_lo = e / (1.0f + e);                   // the smaller of the two softmax probabilities
      const float ls0 = up ? ls_lo : ls_hi, ls1 = up ? ls_hi : ls_lo;
      const float a0 = t0 + (1.0f - t1), a1 = t1 + (1.0f - t0);
      s_cls -= a0 * ls0 + a1 * ls1;
      if (dlogits) {
        // 2 s_c - a_c = (s_c - t_c) - (s_{1-c} - t_{1-c}); both differences from the SMALLER probability, so that a
        // confident, correct window (s_c near t_c = 1) loses nothing to cancellation: s_hi - t_hi = (1 - t_hi) - s_lo
        const float t_hi = up ? t1 : t0, t_lo = up ? t0 : t1;
        const float u_hi = (1.0f - t_hi) - p_lo, u_lo = p_lo - t_lo;
        const float g_hi = (u_hi - u_lo) * (0.5f * inv_b) * gscale;
        dlogits[(size_t)b * 2] = up ? -g_hi : g_hi;
        dlogits[(size_t)b * 2 + 1] = up ? g_hi : -g_hi;
      }
    }
  }
  if (lane == 0) {
    red[0][wave] = s_cls;
    red[1][wave] = s_clu;
    red[2][wave] = s_sep;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, c = 0.f, s = 0.f;
    for (int k = 0; k < 16; ++k) {
      a += red[0][k];
      c += red[1][k];
      s += red[2][k];
    }
    const float cls = a * (0.5f * inv_b), clu = c * inv_b, sep = s * inv_b;
    out[0] = cls + clust_lambda * clu + sep_lambda * sep;
    out[1] = cls;
    out[2] = clu;
    out[3] = sep;
    out[4] = 0.f;
  }
}

// g += wd p: the L2 term torch.optim.Adam(weight_decay) adds to the gradient in front of its moments (da_clamp_adam has none;
// the ProtoPNet optimisers give Adam a weight decay on the breath block and the add-on layers, train_ards_detector.py:1163-1191)
__global__ __launch_bounds__(256) void grad_add_decay_kernel(float* __restrict__ g, const float* __restrict__ p, size_t n,
                                                             float wd) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) g[i] = fmaf(wd, p[i], g[i]);
}

static inline bool pp_proto_shape_ok(int rows, int L, int D, int P) {
  return rows >= 1 && L >= 1 && L <= PF_MAX_L && D >= 32 && D <= PF_MAX_D && D % 32 == 0 && P >= 2 && P <= PF_MAX_P &&
         (size_t)rows * L * D < ((size_t)1 << 31) && (size_t)rows * P * L < ((size_t)1 << 31);
}

static inline bool pp_ba_shape_ok(int M, int N, int act) {
  return M >= 1 && N >= 4 && N <= BA_MAX_N && N % 4 == 0 && (act == PP_RELU || act == PP_SIGMOID) &&
         (size_t)M * N < ((size_t)1 << 31);
}

extern "C" {

int da_bias_act_fwd(const float* x, const float* bias, float* y, int M, int N, int act, hipStream_t stream) {
  if (!x || !bias || !y || !pp_ba_shape_ok(M, N, act)) return DA_EINVAL;
  DA_ENTER();
  const size_t nquad = (size_t)M * (N / 4);
  const dim3 grid((unsigned)((nquad + 255) / 256)), block(256);
  if (act == PP_RELU)
    hipLaunchKernelGGL(bias_act_fwd_kernel<PP_RELU>, grid, block, 0, stream, x, bias, y, nquad, N / 4);
  else
    hipLaunchKernelGGL(bias_act_fwd_kernel<PP_SIGMOID>, grid, block, 0, stream, x, bias, y, nquad, N / 4);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

size_t da_bias_act_bwd_workspace(int M, int N) {
  if (M < 1 || N < 1) return 0;
  return (size_t)((M + BA_ROWS - 1) / BA_ROWS) * N * sizeof(float);
}

int da_bias_act_bwd(const float* dy, const float* y, float* dx, float* dbias, int accumulate, float* workspace, int M, int N,
                    int act, hipStream_t stream) {
  if (!dy || !y || (!dx && !dbias) || (dbias && !workspace) || !pp_ba_shape_ok(M, N, act)) return DA_EINVAL;
  DA_ENTER();
  const int tiles = (M + BA_ROWS - 1) / BA_ROWS;
  const dim3 grid((unsigned)tiles, (unsigned)((N + BA_CC - 1) / BA_CC)), block(256);
  float* part = dbias ? workspace : nullptr;
  if (act == PP_RELU)
    hipLaunchKernelGGL(bias_act_bwd_kernel<PP_RELU>, grid, block, 0, stream, dy, y, dx, part, M, N);
  else
    hipLaunchKernelGGL(bias_act_bwd_kernel<PP_SIGMOID>, grid, block, 0, stream, dy, y, dx, part, M, N);
  DA_CHECK_LAUNCH();
  if (dbias) return da_reduce_rows(part, tiles, N, dbias, accumulate, stream);
  return DA_OK;
}

int da_proto_shape_ok(int rows, int L, int D, int P) { return pp_proto_shape_ok(rows, L, D, P) ? 1 : 0; }

int da_proto_row_tile(int L, int P) {
  if (L < 1 || L > PF_MAX_L || P < 2 || P > PF_MAX_P) return 0;
  return pf_row_tile(L, P);
}

int da_proto_fwd(const float* z, const float* protos, float* dist, float* min_d, int* arg, float* sim, int rows, int L, int D,
                 int P, hipStream_t stream) {
  if (!z || !protos || !min_d || !arg || !sim || !pp_proto_shape_ok(rows, L, D, P)) return DA_EINVAL;
  DA_ENTER();
  const int rt = pf_row_tile(L, P);
  hipLaunchKernelGGL(proto_fwd_kernel, dim3((unsigned)((rows + rt - 1) / rt)), dim3(256), 0, stream, z, protos, dist, min_d, arg,
                     sim, rows, L, D, P, rt);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

size_t da_proto_bwd_workspace(int rows, int D, int P) {
  if (rows < 1 || D < 1 || P < 1) return 0;
  return (size_t)((rows + PB_ROWS - 1) / PB_ROWS) * P * D * sizeof(float);
}

int da_proto_bwd(const float* dsim, const float* dmin, const float* min_d, const int* arg, const float* z, const float* protos,
                 float* dz, float* dprotos, int accumulate, float* workspace, int rows, int L, int D, int P,
                 hipStream_t stream) {
  if ((!dsim && !dmin) || !min_d || !arg || !z || !protos || (!dz && !dprotos) || (dprotos && !workspace) ||
      !pp_proto_shape_ok(rows, L, D, P))
    return DA_EINVAL;
  DA_ENTER();
  if (dz) {
    hipLaunchKernelGGL(proto_bwd_dz_kernel, dim3((unsigned)rows), dim3(256), 0, stream, dsim, dmin, min_d, arg, z, protos, dz, L,
                       D, P);
    DA_CHECK_LAUNCH();
  }
  if (dprotos) {
    const int chunks = (rows + PB_ROWS - 1) / PB_ROWS;
    if (chunks > 65535) return DA_EINVAL;
    hipLaunchKernelGGL(proto_bwd_dp_kernel, dim3((unsigned)P, (unsigned)chunks, (unsigned)((D + BA_CC - 1) / BA_CC)), dim3(256), 0,
                       stream, dsim, dmin, min_d, arg, z, protos, workspace, rows, L, D, P);
    DA_CHECK_LAUNCH();
    return da_reduce_rows(workspace, chunks, P * D, dprotos, accumulate, stream);
  }
  return DA_OK;
}

int da_ppnet_loss(const float* logits, const float* target, const float* min_d, int B, int NB, int P, float max_dist,
                  float clust_lambda, float sep_lambda, float gscale, float* out, float* dlogits, float* dmin_d,
                  hipStream_t stream) {
  if (!logits || !target || !min_d || !out || B < 1 || NB < 1 || P < 2 || P > PF_MAX_P || P % 2 ||
      (size_t)B * NB * P >= ((size_t)1 << 31))
    return DA_EINVAL;
  DA_ENTER();
  hipLaunchKernelGGL(ppnet_loss_kernel, dim3(1), dim3(1024), 0, stream, logits, target, min_d, B, NB, P, max_dist, clust_lambda,
                     sep_lambda, gscale, out, dlogits, dmin_d);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_grad_add_decay(float* g, const float* p, size_t n, float weight_decay, hipStream_t stream) {
  if (!g || !p) return DA_EINVAL;
  if (n == 0) return DA_OK;
  DA_ENTER();
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(grad_add_decay_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, g, p, n,
                     weight_decay);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
