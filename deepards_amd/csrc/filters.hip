// Frequency filters of the batch path (reference deepards/dataset.py:546-557 setup_butter_filter, :1381-1400 __getitem__):
// behind (data - mu) / std the reference runs a 10th-order Butterworth sosfilt and an FFT band mask over every row of every
// item, on the host, in float64.  Both are linear maps on one length-L row, so the batch gather applies them as two short
// float64 sums per output sample:
//
//   y[n] = sum_{m <= n} h[n - m] x[m]              h = the first L samples of the cascade's impulse response (sosfilt from a
//                                                  zero state over a finite row is exactly this causal convolution)
//   z[n] = sum_m g[(n - m) mod L] y[m]             g = real(ifft(mask)), L = 224 (the mask is symmetric in |f|: z is real)
//
// gather_normalize_filter_kernel: one workgroup per row (B NB C rows).  The normalised row, h and g sit in LDS; thread n owns
// output n (and n + 256 when L > 256).  Both sums run in ascending m with fma in float64 into ONE accumulator: a fixed order, no
// atomics, a repeat is bit-identical.  With h = delta or g = delta every term but one is an exact zero, so the stage returns
// its input bit for bit.
//
// gather_normalize_chain_kernel: the whole item chain of dataset.py:1375-1400 -- the padded normalisation (mu is subtracted
// only where the raw sample is non-zero, :1406-1409), the causal stage, post-hoc downsampling (:1384-1391) and the circular
// stage.  scipy.signal.resample to new_len samples is a linear map too:
//
//   r[n] = sum_m R[n][m] y[m]  (n < new_len),  r[n] = 0  (new_len <= n < L)        R built on the host (filters.resample_matrix)
//
// R (up to 512 x 512 doubles) does not fit in LDS beside the rows and is read through L2, stored TRANSPOSED ([L][new_len]) so
// that the threads of a wave read consecutive doubles.  One workgroup takes FLT_CHAIN_ROWS rows, one accumulator per row in
// registers: every stage reads its kernel (h, R, g) once per group of rows instead of once per row.  Each row's sums keep the
// order of gather_normalize_filter_kernel: without R and with padded = 0 the results have that kernel's bits.
#include "common.h"
#include <limits.h>

#define FLT_THREADS 256
#define FLT_MAX_L 512                  // causal stage: up to the C5 tile shape
#define FLT_FFT_L 224                  // circular stage: the reference's mask is built over fftfreq(224) (dataset.py:1394)
#define FLT_R_AHEAD 16                 // values of R a thread of the chain kernel keeps in flight
#define FLT_CHAIN_ROWS 2               // rows per workgroup of the chain kernel (DESIGN_APPENDIX.md: measured against 1, 4, 8)

struct FilterFactors {                 // per-channel scaling factors (dataset.py:627-649), C <= 4
  double mu[4];
  double stdv[4];
};

__global__ __launch_bounds__(FLT_THREADS) void gather_normalize_filter_kernel(
    const double* __restrict__ tiles, const int64_t* __restrict__ idx, FilterFactors f, const double* __restrict__ h,
    const double* __restrict__ g, float* __restrict__ out, int NBC, int C, int L) {
  __shared__ double xs[FLT_MAX_L];     // the normalised row
  __shared__ double ys[FLT_MAX_L];     // behind the causal stage
  __shared__ double hs[FLT_MAX_L];
  __shared__ double gs[FLT_FFT_L];
  const int row = blockIdx.x;
  const int b = row / NBC, w = row - b * NBC, c = w % C;
  const double* src = tiles + ((size_t)idx[b] * NBC + w) * L;
  float* dst = out + (size_t)row * L;
  const double mu = f.mu[c], stdv = f.stdv[c];
  for (int i = threadIdx.x; i < L; i += FLT_THREADS) {
    xs[i] = (src[i] - mu) / stdv;      // the expression of gather_normalize_kernel: same bits
    if (h) hs[i] = h[i];
    if (g) gs[i] = g[i];               // (g != null only with L == FLT_FFT_L: checked by the entry point)
  }
  __syncthreads();
  const double* y = xs;
  if (h) {
    for (int n = threadIdx.x; n < L; n += FLT_THREADS) {
      double acc = 0.0;
      for (int m = 0; m <= n; ++m) acc = fma(hs[n - m], xs[m], acc);
      if (g) ys[n] = acc;
      else dst[n] = (float)acc;
    }
    if (!g) return;
    __syncthreads();
    y = ys;
  }
  for (int n = threadIdx.x; n < L; n += FLT_THREADS) {
    double acc = 0.0;
    int k = n;                         // (n - m) mod L, walked down with m
    for (int m = 0; m < L; ++m) {
      acc = fma(gs[k], y[m], acc);
      k = k == 0 ? L - 1 : k - 1;
    }
    dst[n] = (float)acc;
  }
}

__global__ __launch_bounds__(FLT_THREADS) void gather_normalize_chain_kernel(
    const double* __restrict__ tiles, const int64_t* __restrict__ idx, FilterFactors f, int padded, const double* __restrict__ h,
    const double* __restrict__ rt, int new_len, const double* __restrict__ g, float* __restrict__ out, int rows, int NBC, int C,
    int L) {
  constexpr int G = FLT_CHAIN_ROWS;
  __shared__ double bufs[2][G][FLT_MAX_L];   // a stage reads one and writes the other
  __shared__ double hs[FLT_MAX_L];
  __shared__ double gs[FLT_FFT_L];
  static_assert(sizeof(bufs) + sizeof(hs) + sizeof(gs) <= 64 * 1024, "static LDS of the chain kernel");
  const int row0 = blockIdx.x * G;
  double (*cur)[FLT_MAX_L] = bufs[0];
  double (*nxt)[FLT_MAX_L] = bufs[1];
  for (int q = 0; q < G; ++q) {
    const int row = row0 + q;
    if (row >= rows) {                   // the last group may be short: its spare rows are zeros and are never stored
      for (int i = threadIdx.x; i < L; i += FLT_THREADS) cur[q][i] = 0.0;
      continue;
    }
    const int b = row / NBC, w = row - b * NBC, c = w % C;
    const double* src = tiles + ((size_t)idx[b] * NBC + w) * L;
    const double mu = f.mu[c], stdv = f.stdv[c];
    for (int i = threadIdx.x; i < L; i += FLT_THREADS) {
      const double x = src[i];
      // padded: (x - where(x != 0, mu, 0)) / std -- a NaN counts as non-zero; unpadded: gather_normalize_kernel's expression
      cur[q][i] = (!padded || x != 0.0) ? (x - mu) / stdv : x / stdv;
    }
  }
  for (int i = threadIdx.x; i < L; i += FLT_THREADS) {
    if (h) hs[i] = h[i];
    if (g) gs[i] = g[i];                 // (g != null only with L == FLT_FFT_L: checked by the entry point)
  }
  __syncthreads();
  if (h) {
    for (int n = threadIdx.x; n < L; n += FLT_THREADS) {
      double acc[G];
#pragma unroll
      for (int q = 0; q < G; ++q) acc[q] = 0.0;
      for (int m = 0; m <= n; ++m) {
        const double hv = hs[n - m];
#pragma unroll
        for (int q = 0; q < G; ++q) acc[q] = fma(hv, cur[q][m], acc[q]);
      }
#pragma unroll
      for (int q = 0; q < G; ++q) nxt[q][n] = acc[q];
    }
    __syncthreads();
    double (*t)[FLT_MAX_L] = cur; cur = nxt; nxt = t;
  }
  if (rt) {
    for (int n = threadIdx.x; n < L; n += FLT_THREADS) {
      double acc[G];
#pragma unroll
      for (int q = 0; q < G; ++q) acc[q] = 0.0;
      if (n < new_len) {
        // R[n][m] = rt[m * new_len + n]: consecutive threads, consecutive doubles.  The sum is one dependent chain per output,
        // so the loads must not wait in it: the next FLT_R_AHEAD values of the column are fetched while these are summed.
        const double* col = rt + n;
        double rv[FLT_R_AHEAD], nx[FLT_R_AHEAD];
#pragma unroll
        for (int u = 0; u < FLT_R_AHEAD; ++u) rv[u] = u < L ? col[(size_t)u * new_len] : 0.0;
        for (int m0 = 0; m0 < L; m0 += FLT_R_AHEAD) {
#pragma unroll
          for (int u = 0; u < FLT_R_AHEAD; ++u) {
            const int m = m0 + FLT_R_AHEAD + u;
            nx[u] = m < L ? col[(size_t)m * new_len] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < FLT_R_AHEAD; ++u) {
            const int m = m0 + u;        // ascending m, as everywhere; nothing is added for m >= L
            if (m < L) {
#pragma unroll
              for (int q = 0; q < G; ++q) acc[q] = fma(rv[u], cur[q][m], acc[q]);
            }
            rv[u] = nx[u];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < G; ++q) nxt[q][n] = acc[q];      // (zeros behind new_len: np.pad at the end of the row)
    }
    __syncthreads();
    double (*t)[FLT_MAX_L] = cur; cur = nxt; nxt = t;
  }
  if (g) {
    for (int n = threadIdx.x; n < L; n += FLT_THREADS) {
      double acc[G];
#pragma unroll
      for (int q = 0; q < G; ++q) acc[q] = 0.0;
      int k = n;                         // (n - m) mod L, walked down with m
      for (int m = 0; m < L; ++m) {
        const double gv = gs[k];
#pragma unroll
        for (int q = 0; q < G; ++q) acc[q] = fma(gv, cur[q][m], acc[q]);
        k = k == 0 ? L - 1 : k - 1;
      }
#pragma unroll
      for (int q = 0; q < G; ++q) nxt[q][n] = acc[q];
    }
    __syncthreads();
    cur = nxt;
  }
  for (int q = 0; q < G && row0 + q < rows; ++q) {
    float* dst = out + (size_t)(row0 + q) * L;
    for (int i = threadIdx.x; i < L; i += FLT_THREADS) dst[i] = (float)cur[q][i];
  }
}

extern "C" {

// tiles: [N][NB][C][L] float64 raw windows; idx: [B] int64; mu / stdv: HOST arrays [C]; h, g: DEVICE arrays of L doubles,
// either may be null, not both; out: [B][NB][C][L] float32.  h needs L <= 512, g needs L == 224: anything else returns -1
// before a launch, out untouched.
int da_gather_normalize_filter(const double* tiles, const int64_t* idx, const double* mu, const double* stdv, const double* h,
                               const double* g, float* out, int B, int NB, int C, int L, hipStream_t stream) {
  DA_ENTER();
  if (!tiles || !idx || !out || !mu || !stdv || (!h && !g) || B < 0 || NB < 1 || C < 1 || C > 4 || L < 1) return DA_EINVAL;
  if (L > FLT_MAX_L || (g && L != FLT_FFT_L)) return DA_EINVAL;
  if ((long long)B * NB * C > INT_MAX) return DA_EINVAL;
  FilterFactors f;
  for (int c = 0; c < 4; ++c) {
    f.mu[c] = c < C ? mu[c] : 0.0;
    f.stdv[c] = c < C ? stdv[c] : 1.0;
    if (f.stdv[c] == 0.0) return DA_EINVAL;
  }
  if (B == 0) return DA_OK;
  hipLaunchKernelGGL(gather_normalize_filter_kernel, dim3(B * NB * C), dim3(FLT_THREADS), 0, stream, tiles, idx, f, h, g, out,
                     NB * C, C, L);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

// The whole item chain (dataset.py:1375-1400) for every (b, nb, c) row, in float64, then the cast.  padded != 0: mu is
// subtracted only from non-zero samples (padded_breath_by_breath datasets).  h, rt, g: DEVICE arrays, each may be null (a stage
// that is absent), all three too.  rt: [L][new_len] doubles, the TRANSPOSE of the (new_len, L) resampling matrix; without it
// new_len must be 0, with it 1 <= new_len <= L.  L <= 512 always, g needs L == 224: anything else returns -1 before a launch,
// out untouched.
int da_gather_normalize_chain(const double* tiles, const int64_t* idx, const double* mu, const double* stdv, int padded,
                              const double* h, const double* rt, int new_len, const double* g, float* out, int B, int NB, int C,
                              int L, hipStream_t stream) {
  DA_ENTER();
  if (!tiles || !idx || !out || !mu || !stdv || B < 0 || NB < 1 || C < 1 || C > 4 || L < 1) return DA_EINVAL;
  if (L > FLT_MAX_L || (g && L != FLT_FFT_L)) return DA_EINVAL;
  if (rt ? (new_len < 1 || new_len > L) : new_len != 0) return DA_EINVAL;
  if ((long long)B * NB * C > INT_MAX) return DA_EINVAL;
  FilterFactors f;
  for (int c = 0; c < 4; ++c) {
    f.mu[c] = c < C ? mu[c] : 0.0;
    f.stdv[c] = c < C ? stdv[c] : 1.0;
    if (f.stdv[c] == 0.0) return DA_EINVAL;
  }
  if (B == 0) return DA_OK;
  const int rows = B * NB * C;
  hipLaunchKernelGGL(gather_normalize_chain_kernel, dim3((rows + FLT_CHAIN_ROWS - 1) / FLT_CHAIN_ROWS), dim3(FLT_THREADS), 0,
                     stream, tiles, idx, f, padded != 0, h, rt, new_len, g, out, rows, NB * C, C, L);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
