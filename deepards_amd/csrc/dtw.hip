// Dynamic time warping (reference dtw_lib.py: `from dtwco.warping.core import dtw` with its defaults, read from dtwco's
// documentation -- dtwco itself was never run against this): P independent pairs in one launch, and the ordered segment means
// both of dtw_lib's users take of the distances.
//
// For 1-D x (n >= 1) and y (m >= 1), in the accumulation type T (float or double), every line ONE IEEE operation:
//     c(i,j)  = |x[i] - y[j]|   (metric 0, 'euclidean')   |   (x[i] - y[j])^2   (metric 1; the product rounded on its own)
//     D(i,j)  = c(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1)),   D(-1,-1) = 0 and every other missing neighbour +inf
//     band k >= 0 (Sakoe-Chiba): c(i,j) = +inf where |i - j| > k
//     dtw(x,y) = D(n-1, m-1)
// min of non-NaN values is exact, so the three-way min has no order; the sub, the abs / mul and the add have exactly one.  The
// value of a cell is therefore a function of its three neighbours alone and every traversal gives the same bits.
//
// Geometry (da_dtw_plan): one wave per pair, DTW_WAVES pairs per block, no LDS.  Lane l owns the W columns [l W, (l + 1) W) of
// the matrix -- W = the smallest class of DTW_CLASSES that is >= ceil(m / 64), a template parameter, so the strip (the previous
// row's W values and the W values of y) lives in registers and the walk along it is fully unrolled.  At step t lane l works on
// row t - l: a wavefront.  What lane l needs from its left neighbour -- D(i, l W - 1), the neighbour's last column of the same
// row, finished one step earlier, and x[i], which the neighbour used one step earlier -- moves one lane up per step with a
// whole-wave DPP shift (v_mov_b32 wave_shr:1), not through memory; the value received one step before is the diagonal.  Lane 0
// takes x[t] from a 64-element chunk of x the wave loads (coalesced) every 64 steps, one chunk ahead, by v_readlane.
// lanes = ceil(m / W) of the 64 hold columns, steps = n + lanes - 1: the loop ends with the step in which the lane of column
// m - 1 finishes row n - 1.
//
// No lane is ever masked: a lane whose row t - l is not a row of the matrix computes too, on x = +inf.  Columns at and past m
// hold y = -inf.  Either makes the cost +inf (inf - (-inf) = inf: no NaN), so rows before 0 stay +inf, which is the boundary,
// and rows from n on are +inf that only rows from n on ever read.  The step loop is unrolled by two over two copies of the
// strip (DTW_PINGPONG): a cell reads up and diagonal from one and writes the other, three VALU instructions per float cell
// (v_sub, v_min3, v_add with |.| as a source modifier).  Updating one copy in place costs a register move per cell instead;
// the double strips that would not fit the register file twice do that.
//
// Tables may be float or double (is64 flags, read at the two places that load: the strip of y once per pair, a chunk of x every
// 64 steps); a float element widens to double exactly.  An index outside its table gives NaN for that pair, nothing is read.
// A pair's result depends on its two rows, the metric and the band only -- not on P, its position or the other pairs.  No
// atomics.
#include "common.h"

#include <limits>

#pragma clang fp contract(off)      // the squared cost is rounded before it is added

constexpr int DTW_WAVES = 4;               // pairs (waves) of one block
constexpr int DTW_MAXLEN = 4608;           // 64 lanes x the widest strip
constexpr int DTW_NCLASS = 8;
static const int DTW_CLASSES[DTW_NCLASS] = {1, 2, 4, 8, 16, 32, 48, 72};

// whole-wave shift by one lane towards the higher lanes: lane l receives lane l - 1's src, lane 0 keeps `old`
__device__ __forceinline__ int dtw_shr1_i(int old, int src) { return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ float dtw_shr1(float old, float src) {
  return __int_as_float(dtw_shr1_i(__float_as_int(old), __float_as_int(src)));
}

__device__ __forceinline__ double dtw_shr1(double old, double src) {
  const long long o = __double_as_longlong(old), s = __double_as_longlong(src);
  const int lo = dtw_shr1_i((int)(o & 0xffffffffll), (int)(s & 0xffffffffll));
  const int hi = dtw_shr1_i((int)(o >> 32), (int)(s >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// lane k's value in every lane (k wave-uniform)
__device__ __forceinline__ float dtw_lane(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

__device__ __forceinline__ double dtw_lane(double v, int k) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), k);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), k);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

template <typename T>
__device__ __forceinline__ T dtw_load(const void* row, int is64, int i) {
  return is64 ? (T) reinterpret_cast<const double*>(row)[i] : (T) reinterpret_cast<const float*>(row)[i];
}

__device__ __forceinline__ float dtw_min(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double dtw_min(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ float dtw_abs(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ double dtw_abs(double a) { return __builtin_fabs(a); }
__device__ __forceinline__ float dtw_sq(float a) { return __fmul_rn(a, a); }       // (never contracted into an fma)
__device__ __forceinline__ double dtw_sq(double a) { return __dmul_rn(a, a); }

// one row of a lane's strip: src = the row above, left / dg = D(i, base - 1) / D(i - 1, base - 1), off0 = base - i -> dst (may
// be src itself), returns the last column
template <typename T, int W, bool SQ, bool BAND>
__device__ __forceinline__ T dtw_row(const T (&src)[W], T (&dst)[W], const T (&y)[W], T x, T left, T dg, int off0, int band) {
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const T up = src[c];
    const T d = x - y[c];
    T cost = SQ ? dtw_sq(d) : dtw_abs(d);
    if (BAND) {
      const int off = off0 + c;
      if (off > band || off < -band) cost = std::numeric_limits<T>::infinity();
    }
    const T v = cost + dtw_min(dtw_min(up, dg), left);
    dg = up;
    left = v;
    dst[c] = v;
  }
  return left;
}

template <typename T, int W>
constexpr bool DTW_PINGPONG = sizeof(T) == 4 || W <= 32;
// waves per SIMD the register allocation is held to: 2 strips + y of the widest float class fit 256 registers
template <typename T, int W>
constexpr int DTW_MINWAVES = sizeof(T) == 4 && W > 48 ? 2 : 1;

template <typename T, int W, bool SQ, bool BAND>
__global__ __launch_bounds__(DTW_WAVES * 64, (DTW_MINWAVES<T, W>)) void dtw_pairs_kernel(const void* __restrict__ ta, int a64, int lda, int Sa, int n,
                                                                  const void* __restrict__ tb, int b64, int ldb, int Sb, int m,
                                                                  const int* __restrict__ ia, const int* __restrict__ ib, int P,
                                                                  int band, T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * DTW_WAVES + (threadIdx.x >> 6);
  if (p >= P) return;                                                       // (wave-uniform: the waves that stay are whole)
  const T INF = std::numeric_limits<T>::infinity();
  const int ra = ia[p], rb = ib[p];
  if (ra < 0 || ra >= Sa || rb < 0 || rb >= Sb) {                           // (wave-uniform)
    if (lane == 0) out[p] = std::numeric_limits<T>::quiet_NaN();
    return;
  }
  const char* xrow = reinterpret_cast<const char*>(ta) + (size_t)ra * lda * (a64 ? 8 : 4);
  const char* yrow = reinterpret_cast<const char*>(tb) + (size_t)rb * ldb * (b64 ? 8 : 4);
  const int base = lane * W;
  T y[W], A[W];
#pragma unroll
  for (int c = 0; c < W; ++c) {
    y[c] = base + c < m ? dtw_load<T>(yrow, b64, base + c) : -INF;
    A[c] = INF;
  }
  const int lanes = (m + W - 1) / W, steps = n + lanes - 1;
  T xbuf = lane < n ? dtw_load<T>(xrow, a64, lane) : INF;                   // x[64 q + lane] of the chunk q in use; +inf past n
  T xnext = INF;
  T xcur = INF, last = INF;
  T diag = lane == 0 ? (T)0 : INF;                                          // D(i - 1, base - 1) of the lane's next row
  int t = 0;
#define DTW_STEP(SRC, DST)                                                                            \
  {                                                                                                   \
    const int k = t & 63;                                                                             \
    if (k == 0) {                                                                                     \
      if (t) xbuf = xnext;                                                                            \
      const int j = t + 64 + lane;                                                                    \
      xnext = j < n ? dtw_load<T>(xrow, a64, j) : INF;                                                \
    }                                                                                                 \
    xcur = dtw_shr1(dtw_lane(xbuf, k), xcur);              /* x[t - lane] */                           \
    const T recv = dtw_shr1(INF, last);                    /* D(t - lane, base - 1); lane 0: +inf */   \
    last = dtw_row<T, W, SQ, BAND>(SRC, DST, y, xcur, recv, diag, base - (t - lane), band);           \
    diag = recv;                                                                                      \
    ++t;                                                                                              \
  }
  if constexpr (DTW_PINGPONG<T, W>) {
    T B[W];
    while (t + 1 < steps) {
      DTW_STEP(A, B)
      DTW_STEP(B, A)
    }
    if (t < steps) {
      DTW_STEP(A, B)
#pragma unroll
      for (int c = 0; c < W; ++c) A[c] = B[c];
    }
  } else {
    while (t < steps) DTW_STEP(A, A)
  }
#undef DTW_STEP
  const int cr = (m - 1) % W;                                               // A: row n - 1 in the lane of column m - 1
  T res = INF;
#pragma unroll
  for (int c = 0; c < W; ++c)
    if (c == cr) res = A[c];
  if (lane == (m - 1) / W) out[p] = res;
}

// out[g] = (((0 + d[off[g]]) + d[off[g] + 1]) + ...) / length in double; an empty segment, or one outside [0, P]: NaN
__global__ __launch_bounds__(256) void dtw_segment_mean_kernel(const void* __restrict__ d, int d64, int P,
                                                               const int* __restrict__ off, int G, double* __restrict__ out) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const int lo = off[g], hi = off[g + 1];
  double r = std::numeric_limits<double>::quiet_NaN();
  if (lo >= 0 && hi <= P && lo < hi) {
    double s = 0.0;
    for (int q = lo; q < hi; ++q) s += dtw_load<double>(d, d64, q);
    r = s / (double)(hi - lo);
  }
  out[g] = r;
}

static inline bool dtw_len_ok(int n, int m) { return n >= 1 && m >= 1 && n <= DTW_MAXLEN && m <= DTW_MAXLEN; }

static inline int dtw_class(int m) {
  const int need = (m + 63) / 64;
  for (int q = 0; q < DTW_NCLASS; ++q)
    if (DTW_CLASSES[q] >= need) return DTW_CLASSES[q];
  return 0;
}

template <typename T, int W>
static void dtw_launch(int sq, bool banded, dim3 grid, hipStream_t stream, const void* ta, int a64, int lda, int Sa, int n,
                       const void* tb, int b64, int ldb, int Sb, int m, const int* ia, const int* ib, int P, int band, T* out) {
  const dim3 block(DTW_WAVES * 64);
#define DTW_GO(SQ, BAND)                                                                                                  \
  hipLaunchKernelGGL((dtw_pairs_kernel<T, W, SQ, BAND>), grid, block, 0, stream, ta, a64, lda, Sa, n, tb, b64, ldb, Sb, m, ia, \
                     ib, P, band, out)
  if (sq) {
    if (banded) DTW_GO(true, true); else DTW_GO(true, false);
  } else {
    if (banded) DTW_GO(false, true); else DTW_GO(false, false);
  }
#undef DTW_GO
}

template <typename T>
static int dtw_dispatch(int W, int sq, bool banded, dim3 grid, hipStream_t stream, const void* ta, int a64, int lda, int Sa, int n,
                        const void* tb, int b64, int ldb, int Sb, int m, const int* ia, const int* ib, int P, int band, T* out) {
#define DTW_W(WW)                                                                                              \
  case WW:                                                                                                     \
    dtw_launch<T, WW>(sq, banded, grid, stream, ta, a64, lda, Sa, n, tb, b64, ldb, Sb, m, ia, ib, P, band, out); \
    break;
  switch (W) {
    DTW_W(1) DTW_W(2) DTW_W(4) DTW_W(8) DTW_W(16) DTW_W(32) DTW_W(48) DTW_W(72)
    default:
      return DA_EINVAL;
  }
#undef DTW_W
  return DA_OK;
}

extern "C" {

int da_dtw_max_len(void) { return DTW_MAXLEN; }

int da_dtw_shape_ok(int n, int m, int acc, int a64, int b64) {
  if (!dtw_len_ok(n, m) || (acc != 0 && acc != 1)) return 0;
  if (acc == 0 && (a64 || b64)) return 0;
  return 1;
}

// out[0..6] = lanes that hold columns, columns per lane, steps, waves per block, grid x, threads per block, LDS bytes
int da_dtw_plan(int n, int m, int P, int acc, int* out) {
  if (!dtw_len_ok(n, m) || (acc != 0 && acc != 1) || P < 1 || !out) return DA_EINVAL;
  const int W = dtw_class(m), lanes = (m + W - 1) / W;
  out[0] = lanes;
  out[1] = W;
  out[2] = n + lanes - 1;
  out[3] = DTW_WAVES;
  out[4] = (P + DTW_WAVES - 1) / DTW_WAVES;
  out[5] = DTW_WAVES * 64;
  out[6] = 0;
  return DA_OK;
}

int da_dtw_pairs(const void* ta, int a64, int lda, int Sa, int n, const void* tb, int b64, int ldb, int Sb, int m, const int* ia,
                 const int* ib, int P, int acc, int metric, int band, void* out, hipStream_t stream) {
  DA_ENTER();
  a64 = a64 ? 1 : 0;
  b64 = b64 ? 1 : 0;
  if (!da_dtw_shape_ok(n, m, acc, a64, b64) || (metric != 0 && metric != 1) || P < 1 || Sa < 1 || Sb < 1 || lda < n || ldb < m ||
      !ta || !tb || !ia || !ib || !out)
    return DA_EINVAL;
  const bool banded = band >= 0 && band < (n > m ? n : m);                  // (a band that holds every cell is no band)
  const int W = dtw_class(m);
  const dim3 grid((P + DTW_WAVES - 1) / DTW_WAVES);
  int rc;
  if (acc == 0)
    rc = dtw_dispatch<float>(W, metric, banded, grid, stream, ta, a64, lda, Sa, n, tb, b64, ldb, Sb, m, ia, ib, P, band, (float*)out);
  else
    rc = dtw_dispatch<double>(W, metric, banded, grid, stream, ta, a64, lda, Sa, n, tb, b64, ldb, Sb, m, ia, ib, P, band,
                              (double*)out);
  if (rc != DA_OK) return rc;
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_dtw_segment_mean(const void* dist, int d64, int P, const int* offsets, int G, double* out, hipStream_t stream) {
  DA_ENTER();
  if (P < 0 || G < 1 || !offsets || !out || (P > 0 && !dist)) return DA_EINVAL;
  hipLaunchKernelGGL(dtw_segment_mean_kernel, dim3((G + 255) / 256), dim3(256), 0, stream, dist, d64 ? 1 : 0, P, offsets, G, out);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
