// Grouped k3 p1 Conv1d (groups = 32, stride 1 / 2) on channels-last fp32 maps: conv2 of the SE-ResNeXt 32x4d bottleneck
// (reference models/senet.py:147-168).  Forward, data gradient and weight gradient; C ABI in include/deepards_hip.h
// ("grouped k3 convolution").
//
//     y[r][lo][co] = sum_{k < 3, j < cg} w[co][j][k] x[r][lo S + k - 1][g cg + j],   g = co / cg,  cg = C / 32
//
// What bounds them: 2 * 3 * cg = 24 ... 192 FLOP per output element against 8 bytes moved, i.e. 3 ... 24 FLOP / byte where
// the machine balance is about 25 -- one read and one write of the map, not arithmetic (the fp32 matrix cores run at the
// vector rate on gfx950, so there is no MFMA form).  The design keeps the map traffic at exactly that:
//   * a block owns a slab of 128 channels (4 ... 32 whole groups) and walks `nt` consecutive TILES of 8 output positions of
//     one row; the source positions of a tile are staged ONCE in LDS with 16-byte loads (pads and positions beyond the row are
//     written as zeros, never read) and every tap of every channel of the group reads them from there (one ds_read_b128 per
//     four products' operands, broadcast inside a group);
//   * a thread owns ONE channel and four positions of the tile, and keeps its 3 cg weights in registers over all the block's
//     tiles -- the weight is read in torch's layout (C, cg, 3) straight from L2, no pack;
//   * results leave through LDS so that the stores (and the accumulating form's loads) are 16 bytes per lane.
// The data gradient is the same kernel with the weight read transposed inside its group and the tap -> source map of the
// transposed conv (stride 2: an even input position takes tap 1 of dy[li / 2], an odd one taps 0 and 2 of its two neighbours).
// The weight gradient gives a thread the 3 cg sums of its output channel over a CHUNK of tiles, folds the two position halves
// of the block through LDS, writes one partial (C cg 3 floats) per chunk into the workspace and a second launch folds the
// partials (16 slots in chunk order, then the slots in slot order): no atomics, the order is a function of (rows, L, C,
// stride) alone.
//
// Everything a launch dereferences is a function of (rows, L, C, stride) checked by gc_plan() on the host: the same function
// answers da_gconv3_plan and sizes every launch.
#include "common.h"

#define GC_GROUPS 32
#define GC_CB 128          // channels per block
#define GC_TL 8            // positions of the destination map per tile (4 per thread, two halves)
#define GC_THREADS 256

// source positions staged per tile: forward / weight gradient read x at lo S + k - 1; the data gradient reads dy
__host__ __device__ constexpr int gc_nsrc(int S, bool dgrad) { return dgrad ? (S == 1 ? GC_TL + 2 : GC_TL / 2 + 1) : (GC_TL - 1) * S + 3; }
// per-thread span of source positions (4 destination positions)
__host__ __device__ constexpr int gc_span(int S, bool dgrad) { return dgrad ? (S == 1 ? 6 : 3) : 3 * S + 3; }
// source position (relative to the thread's first) that tap k of destination position q reads; -1: the tap does not reach q
__host__ __device__ constexpr int gc_loc(int S, bool dgrad, int q, int k) {
  if (!dgrad) return q * S + k;
  if (S == 1) return q + 2 - k;
  if ((q & 1) == 0) return k == 1 ? q / 2 : -1;
  return k == 0 ? (q + 1) / 2 : k == 2 ? (q - 1) / 2 : -1;
}
__host__ __device__ constexpr size_t gc_lds_conv(int S, bool dgrad) { return (size_t)(gc_nsrc(S, dgrad) + GC_TL) * GC_CB * 4; }
__host__ __device__ constexpr size_t gc_lds_wgrad(int CG, int S) {
  const size_t tiles = (size_t)(gc_nsrc(S, false) + GC_TL) * GC_CB * 4, fold = (size_t)CG * 3 * GC_CB * 4;
  return tiles > fold ? tiles : fold;
}

// tiles [rows][tpr] of the destination map; a block takes tiles [b nt, min((b + 1) nt, tiles))
struct GcGeom {
  int Lsrc, Ldst, C, tpr, nt;
  long long tiles;
};

// stage source positions [s0, s0 + NSRC) of row `row`, channels [c0, c0 + 128): zeros outside [0, Lsrc)
template <int NSRC>
__device__ __forceinline__ void gc_stage(const float* __restrict__ src, float (*xs)[GC_CB], long long row, int s0, int Lsrc, int C,
                                         int c0) {
  for (int i = threadIdx.x; i < NSRC * (GC_CB / 4); i += GC_THREADS) {
    const int p = i / (GC_CB / 4), c4 = i % (GC_CB / 4);
    const int sp = s0 + p;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (sp >= 0 && sp < Lsrc) v = *reinterpret_cast<const f32x4*>(src + ((size_t)row * Lsrc + sp) * C + c0 + c4 * 4);
    *reinterpret_cast<f32x4*>(&xs[p][c4 * 4]) = v;
  }
}

// forward (DG = false: src = x, dst = y) and data gradient (DG = true: src = dy, dst = dx)
template <int CG, int S, bool DG>
__global__ __launch_bounds__(GC_THREADS) void gconv3_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                            float* __restrict__ dst, GcGeom gm, int accumulate) {
  constexpr int NSRC = gc_nsrc(S, DG), SPAN = gc_span(S, DG);
  __shared__ __attribute__((aligned(16))) float xs[NSRC][GC_CB];
  __shared__ __attribute__((aligned(16))) float os[GC_TL][GC_CB];
  const int tid = threadIdx.x, cl = tid & (GC_CB - 1), half = tid >> 7;
  const int c0 = blockIdx.y * GC_CB, c = c0 + cl;
  const int gl = (cl / CG) * CG;                         // first channel of the thread's group inside the slab
  // the thread's 3 cg weights, [j][k]: forward w[c][j][k]; data gradient w[g cg + j][c - g cg][k]
  float wr[CG * 3];
  if (!DG) {
#pragma unroll
    for (int i = 0; i < CG * 3 / 4; ++i) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(w + (size_t)c * (CG * 3) + i * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) wr[i * 4 + e] = v[e];
    }
  } else {
    const int g0 = c0 + gl, ci = cl - gl;
#pragma unroll
    for (int j = 0; j < CG; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) wr[j * 3 + k] = w[((size_t)(g0 + j) * CG + ci) * 3 + k];
  }
  const int hb = half * (DG ? (S == 1 ? 4 : 2) : 4 * S);   // the thread's first source position inside the staged tile
  const long long t_begin = (long long)blockIdx.x * gm.nt;
  const long long t_end = t_begin + gm.nt < gm.tiles ? t_begin + gm.nt : gm.tiles;
  for (long long t = t_begin; t < t_end; ++t) {
    const long long row = t / gm.tpr;
    const int d0 = (int)(t - row * gm.tpr) * GC_TL;       // first destination position of the tile
    const int s0 = DG ? (S == 1 ? d0 - 1 : d0 / 2) : d0 * S - 1;
    gc_stage<NSRC>(src, xs, row, s0, gm.Lsrc, gm.C, c0);
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j4 = 0; j4 < CG / 4; ++j4) {
      f32x4 xv[SPAN];
#pragma unroll
      for (int p = 0; p < SPAN; ++p) xv[p] = *reinterpret_cast<const f32x4*>(&xs[hb + p][gl + j4 * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            constexpr bool dg = DG;
            const int loc = gc_loc(S, dg, q, k);
            if (loc >= 0) acc[q] = fmaf(wr[(j4 * 4 + e) * 3 + k], xv[loc][e], acc[q]);
          }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) os[half * 4 + q][cl] = acc[q];
    __syncthreads();
    {
      const int p = tid / (GC_CB / 4), c4 = tid % (GC_CB / 4);      // 8 positions x 32 quads = 256 threads
      const int dp = d0 + p;
      if (dp < gm.Ldst) {
        float* o = dst + ((size_t)row * gm.Ldst + dp) * gm.C + c0 + c4 * 4;
        f32x4 v = *reinterpret_cast<const f32x4*>(&os[p][c4 * 4]);
        if (accumulate) v += *reinterpret_cast<const f32x4*>(o);
        *reinterpret_cast<f32x4*>(o) = v;
      }
    }
    // (the next tile's staging writes xs only: every thread read it before the barrier above; os is rewritten behind the
    // next barrier)
  }
}

// weight-gradient partials: part[chunk][co][j][k] = sum over the chunk's tiles of dy[r][lo][co] x[r][lo S + k - 1][g cg + j]
template <int CG, int S>
__global__ __launch_bounds__(GC_THREADS) void gconv3_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                  float* __restrict__ part, GcGeom gm) {
  constexpr int NSRC = gc_nsrc(S, false);
  constexpr size_t LDS = gc_lds_wgrad(CG, S);
  __shared__ __attribute__((aligned(16))) float smem[LDS / 4];
  float(*xs)[GC_CB] = reinterpret_cast<float(*)[GC_CB]>(smem);
  float(*ds)[GC_CB] = reinterpret_cast<float(*)[GC_CB]>(smem + NSRC * GC_CB);
  float(*fold)[GC_CB] = reinterpret_cast<float(*)[GC_CB]>(smem);          // [j * 3 + k][channel], behind the last tile
  const int tid = threadIdx.x, cl = tid & (GC_CB - 1), half = tid >> 7;
  const int c0 = blockIdx.y * GC_CB;
  const int gl = (cl / CG) * CG;
  float acc[CG * 3];
#pragma unroll
  for (int i = 0; i < CG * 3; ++i) acc[i] = 0.f;
  const long long t_begin = (long long)blockIdx.x * gm.nt;
  const long long t_end = t_begin + gm.nt < gm.tiles ? t_begin + gm.nt : gm.tiles;
  for (long long t = t_begin; t < t_end; ++t) {
    const long long row = t / gm.tpr;
    const int d0 = (int)(t - row * gm.tpr) * GC_TL;
    gc_stage<NSRC>(x, xs, row, d0 * S - 1, gm.Lsrc, gm.C, c0);
    gc_stage<GC_TL>(dy, ds, row, d0, gm.Ldst, gm.C, c0);
    __syncthreads();
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = ds[half * 4 + q][cl];
    // every staged position is read once and serves all the (position q, tap k) pairs it belongs to (q S + k = p): up to three
    // under stride 1; per accumulator the positions still arrive in ascending order
#pragma unroll
    for (int j4 = 0; j4 < CG / 4; ++j4)
#pragma unroll
      for (int p = 0; p < gc_span(S, false); ++p) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(&xs[half * 4 * S + p][gl + j4 * 4]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int d = p - k;
          if (d >= 0 && d % S == 0 && d / S < 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[(j4 * 4 + e) * 3 + k] = fmaf(g[d / S], xv[e], acc[(j4 * 4 + e) * 3 + k]);
          }
        }
      }
    __syncthreads();
  }
  // fold the two position halves (fixed order: half 0 + half 1), then one partial per chunk in torch's layout
  if (half == 1) {
#pragma unroll
    for (int i = 0; i < CG * 3; ++i) fold[i][cl] = acc[i];
  }
  __syncthreads();
  if (half == 0) {
    float* o = part + ((size_t)blockIdx.x * gm.C + c0 + cl) * (CG * 3);
#pragma unroll
    for (int i = 0; i < CG * 3 / 4; ++i) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[i * 4 + e] + fold[i * 4 + e][cl];
      *reinterpret_cast<f32x4*>(o + i * 4) = v;
    }
  }
}

// dw (+)= sum_p part[p]; n4 = C cg 3 / 4 quads.  A block folds 16 quads: slot s of 16 sums the partials p = s, s + 16, ... in
// ascending order, then the slots are added in slot order -- a fixed tree, whatever the partial count
#define GC_FOLD_SLOTS 16
#define GC_FOLD_QUADS (GC_THREADS / GC_FOLD_SLOTS)
__global__ __launch_bounds__(GC_THREADS) void gconv3_wgrad_fold_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                       int nparts, int n4, int accumulate) {
  __shared__ f32x4 red[GC_FOLD_SLOTS][GC_FOLD_QUADS];
  const int ql = threadIdx.x % GC_FOLD_QUADS, slot = threadIdx.x / GC_FOLD_QUADS;
  const int i = blockIdx.x * GC_FOLD_QUADS + ql;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (i < n4) {
#pragma unroll 4
    for (int p = slot; p < nparts; p += GC_FOLD_SLOTS) s += *reinterpret_cast<const f32x4*>(part + ((size_t)p * n4 + i) * 4);
  }
  red[slot][ql] = s;
  __syncthreads();
  if (threadIdx.x < GC_FOLD_QUADS && i < n4) {
    s = red[0][ql];
#pragma unroll
    for (int k = 1; k < GC_FOLD_SLOTS; ++k) s += red[k][ql];
    float* o = dw + (size_t)i * 4;
    if (accumulate) s += *reinterpret_cast<const f32x4*>(o);
    *reinterpret_cast<f32x4*>(o) = s;
  }
}

// ---- the one planning function (host only) ----------------------------------------------------------------------------------
struct GcPlan {
  GcGeom gm;
  int cg;
  unsigned grid[3];
  size_t lds, workspace;
  int fold_blocks, nparts;
};

static bool gc_shape_ok(int C, int groups, int stride) {
  return groups == GC_GROUPS && (C == 128 || C == 256 || C == 512 || C == 1024) && (stride == 1 || stride == 2);
}
// tiles one block of the forward / data gradient walks (its 3 cg weights stay in registers meanwhile)
static int gc_conv_nt(int cg) { return cg <= 8 ? 4 : cg == 16 ? 8 : 16; }
// most chunks (= partials) of a weight gradient: the partials of one launch stay under 13 MB (a partial is C cg 3 floats: 6 KB
// ... 393 KB), well under the maps' traffic at the batch sizes where it matters; 256 ... 512 blocks
static int gc_wgrad_max_chunks(int cg) { return cg <= 8 ? 256 : cg == 16 ? 128 : 32; }
#define GC_WGRAD_MIN_NT 4

// which: 0 forward, 1 data gradient, 2 weight gradient; L: the length of x / dx.  false: no legal launch
static bool gc_plan(int which, long long rows, long long L, int C, int stride, GcPlan* p) {
  if (which < 0 || which > 2 || !gc_shape_ok(C, GC_GROUPS, stride) || rows < 1 || L < 1) return false;
  const long long Lo = (L - 1) / stride + 1;
  const long long lim = 1ll << 31;
  if (rows >= lim || L >= lim || rows * L >= lim || rows * L * C >= lim || rows * Lo * C >= lim) return false;
  const int cg = C / GC_GROUPS;
  const long long Ldst = which == 1 ? L : Lo, Lsrc = which == 1 ? Lo : L;      // (weight gradient: tiles over dy, x staged)
  GcGeom gm;
  gm.Lsrc = (int)Lsrc;
  gm.Ldst = (int)Ldst;
  gm.C = C;
  gm.tpr = (int)((Ldst + GC_TL - 1) / GC_TL);
  gm.tiles = rows * gm.tpr;
  if (which == 2) {
    const long long mc = gc_wgrad_max_chunks(cg);
    const long long nt = (gm.tiles + mc - 1) / mc;
    gm.nt = (int)(nt < GC_WGRAD_MIN_NT ? GC_WGRAD_MIN_NT : nt);
  } else {
    gm.nt = gc_conv_nt(cg);
  }
  const long long nblk = (gm.tiles + gm.nt - 1) / gm.nt;
  if (nblk > 2147483647ll || C / GC_CB > 65535) return false;
  p->gm = gm;
  p->cg = cg;
  p->grid[0] = (unsigned)nblk;
  p->grid[1] = (unsigned)(C / GC_CB);
  p->grid[2] = 1;
  p->lds = which == 2 ? gc_lds_wgrad(cg, stride) : gc_lds_conv(stride, which == 1);
  if (p->lds > 64 * 1024) return false;                   // static LDS: the kernels do not opt in to more
  p->nparts = which == 2 ? (int)nblk : 0;
  p->workspace = which == 2 ? (size_t)nblk * C * cg * 3 * sizeof(float) : 0;
  p->fold_blocks = (C * cg * 3 / 4 + GC_FOLD_QUADS - 1) / GC_FOLD_QUADS;
  return true;
}

template <int CG>
static void gc_launch_conv(const GcPlan& p, int stride, bool dgrad, const float* src, const float* w, float* dst, int accumulate,
                           hipStream_t stream) {
  const dim3 grid(p.grid[0], p.grid[1]), block(GC_THREADS);
  if (!dgrad && stride == 1) hipLaunchKernelGGL((gconv3_kernel<CG, 1, false>), grid, block, 0, stream, src, w, dst, p.gm, accumulate);
  else if (!dgrad) hipLaunchKernelGGL((gconv3_kernel<CG, 2, false>), grid, block, 0, stream, src, w, dst, p.gm, accumulate);
  else if (stride == 1) hipLaunchKernelGGL((gconv3_kernel<CG, 1, true>), grid, block, 0, stream, src, w, dst, p.gm, accumulate);
  else hipLaunchKernelGGL((gconv3_kernel<CG, 2, true>), grid, block, 0, stream, src, w, dst, p.gm, accumulate);
}

template <int CG>
static void gc_launch_wgrad(const GcPlan& p, int stride, const float* dy, const float* x, float* part, hipStream_t stream) {
  const dim3 grid(p.grid[0], p.grid[1]), block(GC_THREADS);
  if (stride == 1) hipLaunchKernelGGL((gconv3_wgrad_kernel<CG, 1>), grid, block, 0, stream, dy, x, part, p.gm);
  else hipLaunchKernelGGL((gconv3_wgrad_kernel<CG, 2>), grid, block, 0, stream, dy, x, part, p.gm);
}

#define GC_DISPATCH_CG(cg, STMT) \
  do {                           \
    if ((cg) == 4) {             \
      constexpr int CG = 4;      \
      STMT;                      \
    } else if ((cg) == 8) {      \
      constexpr int CG = 8;      \
      STMT;                      \
    } else if ((cg) == 16) {     \
      constexpr int CG = 16;     \
      STMT;                      \
    } else {                     \
      constexpr int CG = 32;     \
      STMT;                      \
    }                            \
  } while (0)

static bool gc_aligned(const void* a, const void* b, const void* c) {
  return a && b && c && !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15);
}

extern "C" {

int da_gconv3_shape_ok(int C, int groups, int stride) { return gc_shape_ok(C, groups, stride) ? 1 : 0; }

int da_gconv3_plan(int which, int rows, int L, int C, int stride, int* grid, int* block, size_t* lds, size_t* workspace) {
  GcPlan p;
  if (!gc_plan(which, rows, L, C, stride, &p)) return DA_EINVAL;
  if (grid) {
    grid[0] = (int)p.grid[0];
    grid[1] = (int)p.grid[1];
    grid[2] = (int)p.grid[2];
  }
  if (block) {
    block[0] = GC_THREADS;
    block[1] = block[2] = 1;
  }
  if (lds) *lds = p.lds;
  if (workspace) *workspace = p.workspace;
  return DA_OK;
}

int da_gconv3_tiling(int which, int rows, int L, int C, int stride, int* tile_positions, int* tiles_per_block, int* tiles) {
  GcPlan p;
  if (!gc_plan(which, rows, L, C, stride, &p) || p.gm.tiles > 2147483647ll) return DA_EINVAL;
  if (tile_positions) *tile_positions = GC_TL;
  if (tiles_per_block) *tiles_per_block = p.gm.nt;
  if (tiles) *tiles = (int)p.gm.tiles;
  return DA_OK;
}

int da_gconv3_fwd(const float* x, const float* w, float* y, int rows, int L, int C, int stride, hipStream_t stream) {
  DA_ENTER();
  GcPlan p;
  if (!gc_plan(0, rows, L, C, stride, &p) || !gc_aligned(x, w, y)) return DA_EINVAL;
  GC_DISPATCH_CG(p.cg, gc_launch_conv<CG>(p, stride, false, x, w, y, 0, stream));
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_gconv3_dgrad(const float* dy, const float* w, float* dx, int rows, int Lin, int C, int stride, int accumulate,
                    hipStream_t stream) {
  DA_ENTER();
  GcPlan p;
  if (!gc_plan(1, rows, Lin, C, stride, &p) || !gc_aligned(dy, w, dx)) return DA_EINVAL;
  GC_DISPATCH_CG(p.cg, gc_launch_conv<CG>(p, stride, true, dy, w, dx, accumulate ? 1 : 0, stream));
  DA_CHECK_LAUNCH();
  return DA_OK;
}

int da_gconv3_wgrad(const float* dy, const float* x, float* dw, float* workspace, int rows, int Lin, int C, int stride,
                    int accumulate, hipStream_t stream) {
  DA_ENTER();
  GcPlan p;
  if (!gc_plan(2, rows, Lin, C, stride, &p) || !gc_aligned(dy, x, dw) || !workspace || ((uintptr_t)workspace & 15)) return DA_EINVAL;
  GC_DISPATCH_CG(p.cg, gc_launch_wgrad<CG>(p, stride, dy, x, workspace, stream));
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(gconv3_wgrad_fold_kernel, dim3(p.fold_blocks), dim3(GC_THREADS), 0, stream, workspace, dw, p.nparts,
                     C * p.cg * 3 / 4, accumulate ? 1 : 0);
  DA_CHECK_LAUNCH();
  return DA_OK;
}

}  // extern "C"
