// Batched Grad-CAM of a cnn_linear + DenseNet model (reference gradcam.py:28-205: CamExtractor, GradCam, MaxMinNormCam,
// FracTotalNormCam, UnNormalizedCam) from the norm5 map alone.
//
// Behind `features` the head is relu -> AvgPool1d(Lm) -> view(-1) -> linear_final, so the guided gradient the reference
// obtains with a hook and a backward is closed form:  d out[k] / d F[n][l][c] = (F[n][l][c] > 0) W[k][n C + c] / Lm.
// Per window b (NB rows of the map F (B NB, Lm, C) channels-last, WITHOUT the final ReLU), k in {0, 1}:
//
//     P[n][c]    = (1 / Lm) sum_l max(F, 0)                  logits[k] = bias[k] + sum_{n,c} W[k][n C + c] P[n][c]
//     m[n][c]    = #{l : F[n][l][c] > 0}                     (an exact 0 does not count, as in the ReLU's backward)
//     wr_k[n][c] = W[k][n C + c] m[n][c] / Lm^2              (np.mean(grad, axis=2), generate_read_cam)
//     ww_k[c]    = (1 / NB) sum_n wr_k[n][c]                 (np.mean(grad, axis=(0, 2)), generate_cam)
//     R_k[n][l]  = sum_c wr_k[n][c] F[n][l][c]               the read CAM
//     A_k[l]     = sum_c ww_k[c] ((1 / NB) sum_n F[n][l][c]) the window CAM
//
// Two launches.  gradcam_partial_kernel: a block per (window, 64 channels) reads its slice of the map ONCE and writes the
// slice's share of logits, R and A (ww and the row mean are complete inside a channel slice).  gradcam_finish_kernel: a block
// per window folds the slices, takes the arg-max and the reference's three normalisations.
//
// Summation order (fixed by (NB, Lm, C) alone: no atomics, a window's bits do not depend on the batch around it):
//   P         the Lm positions in order                                                                       chain Lm - 1
//   logits    per thread (channel quad q, slot s): rows s, s + 16, ... as one fmaf chain per channel, the 4 channels
//             pairwise (2); xor-butterfly of the wave (6), the 4 waves pairwise (2), the slices by the wave butterfly of
//             the second launch (6), + bias                                                   chain ceil(NB / 16) + 17
//   R         4 channels in the lane (fmaf chain from the first product), butterfly of the 16 lanes of a slice (4), the
//             slices alternately into two sums (<= 15 each), the two added                  chain 3 + 4 + 15 + 1 = 23
//   A         ww and the row mean: rows s, s + 16, ... in the lane, the 16 slots pairwise (4); the product; butterfly of
//             the 64 channels (6); the slices in four strided sums (<= 8) folded by a butterfly (2)
//                                                                                 chain ceil(NB / 16) + 4 + 6 + 8 + 2
// With NB <= GC_MAX_NB = 1024 (beyond: DA_EINVAL) no chain is longer than 64 + 20 = 84 additions; at the reference's
// NB = 20, Lm = 7: P 6, logits 19 (+ P's 6 in front), R 23, A 22.
#include "common.h"

#define GC_CC 64            // channels of one block of the first launch (16 lanes x 4)
#define GC_SLOTS 16         // row slots of a block: slot s takes the rows s, s + 16, ...
#define GC_MAX_LM 8
#define GC_MAX_NB 1024
#define GC_MAX_C 1920
#define GC_TILE 64          // rows of the map a block of the second launch normalises per pass

// workspace record of one (window, channel slice): [NB rows][2 classes][8] R shares | [2][8] A shares | [4] logits shares, pad
__host__ __device__ static inline size_t gc_record(int NB) { return (size_t)(NB + 1) * 16 + 4; }

template <int LM>
__global__ __launch_bounds__(256) void gradcam_partial_kernel(const float* __restrict__ F, const float* __restrict__ W,
                                                              float* __restrict__ ws, int NB, int C, int nchunk) {
  __shared__ f32x4 sF[GC_SLOTS][LM][16];                 // a slot's sum over its rows of F[.][l][c0 .. c0 + 3]
  __shared__ f32x4 sW[GC_SLOTS][2][16];                  // ... of wr_k
  __shared__ float sL[4][2];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / nchunk, ch = blockIdx.x - b * nchunk;
  const int q = tid & 15, slot = tid >> 4;
  const int c0 = ch * GC_CC + q * 4;
  const bool live = c0 < C;                              // C % 32 == 0: the last slice of a C % 64 == 32 map is half empty
  float* __restrict__ rec = ws + ((size_t)b * nchunk + ch) * gc_record(NB);
  const float inv_lm = 1.0f / (float)LM, inv_lm2 = 1.0f / (float)(LM * LM);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 fsum[LM], wsum0 = zero, wsum1 = zero;
#pragma unroll
  for (int l = 0; l < LM; ++l) fsum[l] = zero;
  f32x4 lv0 = zero, lv1 = zero;
  for (int n = slot; n < NB; n += GC_SLOTS) {            // (uniform in the 16 lanes that share a slot)
    f32x4 f[LM], w0 = zero, w1 = zero;
#pragma unroll
    for (int l = 0; l < LM; ++l) f[l] = zero;
    if (live) {
      const float* p = F + ((size_t)(b * NB + n) * LM) * C + c0;
#pragma unroll
      for (int l = 0; l < LM; ++l) f[l] = *reinterpret_cast<const f32x4*>(p + (size_t)l * C);
      w0 = *reinterpret_cast<const f32x4*>(W + (size_t)n * C + c0);
      w1 = *reinterpret_cast<const f32x4*>(W + (size_t)(NB + n) * C + c0);
    }
    f32x4 pos = zero, cnt = zero;
#pragma unroll
    for (int l = 0; l < LM; ++l) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool on = f[l][e] > 0.f;
        pos[e] += on ? f[l][e] : 0.f;
        cnt[e] += on ? 1.f : 0.f;
      }
      fsum[l] += f[l];
    }
    f32x4 wr0, wr1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float pe = pos[e] * inv_lm;
      lv0[e] = fmaf(w0[e], pe, lv0[e]);
      lv1[e] = fmaf(w1[e], pe, lv1[e]);
      wr0[e] = (w0[e] * cnt[e]) * inv_lm2;
      wr1[e] = (w1[e] * cnt[e]) * inv_lm2;
    }
    wsum0 += wr0;
    wsum1 += wr1;
    float r[2][GC_MAX_LM];
#pragma unroll
    for (int l = 0; l < GC_MAX_LM; ++l) {
      float a0 = 0.f, a1 = 0.f;
      if (l < LM) {
        a0 = wr0[0] * f[l][0];
        a1 = wr1[0] * f[l][0];
#pragma unroll
        for (int e = 1; e < 4; ++e) {
          a0 = fmaf(wr0[e], f[l][e], a0);
          a1 = fmaf(wr1[e], f[l][e], a1);
        }
        // INVARIANT: these shuffles run inside the row loop, whose trip count differs between the four slots of a wave
        // when NB % 16 != 0.  They are safe only because every offset is < 16 and a slot is an ALIGNED group of 16 lanes
        // (slot = tid >> 4): a lane exchanges with lanes of its own slot alone, and those share n and so the trip count.
        // A change of GC_SLOTS, of the lane -> (q, slot) mapping or of the offsets must keep every partner inside a group
        // with one trip count (or hoist the shuffles out of the loop).
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {                // the 16 lanes of the slot: every one ends with the slice's sum
          a0 += __shfl_xor(a0, o, 64);
          a1 += __shfl_xor(a1, o, 64);
        }
      }
      r[0][l] = a0;
      r[1][l] = a1;
    }
    if (q == 0) {                                        // [k][8], positions >= LM written as zeros
      f32x4* d = reinterpret_cast<f32x4*>(rec + (size_t)n * 16);
      d[0] = f32x4{r[0][0], r[0][1], r[0][2], r[0][3]};
      d[1] = f32x4{r[0][4], r[0][5], r[0][6], r[0][7]};
      d[2] = f32x4{r[1][0], r[1][1], r[1][2], r[1][3]};
      d[3] = f32x4{r[1][4], r[1][5], r[1][6], r[1][7]};
    }
  }
#pragma unroll
  for (int l = 0; l < LM; ++l) sF[slot][l][q] = fsum[l];
  sW[slot][0][q] = wsum0;
  sW[slot][1][q] = wsum1;
  const float lg0 = wave_sum((lv0[0] + lv0[1]) + (lv0[2] + lv0[3]));
  const float lg1 = wave_sum((lv1[0] + lv1[1]) + (lv1[2] + lv1[3]));
  if ((tid & 63) == 0) {
    sL[tid >> 6][0] = lg0;
    sL[tid >> 6][1] = lg1;
  }
  __syncthreads();
  // the slice's share of A: thread = (channel c of the 64, wave w takes the positions w, w + 4)
  {
    const int c = tid & 63, w = tid >> 6;
    const float inv_nb = 1.0f / (float)NB;
    const float* fW = reinterpret_cast<const float*>(sW);
    const float* fF = reinterpret_cast<const float*>(sF);
    float ww[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float v[GC_SLOTS];
#pragma unroll
      for (int s = 0; s < GC_SLOTS; ++s) v[s] = fW[(s * 2 + k) * 64 + c];
#pragma unroll
      for (int h = GC_SLOTS / 2; h > 0; h >>= 1)
#pragma unroll
        for (int s = 0; s < h; ++s) v[s] = v[2 * s] + v[2 * s + 1];
      ww[k] = v[0] * inv_nb;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int l = w + 4 * i;                           // (wave-uniform)
      float a0 = 0.f, a1 = 0.f;
      if (l < LM) {
        float v[GC_SLOTS];
#pragma unroll
        for (int s = 0; s < GC_SLOTS; ++s) v[s] = fF[(s * LM + l) * 64 + c];
#pragma unroll
        for (int h = GC_SLOTS / 2; h > 0; h >>= 1)
#pragma unroll
          for (int s = 0; s < h; ++s) v[s] = v[2 * s] + v[2 * s + 1];
        const float fb = v[0] * inv_nb;
        a0 = wave_sum(ww[0] * fb);
        a1 = wave_sum(ww[1] * fb);
      }
      if (c == 0) {
        rec[(size_t)NB * 16 + l] = a0;
        rec[(size_t)NB * 16 + 8 + l] = a1;
      }
    }
  }
  if (tid == 0) {
    float* d = rec + (size_t)(NB + 1) * 16;
    d[0] = (sL[0][0] + sL[1][0]) + (sL[2][0] + sL[3][0]);
    d[1] = (sL[0][1] + sL[1][1]) + (sL[2][1] + sL[3][1]);
    d[2] = 0.f;
    d[3] = 0.f;
  }
}

// u = trunc(255 (r - mn) / (mx - mn)) of a ReLU'd value (MaxMinNormCam.normalize, gradcam.py:157-162); the caller has
// ruled out mx == mn
__device__ __forceinline__ unsigned char gc_maxmin(float r, float mn, float mx) {
  return (unsigned char)(int)(255.f * ((r - mn) / (mx - mn)));
}

// block = one window: fold the slices, arg-max, the normalisations of the target class
__global__ __launch_bounds__(256) void gradcam_finish_kernel(const float* __restrict__ ws, const float* __restrict__ bias,
                                                             const int* __restrict__ target_in, int NB, int LM, int nchunk,
                                                             float* __restrict__ logits, int* __restrict__ target,
                                                             float* __restrict__ A, float* __restrict__ R,
                                                             float* __restrict__ cam, unsigned char* __restrict__ cam_mm,
                                                             unsigned char* __restrict__ cam_deg,
                                                             unsigned char* __restrict__ read_mm,
                                                             unsigned char* __restrict__ read_deg,
                                                             unsigned char* __restrict__ read_frac) {
  __shared__ int s_t;
  __shared__ float sA[16];
  __shared__ float sR[GC_TILE][17];
  const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63;
  const size_t recn = gc_record(NB);
  const float* __restrict__ base = ws + (size_t)b * nchunk * recn;
  if (tid < 64) {                                        // wave 0: logits and the target (nchunk <= 30 slices, one a lane)
    float l0 = 0.f, l1 = 0.f;
    if (lane < nchunk) {
      const float* d = base + (size_t)lane * recn + (size_t)(NB + 1) * 16;
      l0 = d[0];
      l1 = d[1];
    }
    l0 = wave_sum(l0) + bias[0];
    l1 = wave_sum(l1) + bias[1];
    if (lane == 0) {
      const int ti = target_in[b];
      // np.argmax: the first maximum, and a NaN counts as one
      const int am = (l1 > l0 || (l1 != l1 && l0 == l0)) ? 1 : 0;
      const int t = ti < 0 ? am : (ti != 0 ? 1 : 0);
      logits[(size_t)b * 2] = l0;
      logits[(size_t)b * 2 + 1] = l1;
      target[b] = t;
      s_t = t;
    }
  } else if (tid < 128) {                                // wave 1: A, lane = (value j = k * 8 + l, slice group g)
    const int j = lane & 15, g = lane >> 4;
    float a = 0.f;
    for (int ch = g; ch < nchunk; ch += 4) a += base[(size_t)ch * recn + (size_t)NB * 16 + j];
    a += __shfl_xor(a, 16, 64);
    a += __shfl_xor(a, 32, 64);
    if (g == 0) {
      sA[j] = a;
      if ((j & 7) < LM) A[((size_t)b * 2 + (j >> 3)) * LM + (j & 7)] = a;
    }
  }
  __syncthreads();
  const int t = s_t;
  if (tid == 0) {                                        // the window CAM of the target class
    float mn = 0.f, mx = 0.f;
    for (int l = 0; l < LM; ++l) {
      const float r = fmaxf(sA[t * 8 + l], 0.f);
      cam[(size_t)b * LM + l] = r;
      mn = l ? fminf(mn, r) : r;
      mx = l ? fmaxf(mx, r) : r;
    }
    const bool deg = !(mx > mn);
    cam_deg[b] = deg ? 1 : 0;
    for (int l = 0; l < LM; ++l)
      cam_mm[(size_t)b * LM + l] = deg ? (unsigned char)0 : gc_maxmin(fmaxf(sA[t * 8 + l], 0.f), mn, mx);
  }
  for (int n0 = 0; n0 < NB; n0 += GC_TILE) {
    {
      const int r = tid >> 2, part = tid & 3, n = n0 + r;      // part = (class k, half of the 8 positions)
      if (n < NB) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        const float* p = base + (size_t)n * 16 + part * 4;
        int ch = 0;
        for (; ch + 2 <= nchunk; ch += 2) {
          a0 += *reinterpret_cast<const f32x4*>(p + (size_t)ch * recn);
          a1 += *reinterpret_cast<const f32x4*>(p + (size_t)(ch + 1) * recn);
        }
        if (ch < nchunk) a0 += *reinterpret_cast<const f32x4*>(p + (size_t)ch * recn);
        a0 += a1;
        const int k = part >> 1, lb = (part & 1) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sR[r][part * 4 + e] = a0[e];
          if (lb + e < LM) R[(((size_t)b * 2 + k) * NB + n) * LM + lb + e] = a0[e];
        }
      }
    }
    __syncthreads();
    if (tid < GC_TILE && n0 + tid < NB) {
      const int n = n0 + tid;
      const float* rt = &sR[tid][t * 8];
      const float* ro = &sR[tid][(t ^ 1) * 8];
      float mn = 0.f, mx = 0.f;
      for (int l = 0; l < LM; ++l) {
        const float r = fmaxf(rt[l], 0.f);
        mn = l ? fminf(mn, r) : r;
        mx = l ? fmaxf(mx, r) : r;
      }
      const bool deg = !(mx > mn);
      read_deg[(size_t)b * NB + n] = deg ? 1 : 0;
      const size_t o = ((size_t)b * NB + n) * LM;
      for (int l = 0; l < LM; ++l) {
        const float r = fmaxf(rt[l], 0.f), q = fmaxf(ro[l], 0.f);
        read_mm[o + l] = deg ? (unsigned char)0 : gc_maxmin(r, mn, mx);
        const float den = q + r;
        read_frac[o + l] = den > 0.f ? (unsigned char)(int)(255.f * (r / den)) : (unsigned char)0;   // FracTotalNormCam.normalize
      }
    }
    __syncthreads();
  }
}

extern "C" int da_gradcam_shape_ok(int NB, int Lm, int C) {
  return NB >= 1 && NB <= GC_MAX_NB && Lm >= 1 && Lm <= GC_MAX_LM && C >= 32 && C <= GC_MAX_C && C % 32 == 0;
}

extern "C" size_t da_gradcam_workspace(int B, int NB, int C) {
  if (B < 1 || NB < 1 || C < 1) return 0;
  return (size_t)B * ((C + GC_CC - 1) / GC_CC) * gc_record(NB) * sizeof(float);
}

extern "C" int da_gradcam(const float* F, const float* W, const float* bias, const int* target_in, int B, int NB, int Lm,
                          int C, float* workspace, float* logits, int* target, float* A, float* R, float* cam,
                          unsigned char* cam_maxmin, unsigned char* cam_degenerate, unsigned char* read_maxmin,
                          unsigned char* read_degenerate, unsigned char* read_frac, hipStream_t stream) {
  if (B < 1 || !da_gradcam_shape_ok(NB, Lm, C)) return DA_EINVAL;              // refusals first: no runtime call before them
  const int nchunk = (C + GC_CC - 1) / GC_CC;
  if ((size_t)B * NB * Lm * C >= ((size_t)1 << 31) || (size_t)B * nchunk >= ((size_t)1 << 31)) return DA_EINVAL;
  DA_ENTER();
  const dim3 grid1((unsigned)(B * nchunk)), block(256);
  switch (Lm) {
#define GC_CASE(n) \
  case n: hipLaunchKernelGGL(gradcam_partial_kernel<n>, grid1, block, 0, stream, F, W, workspace, NB, C, nchunk); break;
    GC_CASE(1) GC_CASE(2) GC_CASE(3) GC_CASE(4) GC_CASE(5) GC_CASE(6) GC_CASE(7) GC_CASE(8)
#undef GC_CASE
  }
  DA_CHECK_LAUNCH();
  hipLaunchKernelGGL(gradcam_finish_kernel, dim3((unsigned)B), block, 0, stream, (const float*)workspace, bias, target_in, NB, Lm,
                     nchunk, logits, target, A, R, cam, cam_maxmin, cam_degenerate, read_maxmin, read_degenerate, read_frac);
  DA_CHECK_LAUNCH();
  return DA_OK;
}
