/* deepards_hip.h -- C ABI of libdeepards_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the ONE hot path of hahnicity/deepards: cnn_linear / resnet18-1D /
 * densenet18-1D forward + backward over (sub_batch, 1, seq_len) windows.  The reference has no
 * FFI for this path: every op below replaces a stock torch.nn call reached from
 * deepards/models/{resnet,densenet,torch_cnn_linear_network}.py and train_ards_detector.py
 * (file:line cited per entry point).  The Python host in deepards_amd/ binds these with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless said otherwise; fp32 throughout
 *   - caller allocates outputs and workspaces; nothing is retained between calls
 *   - all launches go to `stream`, no hidden synchronisation, graph-capturable
 *   - return 0 on success, -1 on invalid arguments, >0 = hipError_t of a failed launch
 *   - activation layout "RLC": act[row][l][c] with channel pitch ld (floats, multiple of 4);
 *     a BatchNorm *window* = rows_per_window consecutive rows = Wn = rows_per_window*L positions
 */
#ifndef DEEPARDS_HIP_H
#define DEEPARDS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* da_stream_t; /* == hipStream_t */

int da_version(void);

/* Activation storage type.  `da_act_t*` parameters below are RLC activation / activation-gradient tensors whose element
   type is float (default) or bf16 (after da_set_act_dtype(1): BASELINE's bf16 configs -- every tensor between two
   kernels of the breath block is then stored in bf16; statistics, sums, features, parameters and their gradients stay
   float, all arithmetic is fp32 or bf16-MFMA with fp32 accumulation).  Pitches (`ld*`) count ELEMENTS.  The setting is
   process-wide and not thread-safe: set it before the step is built.  Entry points that take `float*` activations
   (the fp32 conv kernels, concat / slice / dropout) return -1 while bf16 is selected. */
typedef void da_act_t;
int da_set_act_dtype(int bf16);
int da_get_act_dtype(void);
/* sizeof of {da_wgrad_job, da_conv_job, da_wgrad_reduce_desc, da_repack_desc, da_bn_running_desc, da_bn_pgrad_desc} as the
   library was built (ABI drift check for bindings) */
void da_abi_sizes(int* out);
int da_sizeof_wgrad_reduce_desc(void);
int da_sizeof_bn_running_desc(void);
int da_sizeof_bn_pgrad_desc(void);
/* address of hipGetLastError as bound by this library (loader sanity check: same HIP runtime as the host) */
const void* da_hip_runtime_symbol(void);

/* ---- Conv1d as implicit GEMM on the fp32 matrix cores ------------------------------------
 * replaces nn.Conv1d fwd + dgrad: resnet.py:5-8 (conv2x2), :16-19,:126-128 (BasicBlock convs,
 * 1x1 s2 downsample); densenet.py:25-32 (1x1 bottleneck, k3 growth), :75-76 (transition conv).
 * Y[row][j*dst_stride+dst_off][n] (+)= sum_t sum_c X[row][j*src_stride+src_off[t]][c] *
 * Wp[wtap[t]][n][c],  j in [0,Lm); reads outside [0,Lsrc) are zero.  Wp: packed [tap][N][C].
 * C % 32 == 0, N % 32 == 0, ntaps <= 3.  src_off / wtap are HOST int arrays. */
int da_conv_gemm(const float* x, const float* w, float* y, int rows, int Lm, int Lsrc, int ldx, int C,
                 int Ldst, int ldy, int N, int dst_stride, int dst_off, int src_stride, int ntaps,
                 const int* src_off, const int* wtap, int accumulate, da_stream_t stream);

/* nn.Conv1d weight gradient (autograd of the calls above; train_ards_detector.py:163).
 * dW[co][ci][k] (torch layout) (+)= sum_positions dY[row][j*dy_stride+dy_off][co] *
 * X[row][j*src_stride+src_off[k]][ci].  workspace: da_conv_wgrad_workspace() bytes. */
size_t da_conv_wgrad_workspace(int rows, int Lm, int N, int C, int ntaps);
int da_conv_wgrad(const float* dy, const float* x, float* dw, float* workspace, int rows, int Lm, int Ldy,
                  int lddy, int N, int Lx, int ldx, int C, int dy_stride, int dy_off, int src_stride, int ntaps,
                  const int* src_off, int accumulate, da_stream_t stream);

/* comparison forms for tests: key 3 = 0: no half-tile tail round in the 64x64 conv launches; key 7 = 0: the dense-block
   weight gradients as one launch per tile shape; key 11 = 0: the F(4,3) conv / weight-gradient kernels compute the sixth
   product for every quad, also where L = 5, 6, 7 leaves it unused.  Any other key returns DA_EINVAL. */
int da_debug_set(int key, int value);

/* n <= 4 independent da_conv_gemm problems (jobs: HOST array, N % 64 == 0, disjoint outputs) in ONE launch: the
   stride-2 conv + 1x1 downsample of a block (same input), the even / odd sub-problems of a stride-2 data gradient */
typedef struct {
  const float* x; const float* w; float* y;
  int rows, Lm, Lsrc, ldx, C, Ldst, ldy, N, dst_stride, dst_off, src_stride, ntaps; int src_off[3]; int wtap[3];
  int accumulate;
  const float* x2; const float* w2; int tap_split;   /* optional: taps >= tap_split read x2 / w2 (same shapes): two
                                                        convolutions adding into one output as one contraction */
} da_conv_job;
int da_conv_gemm_multi(const da_conv_job* jobs, int n, da_stream_t stream);
/* k3 stride-1 pad-1 conv (forward, or data gradient with the transposed taps) as Winograd F(2,3): y (+)= conv(x);
   u = da_wino_weights() taps [4][N][C].  x: [rows][L][ldx] (C channels), y: [rows][L][ldy] (N channels).
   replaces nn.Conv1d(k=3, s=1, p=1) forward / input-grad, reference models/resnet.py:5-8,27-38, models/densenet.py:25-32 */
int da_conv3_winograd(const float* x, const float* u, float* y, int rows, int L, int ldx, int C, int ldy, int N,
                      int accumulate, da_stream_t stream);
/* tuning / tests: 0 = the partly filled last round of tiles is NOT cut into split-K half tiles (1 = default);
   2 / 3 = da_conv3_winograd4 with a K step of 32 / 16 (default) channels */
int da_wino_debug_tail(int on);
/* u[4][co][ci] (transpose = 0, forward) or u[4][ci][co] (transpose = 1, data gradient) from w[co][ci][3] */
int da_wino_weights(const float* w, float* u, int co, int ci, int transpose, da_stream_t stream);
/* Winograd F(4,3) variants (half the direct conv's MFMAs): u = 6 * N * C floats. */
int da_conv3_winograd4(const float* x, const float* u, float* y, int rows, int L, int ldx, int C, int ldy, int N,
                       int accumulate, da_stream_t stream);
int da_wino4_weights(const float* w, float* u, int co, int ci, int transpose, da_stream_t stream);

/* ---- bf16 matrix arithmetic for the k3 s1 p1 convs (BASELINE config C3) ----------------------
 * same nn.Conv1d calls as da_conv3_winograd (resnet.py:5-8,27-38): fp32 activations in and out, rounded to bf16
 * (nearest-even) on the way into LDS, bf16 taps wpk [3][N][C] from da_pack_conv3_bf16, v_mfma_f32_32x32x16_bf16 with
 * fp32 accumulation.  C % 32 == 0, N % 64 == 0.  wf [3][Co][Ci] forward taps, wd [3][Ci][Co] data-gradient taps
 * (reversed); either may be NULL. */
int da_conv3_bf16(const da_act_t* x, const void* wpk, da_act_t* y, int rows, int L, int ldx, int C, int ldy, int N,
                  int accumulate, da_stream_t stream);
/* da_conv3_bf16 with a BatchNorm (windows of R rows, R * L >= 130) folded into either end -- resnet.py:27-33 conv1 -> bn1 ->
 * relu -> conv2 without a pass for bn1.  stat_part != NULL: the statistics records of y AS STORED
 * (da_stat_records_floats(rows * L, N) floats, units = positions) from the epilogue.  in_pend != NULL: x is a raw conv output
 * with records in_pend; relu(gamma (x - mean) invstd + beta) is applied while x is staged and (mean, invstd) are published to
 * in_mean / in_invstd [rows / R][C] (the backward and the running statistics read them). */
int da_conv3_bf16_bn(const da_act_t* x, const void* wpk, da_act_t* y, int rows, int L, int ldx, int C, int ldy, int N, int R,
                     const float* in_pend, float* in_mean, float* in_invstd, const float* gamma, const float* beta, float eps,
                     float* stat_part, da_stream_t stream);
int da_pack_conv3_bf16(const float* w, void* wf, void* wd, int co, int ci, da_stream_t stream);
/* ---- fp32 convolutions on the bf16 matrix cores with PRE-SPLIT operands (conv_x3p.hip; conv arithmetic 'f32x3p', opt-in) ----
 * Every operand is split exactly into three bf16 terms and a product taken as six bf16 MFMA products (the dropped ones
 * are below one fp32 rounding); fp32 in / out / sums.  The "x3" activation format: an fp32 activation stored as its exact three-term bf16 split, per position C/16 groups of
 * [h 16 ch | m 16 ch | l 16 ch] bf16 (3 C bf16 = 6 C bytes per position, no pitch).  The BatchNorm / pool kernels in front
 * of a k3 s1 p1 conv store it (da_bn_fwd_x / da_bn_bwd_x / da_bn_relu_pool_fwd_x below), da_x3_split / da_x3_merge convert
 * fp32 <-> x3 for tests and boundaries.  da_conv3_x3p: same nn.Conv1d calls as da_conv3_bf16 (resnet.py:5-8,27-38), x in
 * x3 format, y fp32; wpk: the chunked split-bf16 pack -- (N/64) x (C/16) chunks of 18 KB laid out
 * [3 taps][2 halves of 32 outputs][3 terms][64 lanes][8 bf16] -- which da_repack_desc.points = 49 emits (Uf forward,
 * Ud data gradient; Co, Ci multiples of 64).  C % 16 == 0, N % 64 == 0. */
/* The stride-2 block entry on x3 operands (conv arithmetic 'f32x3p'), ONE launch each way:
 * forward   y1 = Conv1d(C, N, 3, stride 2, pad 1)(x) and yd = Conv1d(C, N, 1, stride 2)(x)   -- reference
 *           models/resnet.py:16-19 (conv3x3 stride 2), :27-29, :123-131 (downsample) on the same block input;
 * backward  dx = their two data gradients summed, every position written.
 * x3 / dy1_3 / dyd_3: x3 activations (da_x3_split); packs: da_repack_multi points 49 (forward / data-gradient side; the
 * 1x1 weights pack with K = 1 into tap 1 of the chunks).  Lin even; C, N multiples of 64. */
int da_conv_x3p_s2_fwd(const void* x3, const void* w1pk, const void* wdpk, float* y1, float* yd, int rows, int Lin, int C, int N,
                       da_stream_t stream);
int da_conv_x3p_s2_dgrad(const void* dy1_3, const void* w1pk, const void* dyd_3, const void* wdpk, float* dx, int rows, int Lout,
                         int N, int C, da_stream_t stream);
int da_conv3_x3p(const void* x, const void* wpk, float* y, int rows, int L, int C, int ldy, int N, int accumulate,
                 da_stream_t stream);
int da_x3_split(const float* x, int ld, void* out, size_t npos, int C, da_stream_t stream);
int da_x3_merge(const void* x, float* out, int ld, size_t npos, int C, da_stream_t stream);
/* da_conv_gemm_multi's contract with bf16 operands for the stride-2 block heads and 1x1 downsamples
 * (resnet.py:5-8,126-128), forward and data gradient: per job Lsrc == src_stride * Lm, source offsets within a span of
 * 2, x2 == NULL, w = bf16 [taps][N][C] (da_repack_desc.points = 16 emits them for K = 1 and K = 3); the jobs of a call
 * share src_stride (1 or 2); up to 4 per launch. */
int da_conv_bf16_multi(const da_conv_job* jobs, int n, da_stream_t stream);   /* jobs[].x / .y are da_act_t tensors here */
/* all weight-gradient GEMMs of a step in one launch per tile shape (jobs: HOST array); slabs only, reduce afterwards */
typedef struct {
  const float* dy; const float* x; float* workspace;
  int rows, Lm, Ldy, lddy, N, Lx, ldx, C, dy_stride, dy_off, src_stride, ntaps; int src_off[3];
  int winograd;   /* != 0: k3 s1 p1 job (N, C multiples of 64) in Winograd F(2,3) form (6: F(4,3) form);
                     16: bf16 operands; 49: split-bf16 (fp32-equivalent) products with dy AND x in the x3
                     format (see da_conv3_x3p; lddy == N, ldx == C), k3 s1 p1 only */
  /* dense-block operand forms of stride-1 jobs on the direct kernels (winograd == 0; see da_conv1x1_bn): xform = 1: X is
     relu(BatchNorm(x)) recomputed while staged from the statistics tables [rows * Lm / Wn][ldstat] (Wn >= 32);
     dy_half = 1: dY has Ldy = Lm / 2 positions per row, position j reads dy[j / 2] / 2 */
  int xform, dy_half, Wn, ldstat; const float* mean; const float* invstd; const float* gamma; const float* beta;
} da_wgrad_job;
int da_conv_wgrad_multi(const da_wgrad_job* jobs, int n, da_stream_t stream);  /* winograd == 16 jobs: dy / x are da_act_t tensors (the only kind accepted while bf16 is selected) */
/* the same call with the slab reductions chained: dws[i] = job i's gradient destination dW[co][ci][k] (or NULL); the
   reduction dws[i] (+)= sum of job i's slabs rides as the FIRST blocks of the NEXT launch of this call (memory-bound blocks
   beside matrix-bound ones, on slabs still in the Infinity Cache) and reduced[i] = 1; reduced[i] = 0: the caller still
   owes it (the jobs of the call's last launch, always) -- da_wgrad_reduce_multi / da_step_tail_multi.  The sums are the
   ones da_wgrad_reduce_multi forms, bit for bit.  (replaces nothing of its own in the reference: the reduction of
   loss.backward()'s conv weight gradients, train_ards_detector.py:161-173) */
int da_conv_wgrad_multi_reduce(const da_wgrad_job* jobs, int n, float* const* dws, int accumulate, int* reduced, da_stream_t stream);
/* host only (no HIP call): slabs[i] = the number of slabs (ntaps*N*C floats each) the matching launch will write into job
   i's workspace -- chained = 0: da_conv_wgrad_multi, chained = 1: da_conv_wgrad_multi_reduce.  It is the launch's own
   planning pass: the same shape validation (DA_EINVAL for the same jobs), the jobs' `workspace` pointers ignored (may be
   NULL).  Size every workspace from it and give the same figure to the job's reduction.  Unchained, slabs[i] depends on
   job i alone, so any subset of the array may be launched with the workspaces sized for the whole array; chained, it
   depends on the whole array (the dense-block jobs of a call with 8 or more of them share one launch and are planned as
   a batch; the winograd == 1 jobs of the launch's last, partly filled round run with half the pairs per split). */
int da_conv_wgrad_plan(const da_wgrad_job* jobs, int n, int chained, int* slabs);
/* the smallest N' >= N (a multiple of 32) for which da_conv_wgrad has an output tile against C input channels (host only,
 * from the plan the launch uses): N where the shape is taken, else the width to zero-pad dy's channels to; -1: none */
int da_conv_wgrad_padded_n(int N, int C);
/* deferred slab reduction: da_conv_wgrad with dw == NULL leaves da_conv_wgrad_splits() slabs in the workspace */
int da_conv_wgrad_splits(int rows, int Lm, int N, int C, int ntaps);
typedef struct { const float* slab; float* dw; int splits, ntaps, N, C; } da_wgrad_reduce_desc;
int da_wgrad_reduce_multi(const da_wgrad_reduce_desc* descs, int n, int accumulate, da_stream_t stream);
/* The tail of a training step in ONE launch: the slab reductions, every BatchNorm's dgamma / dbeta fold
   (da_bn_param_grad_multi) and running-statistics update (da_bn_running_multi), and -- stem_partial != NULL -- the fold of
   the stem's weight-gradient partials that da_stem_bwd(dw = NULL) left behind (da_stem_bwd_partials says where).  n <= 32
   reductions and <= 24 BatchNorms of each kind share the launch, anything else runs as the separate calls. */
struct da_bn_pgrad_desc_;
struct da_bn_running_desc_;
int da_step_tail_multi(const da_wgrad_reduce_desc* descs, int n, const struct da_bn_pgrad_desc_* pg, int npg,
                       const struct da_bn_running_desc_* run, int nrun, const float* stem_partial, int stem_nblk, int stem_n,
                       float* stem_dw, int accumulate, da_stream_t stream);

/* torch [Co][Ci][K] -> Wf [K][Co][Ci] (forward) and Wd [K][Ci][Co] (data gradient). */
int da_repack_conv_weight(const float* W, float* Wf, float* Wd, int Co, int Ci, int K, da_stream_t stream);
/* Uf / Ud (K == 3 only, may be NULL): the Winograd taps of da_wino_weights (points 0 / 4) or da_wino4_weights
   (points == 6) for the forward / data gradient; points == 16: Uf / Ud point at bf16 buffers and receive the tap packs
   of da_pack_conv3_bf16 (K = 3) or [1][Co][Ci] / [1][Ci][Co] (K = 1); Co and Ci multiples of 32 */
typedef struct { const float* W; float* Wf; float* Wd; float* Uf; float* Ud; int Co, Ci, K; int points; } da_repack_desc;
int da_repack_multi(const da_repack_desc* descs, int n, da_stream_t stream);

/* ---- stem: Conv1d(1, C0, k7, s2, p3)  resnet.py:86-87,142 ; densenet.py:118-119 ----------- */
int da_stem_conv_fwd(const float* x, const float* w, da_act_t* y, int rows, int Lin, int C0, int ldy,
                     da_stream_t stream);
size_t da_stem_wgrad_workspace(int rows, int C0);
int da_stem_conv_wgrad(const da_act_t* dy, int lddy, const float* x, float* dw, float* workspace, int rows, int Lin,
                       int C0, int accumulate, da_stream_t stream);
/* The same for the other first convolutions the constructors can select: x [rows][Cin][Lin] (the NCL rows the dataset
 * hands over), w [C0][Cin][K], pad = K / 2, Lin % stride == 0 -> y [rows][Lin / stride][ldy].  Instantiated shapes
 * (Cin, K, stride): (1, 7, 2) the default; (2, 7, 2) / (3, 7, 2) DenseNet(only_fft / with_fft) conv0, densenet.py:109-119;
 * (1, 3, 1) ResNet(double_conv_first).conv1_alt, resnet.py:88-89,145.  Any other shape returns -1. */
int da_stem_conv_fwd_g(const float* x, const float* w, da_act_t* y, int rows, int Lin, int Cin, int K, int stride, int C0,
                       int ldy, da_stream_t stream);
size_t da_stem_wgrad_workspace_g(int rows, int C0, int Cin, int K);
int da_stem_conv_wgrad_g(const da_act_t* dy, int lddy, const float* x, float* dw, float* workspace, int rows, int Lin,
                         int Cin, int K, int stride, int C0, int accumulate, da_stream_t stream);

/* ---- window-grouped train-mode BatchNorm1d (+ReLU, +residual) ------------------------------
 * resnet.py:27-38,143,152 ; densenet.py:23-29,72-74,146 ; per-window statistics because
 * torch_cnn_linear_network.py:108-113 calls breath_block(x[i]) one window at a time. */
/* descriptors for the batched small kernels: HOST arrays of these are passed, 32 served per launch */
typedef struct da_bn_running_desc_ {
  const float* mean; const float* invstd; float* running_mean; float* running_var;
  long long* num_batches_tracked; int W, C, Wn; float eps, momentum;
} da_bn_running_desc;
typedef struct da_bn_pgrad_desc_ { const float* s1; const float* s2; float* dgamma; float* dbeta; int W, C; } da_bn_pgrad_desc;

/* two-stage statistics: P chunks of `chunk` positions per window so that W*C/32*P blocks fill the chip.  W < 1, Wn < 1 or
 * C < 32 (less than one channel group) has no geometry: P = 0 and chunk = 0, and da_bn_workspace() returns 0; the entry
 * points that launch over it (da_bn_stats_partial, da_bn_stats_merge, da_stem_stats_partial) answer DA_EINVAL for C < 32. */
void da_bn_chunks(int W, int Wn, int C, int* P, int* chunk);
size_t da_bn_workspace(int W, int Wn, int C);      /* bytes of part[w][p][{mean,M2}][C] / backward scratch */
int da_bn_stats_partial(const da_act_t* x, int ld, int W, int Wn, int C, float* part, da_stream_t stream);
int da_bn_stats_merge(const float* part, int W, int Wn, int C, float eps, float* mean, float* invstd,
                      da_stream_t stream);
/* the reference's W sequential momentum-0.1 updates per BatchNorm in closed form; num_batches_tracked += W */
int da_bn_running_multi(const da_bn_running_desc* descs, int n, da_stream_t stream);
/* out = act(bn(x) (+res)); with part != NULL the chunk records are merged on the fly and mean/invstd WRITTEN */
int da_bn_apply(const da_act_t* x, int ldx, const da_act_t* res, int ldr, da_act_t* out, int ldo, int W, int Wn, int C,
                float* mean, float* invstd, const float* gamma, const float* beta, int relu, const float* part,
                float eps, da_stream_t stream);
/* statistics + normalisation in one call (mean/invstd [W][C] are OUTPUTS): one single-pass kernel when a window
   slab fits a block's registers (Wn <= 1280), else da_bn_stats_partial + da_bn_apply.  scratch: da_bn_workspace().
   replaces nn.BatchNorm1d(+ReLU)(+residual) forward, reference models/resnet.py:27-38, models/densenet.py:23-29 */
int da_bn_fwd(const da_act_t* x, int ldx, const da_act_t* res, int ldr, da_act_t* out, int ldo, int W, int Wn, int C,
              float* mean, float* invstd, const float* gamma, const float* beta, int relu, float eps, float* scratch,
              da_stream_t stream);
/* tests: on != 0 forces the two-stage kernels in da_bn_fwd / da_bn_bwd (both paths are checked against the oracle) */
int da_bn_debug_two_stage(int on);
/* tuning: blocks per launch the single-pass BatchNorm geometry aims for before its channel group stops shrinking
   (default 256 = one (window, 16-32 channel) slab per CU) */
int da_bn_debug_target_blocks(int blocks);
/* mask_mode 0: no ReLU; 1: ReLU, mask recomputed from bn(x); 2: ReLU, mask from `out` (residual).
 * scratch: da_bn_workspace() bytes.  ds: [2][W][C] per-window totals, always written.  dgamma/dbeta NULL:
 * fold ds later with da_bn_param_grad_multi. */
int da_bn_bwd(const da_act_t* dout, int ldd, const da_act_t* x, int ldx, const da_act_t* out, int ldo, da_act_t* dx, int lddx,
              da_act_t* gout, int ldg, int W, int Wn, int C, const float* mean, const float* invstd,
              const float* gamma, const float* beta, int mask_mode, float* scratch, float* ds, float* dgamma,
              float* dbeta, int accumulate, da_stream_t stream);
/* ReLU decisions as a bit mask, 64 bits per thread of the single-pass kernels (da_bn_mask_words() words; 0 = this shape
   takes the two-stage kernels, no mask form): da_bn_fwd_mask = da_bn_fwd(relu) + mask; da_bn_bwd_mask = da_bn_bwd of a
   ReLU'd BatchNorm(+residual) that reads the mask instead of the output tensor (mask_mode 2 reads `out` only for its sign) */
size_t da_bn_mask_words(int W, int Wn, int C);
int da_bn_fwd_mask(const da_act_t* x, int ldx, const da_act_t* res, int ldr, da_act_t* out, int ldo, int W, int Wn, int C,
                   float* mean, float* invstd, const float* gamma, const float* beta, float eps, float* scratch,
                   unsigned long long* mask, da_stream_t stream);
int da_bn_bwd_mask(const da_act_t* dout, int ldd, const da_act_t* x, int ldx, da_act_t* dx, int lddx, da_act_t* gout, int ldg, int W,
                   int Wn, int C, const float* mean, const float* invstd, const float* gamma, const float* beta,
                   float* scratch, float* ds, float* dgamma, float* dbeta, int accumulate,
                   const unsigned long long* mask, da_stream_t stream);
/* The block-output BatchNorm of the LAST BasicBlock with the head's AvgPool1d(L) folded in (resnet.py:33-38 into
   :112,159-160): da_bn_fwd_mask(relu) whose output map is never stored -- flat[W * Wn / L][C] (always float) receives the
   average over the L positions of every row, bit for bit what da_head_fwd pools from the stored map -- and its backward,
   da_bn_bwd_mask whose dout is dflat[rows][ldd] (float), the gradient of those pooled features.  da_bn_pool_ok: single-pass
   geometry, L | Wn, Wn <= 160. */
int da_bn_pool_ok(int W, int Wn, int C, int L);
int da_bn_fwd_pool(const da_act_t* x, int ldx, const da_act_t* res, int ldr, float* flat, int W, int Wn, int C, int L, float* mean,
                   float* invstd, const float* gamma, const float* beta, float eps, unsigned long long* mask, da_stream_t stream);
int da_bn_bwd_pool(const float* dflat, int ldd, const da_act_t* x, int ldx, da_act_t* dx, int lddx, da_act_t* gout, int ldg, int W,
                   int Wn, int C, int L, const float* mean, const float* invstd, const float* gamma, const float* beta, float* ds,
                   const unsigned long long* mask, da_stream_t stream);
/* da_bn_bwd_mask / da_bn_bwd_pair with the upstream gradient as TWO terms, dout + dout2 (resnet.py:33-38 backward: the gradient
   of a block's output = the next block's data-gradient conv output + its identity branch; summed here, the conv needs no
   accumulating epilogue).  da_bn_two_ok: single-pass geometry of at most 512 threads.  ds only. */
int da_bn_two_ok(int W, int Wn, int C);
int da_bn_bwd_mask2(const da_act_t* dout, int ldd, const da_act_t* dout2, int ldd2, const da_act_t* x, int ldx, da_act_t* dx, int lddx,
                    da_act_t* gout, int ldg, int W, int Wn, int C, const float* mean, const float* invstd, const float* gamma,
                    const float* beta, float* ds, const unsigned long long* mask, da_stream_t stream);
/* da_bn_bwd with dx = input gradient + add[pos][0:C] (pitch ldadd): a concatenation's pass-through gradient
   (densenet.py:41) joins in the same pass */
int da_bn_bwd_add(const da_act_t* dout, int ldd, const da_act_t* x, int ldx, const da_act_t* out, int ldo, da_act_t* dx, int lddx,
                  da_act_t* gout, int ldg, int W, int Wn, int C, const float* mean, const float* invstd, const float* gamma,
                  const float* beta, int mask_mode, float* scratch, float* ds, float* dgamma, float* dbeta,
                  int accumulate, const da_act_t* add, int ldadd, da_stream_t stream);
/* ---- the dense block as one design (reference models/densenet.py:18-44 _DenseLayer, :46-66 _DenseBlock, :68-81 _Transition)
 * One pitched buffer [rows][L][Cb] per block: the growth conv writes its 32 new channels at their offset (with F.dropout in
 * its epilogue), per-(window, channel) statistics live in ONE pitched table per block ([W][ldstat] mean / invstd) and are
 * reused by every later norm1 and the transition norm, and h = relu(norm1(x)) is never stored: the 1x1 conv applies it while
 * staging (da_conv1x1_bn), its weight gradient recomputes it (da_wgrad_job.xform), the BatchNorm backward takes the ReLU
 * decision from the same fused multiply-add (da_bn_bwd_ss).  fp32 activations, single-pass BatchNorm geometry
 * (da_bn_mask_words() > 0) only; callers keep the per-op entry points above for every other shape. */
/* statistics only: mean / invstd of x[:, 0:C] per window, written into the pitched tables */
int da_bn_stats_fused(const float* x, int ldx, int W, int Wn, int C, float* mean, float* invstd, int ldstat, float eps,
                      da_stream_t stream);
/* out[:, 0:C] = max(fmaf(x, gamma invstd, beta - mean gamma invstd), 0): the un-stored activation, for tests / explainers */
int da_bn_relu_ss(const float* x, int ldx, float* out, int ldo, int W, int Wn, int C, const float* mean, const float* invstd,
                  int ldstat, const float* gamma, const float* beta, da_stream_t stream);
/* backward of relu(norm(x)) (relu = 1: ReLU decision from the fused multiply-add form, the forward of da_conv1x1_bn;
 * relu = 2: from the sign of the stored output `out`, the forward of da_bn_fwd) or norm(x) (relu = 0): statistics from the
 * pitched tables; half_dout: dout has Wn / 2 positions per window, g[p] = dout[p / 2] / 2 (a transition's AvgPool1d(2,2) in
 * front of its conv); dx = input gradient (+ add[:, 0:C]; dx may alias add), then with drop_p > 0 the dropout mask
 * (da_dropout's, seed / salt, contiguous [W Wn][drop_g]) on dx's channels [C - drop_g, C); ds [2][W][C] window sums;
 * hout != NULL (relu = 1): the activation relu(norm(x)) itself, which the forward never stored, is written there for the
 * weight gradient of the conv behind it (the residual blocks' bn1 under da_conv3_bf16_bn) */
int da_bn_bwd_ss(const da_act_t* dout, int ldd, const da_act_t* x, int ldx, const da_act_t* out, int ldo, da_act_t* dx, int lddx,
                 const da_act_t* add, int ldadd, int W, int Wn, int C, const float* mean, const float* invstd, int ldstat,
                 const float* gamma, const float* beta, int relu, int half_dout, const long long* drop_seed, unsigned drop_salt,
                 float drop_p, int drop_g, float* ds, da_act_t* hout, int ldh, da_stream_t stream);
/* y[m][0:N] (pitch ldy) = sum_c w[n][c] relu(norm(x))[m][c], the activation applied while x (first C channels, pitch ldx) is
 * staged; pool != 0: the transition form, (h[2m] + h[2m+1]) / 2 in front of the conv (Lin even, Lin / 2 outputs per row).
 * w [N][C] = the torch weight of the k = 1 conv as it lies.  N % 64 == 0, C % 32 == 0, R * Lout >= 64.
 * replaces norm1 -> relu1 -> conv1 (densenet.py:23-26) and norm -> relu -> conv -> pool (:72-79) */
int da_conv1x1_bn(const float* x, int ldx, const float* w, float* y, int ldy, int rows, int R, int Lin, int C, int N, int pool,
                  float* mean, float* invstd, int ldstat, const float* gamma, const float* beta, const float* pend, int pend_c0,
                  long pend_units, int pend_Wu, float eps, float* out_part, da_stream_t stream);
/* the growth conv on the 1x1 conv's OUTPUT x with relu(norm2(x)) applied while x is staged (densenet.py:27-32 norm2 -> relu2
 * -> conv2: the activation is never stored): x [rows][L][C] contiguous, C <= 128; statistics of x from the records in_pend
 * (da_conv1x1_bn out_part of the conv in front), published to in_mean / in_invstd [rows / R][C]; dropout / output records as
 * da_conv3_winograd_drop.  R * ceil(L / 2) >= 64. */
int da_conv3_winograd_bn(const float* x, const float* u, float* y, int rows, int L, int C, int ldy, int N, int R,
                         const float* in_pend, float* in_mean, float* in_invstd, const float* gamma, const float* beta,
                         float eps, const long long* drop_seed, unsigned drop_salt, float drop_p, float* stat_part,
                         da_stream_t stream);
/* Statistics records: a kernel that WRITES activation channels can hand their per-window BatchNorm statistics over from its
 * epilogue -- per 64-unit tile and window slot (a tile touches <= 2 windows) the count, mean and centred second moment of
 * each channel: floats [tiles][2][{mean, M2}][N] then counts [tiles][2] (da_stat_records_floats).  The consuming
 * da_conv1x1_bn (pend != NULL: channels [pend_c0, C) of its input, pend_units units in windows of pend_Wu >= 64) merges
 * them per window in tile order (Chan's update, as da_bn_stats_merge) and publishes mean / invstd to the tables, which
 * every later kernel reads.  Producers: da_conv3_winograd_drop (units = output PAIRS, rows * ceil(L / 2)) and
 * da_conv1x1_bn(out_part != NULL) (units = its output positions). */
size_t da_stat_records_floats(long units, int N);
/* da_conv3_winograd + F.dropout(p) in the epilogue (mask of da_dropout on the contiguous [rows L][N] tensor), y at pitch ldy:
 * a _DenseLayer's growth conv storing its new features at their channel offset (densenet.py:30-40) */
int da_conv3_winograd_drop(const float* x, const float* u, float* y, int rows, int L, int ldx, int C, int ldy, int N,
                           const long long* drop_seed, unsigned drop_salt, float drop_p, float* stat_part, int R,
                           da_stream_t stream);     /* stat_part != NULL: + the records of y for windows of R rows */

int da_bn_param_grad_multi(const da_bn_pgrad_desc* descs, int n, int accumulate, da_stream_t stream);
/* Two BatchNorms of ONE geometry (W, Wn, C) in one launch -- a stride-2 BasicBlock entry (resnet.py:27-29,33-38,126-128):
 * forward: bn1 + ReLU on conv1's output and the downsample's BatchNorm on the 1x1 conv's (d[0], d[1] as da_bn_fwd /
 * da_bn_fwd_mask take them); backward: the block-output BatchNorm (bn2) and the downsample's take the SAME masked gradient
 * dout * [out > 0] (mask = the ReLU bit mask of da_bn_fwd_mask), ds_i [2][W][C] for da_bn_param_grad_multi.
 * Single-pass geometry only (da_bn_mask_words(W, Wn, C) > 0, else -1: the caller issues the two calls). */
typedef struct {
  const da_act_t* x; int ldx; const da_act_t* res; int ldr; da_act_t* out; int ldo; float* mean; float* invstd;
  const float* gamma; const float* beta; int relu; unsigned long long* mask;
} da_bn_fwd_desc;
typedef struct {
  const da_act_t* x; int ldx; da_act_t* dx; int lddx; const float* mean; const float* invstd; const float* gamma;
  const float* beta; float* ds;
} da_bn_bwd_desc;
int da_bn_fwd_pair(const da_bn_fwd_desc* d, int W, int Wn, int C, float eps, da_stream_t stream);
int da_bn_bwd_pair(const da_act_t* dout, int ldd, const da_bn_bwd_desc* d, int W, int Wn, int C,
                   const unsigned long long* mask, da_stream_t stream);
int da_bn_bwd_pair2(const da_act_t* dout, int ldd, const da_act_t* dout2, int ldd2, const da_bn_bwd_desc* d, int W, int Wn, int C,
                    const unsigned long long* mask, da_stream_t stream);      /* upstream gradient dout + dout2 (da_bn_bwd_mask2) */
/* The same BatchNorm forward / backward (resnet.py:27-38) in front of an x3 consumer (conv arithmetic 'f32x3', see
 * da_conv3_x3p): float in, and res_x3 / out_x3 / dx_x3 say which of `res`, `out`, `dx` are in the x3 format (their pitches are
 * ignored).  Single-pass geometry only (da_bn_mask_words() > 0; -1 otherwise); mask may be NULL (no ReLU bit mask wanted /
 * mask_mode 0 or 1 in the backward). */
int da_bn_fwd_x(const float* x, int ldx, const void* res, int ldr, void* out, int ldo, int W, int Wn, int C, float* mean,
                float* invstd, const float* gamma, const float* beta, int relu, float eps, unsigned long long* mask,
                int res_x3, int out_x3, da_stream_t stream);
int da_bn_bwd_x(const float* dout, int ldd, const float* x, int ldx, void* dx, int lddx, float* gout, int ldg, int W, int Wn,
                int C, const float* mean, const float* invstd, const float* gamma, const float* beta, int mask_mode,
                float* ds, const unsigned long long* mask, int dx_x3, da_stream_t stream);

/* ---- pools ------------------------------------------------------------------------------
 * stem BN+ReLU+{Max,Avg}Pool1d(3,2,1): resnet.py:100-104,152-153 ; densenet.py:120-123
 * pool_mode 0: max over {2j-1, 2j, 2j+1}, 1: avg (count_include_pad), out length (Lin - 1) / 2 + 1;
 * pool_mode 2: MaxPool1d(3, stride 2, ceil_mode=True) without padding (senet.py:245): max over {2j, 2j+1, 2j+2} clipped at
 * Lin, out length by ATen's ceil-mode rule = Lin / 2 (Lin >= 2).  The backward gives a window's gradient to its FIRST maximum
 * in every max mode, as ATen does.  Every pool entry point below (stored-map and recomputing stem) takes the three modes. */
int da_bn_relu_pool_fwd(const da_act_t* y, int ldy, da_act_t* out, int ldo, int rows, int R, int Lin, int C,
                        const float* mean, const float* invstd, const float* gamma, const float* beta,
                        int pool_mode, da_stream_t stream);
/* ... with the pooled output stored in the x3 format (float activations): layer1's input under conv arithmetic 'f32x3' */
/* The recomputing default stem (conv k7 s2 p3 on ONE input channel -> BatchNorm -> ReLU -> pool(3,2,1): reference
 * models/resnet.py:86-87,100-104,141-153, models/densenet.py:118-124): the conv output is 36.7 MB at B = 64 and costs 7 FMAs
 * an element, so these entry points take the RAW rows xrows (rows, Lin) and the weights wt (C, 1, 7) and recompute it wherever
 * it is needed instead of storing and re-reading it.  Forward: da_stem_stats_partial (chunk records as da_bn_stats_partial's
 * on the stored map, bit for bit) -> da_bn_stats_merge -> da_stem_bn_relu_pool_fwd (the pooled map, float or x3: bit for bit
 * da_stem_conv_fwd + da_bn_relu_pool_fwd).  Backward: da_stem_bwd = da_pool_bwd + da_bn_bwd + da_stem_conv_wgrad in two passes
 * over dout: dw (C, 1, 7) and ds (2, W, C) for da_bn_param_grad_multi; workspace da_stem_bwd_workspace() bytes.  out / dout
 * in the activation storage type (with bf16 storage the conv output, being recomputed in fp32, is never rounded -- the
 * stored-map stem rounds it); Lin even, C a multiple of 32 (statistics) with 2 C <= 256. */
int da_stem_stats_partial(const float* xrows, const float* wt, int rows, int R, int Lin, int C, float* part, da_stream_t stream);
int da_stem_bn_relu_pool_fwd(const float* xrows, const float* wt, da_act_t* out, int ldo, int rows, int R, int Lin, int C,
                             const float* mean, const float* invstd, const float* gamma, const float* beta, int pool_mode,
                             int out_x3, da_stream_t stream);
size_t da_stem_bwd_workspace(int rows, int C);
/* da_stem_bwd with dw == NULL leaves its weight-gradient partials [nblk][C * 7] at workspace + *offset (floats): fold them
   with da_step_tail_multi (the step's tail launch) or da_stem_wgrad_reduce */
int da_stem_bwd_partials(int rows, int R, int C, size_t* offset, int* nblk);
int da_stem_wgrad_reduce(const float* partial, int nblk, int n, float* dw, int accumulate, da_stream_t stream);
int da_stem_bwd(const da_act_t* dout, int ldd, const float* xrows, const float* wt, int rows, int R, int Lin, int C,
                const float* mean, const float* invstd, const float* gamma, const float* beta, int pool_mode, float* ds,
                float* dw, int accumulate, float* workspace, da_stream_t stream);
int da_bn_relu_pool_fwd_x(const float* y, int ldy, void* out, int rows, int R, int Lin, int C, const float* mean,
                          const float* invstd, const float* gamma, const float* beta, int pool_mode, da_stream_t stream);
int da_pool_bwd(const da_act_t* dout, int ldd, const da_act_t* y, int ldy, da_act_t* dz, int lddz, int rows, int R, int Lin,
                int C, const float* mean, const float* invstd, const float* gamma, const float* beta, int pool_mode,
                da_stream_t stream);
/* AvgPool1d(k, stride k): densenet.py:79 (k=2) ; AvgPool1d(7,1) on L=7: resnet.py:112,159, densenet.py:167,183 */
int da_avgpool_fwd(const float* x, int ldx, float* out, int ldo, int rows, int Lin, int k, int C,
                   da_stream_t stream);
int da_avgpool_bwd(const float* dout, int ldd, float* dx, int lddx, int rows, int Lin, int k, int C,
                   da_stream_t stream);
/* AvgPool1d(k, stride 1) on a map longer than k followed by x.view(x.size(0), -1) (resnet.py:159-160,
 * densenet.py:183-184 when seq_len > 224): feat[row][c * Lout + j], Lout = Lin - k + 1. */
int da_avgpool_slide_fwd(const da_act_t* x, int ldx, float* feat, int rows, int Lin, int k, int C, da_stream_t stream);
int da_avgpool_slide_bwd(const float* dfeat, da_act_t* dx, int lddx, int rows, int Lin, int k, int C,
                         da_stream_t stream);
/* The activation -> feature boundary, AvgPool1d(L, stride 1) on an L-long map + view (resnet.py:112,159-160,
 * densenet.py:167,183-184): x in the activation storage type, feat[row][c] always float; and its backward. */
int da_global_avgpool_fwd(const da_act_t* x, int ldx, float* feat, int rows, int L, int C, da_stream_t stream);
int da_global_avgpool_bwd(const float* dfeat, da_act_t* dx, int lddx, int rows, int L, int C, da_stream_t stream);


/* ---- head + loss ---------------------------------------------------------------------------
 * linear_final on view(-1) of the (NB,F) block: torch_cnn_linear_network.py:102,110-112 ;
 * BCEWithLogitsLoss (mean): train_ards_detector.py:530,929-930
 * bias / dbias may be null: a Linear(K, 2, bias=False) (PPNet.last_layer); with one, nothing changes. */
int da_linear2_fwd(const float* flat, const float* W, const float* bias, float* logits, int B, int K,
                   da_stream_t stream);
int da_bce_logits(const float* logits, const float* target, int n, float gscale, float* loss, float* dlogits,
                  da_stream_t stream);
int da_linear2_bwd(const float* dlogits, const float* flat, const float* W, float* dflat, float* dW, float* dbias,
                   int B, int K, int accumulate, da_stream_t stream);
/* The per-breath losses: logits [n_windows][nb][2] (nb = 1: a window-level head), target [n_windows][2] repeated over the
 * breaths, loss 1 float, dlogits [n_windows][nb][2] or null; one launch each, fixed-order sums, gscale on the gradient only.
 * ConfidencePenaltyLoss(beta), loss.py:26-35: BCE mean + beta * mean(softmax * log_softmax). */
int da_confidence_loss(const float* logits, const float* target, int n_windows, int nb, float beta, float gscale,
                       float* loss, float* dlogits, da_stream_t stream);
/* VacillatingLoss(alpha), loss.py:7-23: BCE mean + mean over [n_windows][2] of v(mean over the breaths of softmax);
 * alpha > 0, inf included; a window mean of exactly 0.5 (the reference raises) takes the left branch. */
int da_vacillating_loss(const float* logits, const float* target, int n_windows, int nb, float alpha, float gscale,
                        float* loss, float* dlogits, da_stream_t stream);
/* The head chain of CNNLinearNetwork in two launches instead of six: da_head_fwd = AvgPool1d(L,1) + view -> flat and the
 * row groups' shares `part` [B][da_head_groups(R, F)][2] of linear_final's two dot products (finish != 0, forward-only callers:
 * also logits and the BCEWithLogitsLoss mean); da_head_bwd = logits / loss terms / dlogits from `part`, linear + pool
 * backward in one kernel, then dW / dbias and the loss mean (resnet.py:112,159-160 / densenet.py:167,183-184;
 * torch_cnn_linear_network.py:102,110-112; train_ards_detector.py:530).  x / dx: the breath block's last map
 * [B * R][L][ld] in the activation storage type. */
int da_head_groups(int R, int F);
int da_head_fwd(const da_act_t* x, int ldx, const float* W, const float* bias, const float* target, float* flat, float* part,
                float* logits, float* loss, int B, int R, int L, int F, int finish, da_stream_t stream);
int da_head_bwd(const float* part, const float* bias, const float* target, const float* flat, const float* W, da_act_t* dx,
                int lddx, float* logits, float* dlogits, float* terms, float* dW, float* dbias, float* loss, int B, int R, int L,
                int F, float gscale, int accumulate, da_stream_t stream);
/* the same two calls on features da_bn_fwd_pool pooled already: flat_in [B * R][F] (float) in the place of the map (a map of
   ONE position), dflat [B * R][F] (float) in the place of dx -- whatever the activation storage type */
int da_head_flat_fwd(const float* flat_in, const float* W, const float* bias, const float* target, float* flat, float* part,
                     float* logits, float* loss, int B, int R, int F, int finish, da_stream_t stream);
int da_head_flat_bwd(const float* part, const float* bias, const float* target, const float* flat, const float* W, float* dflat,
                     float* logits, float* dlogits, float* terms, float* dW, float* dbias, float* loss, int B, int R, int F,
                     float gscale, int accumulate, da_stream_t stream);


/* ---- optimiser: clamp hook + SGD(momentum .9, nesterov, weight decay) / Adam, fused ----------
 * train_ards_detector.py:474-476 (clamp), :419-421 (optimisers).  gscale = 1/world_size after the
 * gradient all-reduce (the clamp runs AFTER the reduce, SURVEY.md finding 7). */
int da_clamp_sgd_nesterov(float* p, const float* g, float* buf, size_t n, float lr, float momentum,
                          float weight_decay, float clip, float gscale, int first, da_stream_t stream);
/* Adam's betas are doubles (as torch holds them): 1 - beta and the bias corrections 1 - beta^t are formed in double */
int da_clamp_adam(float* p, const float* g, float* m, float* v, size_t n, float lr, double beta1, double beta2,
                  float eps, int step, float clip, float gscale, da_stream_t stream);
/* the same with the step count in device memory (int64, incremented by the call): graph-replayable */
int da_clamp_adam_dev(float* p, const float* g, float* m, float* v, size_t n, float lr, double beta1, double beta2, float eps,
                      long long* step, float clip, float gscale, da_stream_t stream);

/* ---- device-resident window store: batch gather fused with the (x-mu)/std normalisation -------------------
 * ARDSRawDataset.__getitem__ dataset.py:1343-1404 (index map :1349-1350, normalisation :1364,1379 in float64)
 * + the .float() cast of train_ards_detector.py:150-152; replaces DataLoader/collate/H2D per step. */
int da_gather_normalize(const double* tiles, const int64_t* idx, double mu, double stdv, float* out, int B,
                        int tile_elems, da_stream_t stream);
/* windows with C <= 4 channels, [N][NB][C][L]: the flow channel plus the real / imaginary channels of its spectrum
 * (ARDSRawDataset._perform_fft dataset.py:1330-1341, selected by --with-fft / --only-fft / --fft-real-only,
 * train_ards_detector.py:228-230); every channel has its own factors (dataset.py:627-649).  mu / stdv: HOST arrays [C]. */
int da_gather_normalize_ch(const double* tiles, const int64_t* idx, const double* mu, const double* stdv, float* out, int B,
                           int NB, int C, int L, da_stream_t stream);
/* the same gather with the reference's two frequency filters behind the normalisation, before the cast: the 10th-order
 * Butterworth sosfilt (setup_butter_filter dataset.py:546-557, applied :1381-1382) as the causal sum
 * y[n] = sum_{m<=n} h[n-m] x[m] and the FFT band mask (:1393-1400) as the circular sum z[n] = sum_m g[(n-m) mod L] y[m], both
 * per row of L samples, every channel, in float64, ascending m, fma -- a repeat is bit-identical.  h, g: DEVICE arrays of L
 * doubles (impulse response of the cascade; real(ifft(mask))); either may be NULL, not both.  h: L <= 512; g: L == 224 (the
 * mask is built over fftfreq(224)); C <= 4; mu / stdv: HOST arrays [C].  Anything else: -1, out untouched. */
int da_gather_normalize_filter(const double* tiles, const int64_t* idx, const double* mu, const double* stdv, const double* h,
                               const double* g, float* out, int B, int NB, int C, int L, da_stream_t stream);
/* the whole item chain of ARDSRawDataset.__getitem__ (dataset.py:1375-1400) in one gather launch, float64 then the cast:
 * the normalisation -- padded != 0: (x - mu) / std where x != 0 and x / std where x == 0, the padded_breath_by_breath rule
 * (_get_padding_mask :1406-1409; a NaN counts as non-zero); padded == 0: (x - mu) / std, the bits of da_gather_normalize --,
 * the causal sum with h, post-hoc downsampling (:1384-1391: scipy.signal.resample to new_len samples, zeros behind them) as
 * r[n] = sum_m R[n][m] y[m], and the circular sum with g over the zero-padded row.  Ascending m, fma, one accumulator per
 * output -- a repeat is bit-identical.  h, rt, g: DEVICE arrays, each may be NULL (that stage is absent), all three too.
 * rt: [L][new_len] doubles, the TRANSPOSE of the (new_len, L) resampling matrix; NULL needs new_len == 0, otherwise
 * 1 <= new_len <= L.  L <= 512; g: L == 224; C <= 4; mu / stdv: HOST arrays [C].  Anything else: -1, out untouched. */
int da_gather_normalize_chain(const double* tiles, const int64_t* idx, const double* mu, const double* stdv, int padded,
                              const double* h, const double* rt, int new_len, const double* g, float* out, int B, int NB, int C,
                              int L, da_stream_t stream);
/* ---- sibling heads of CNNLinearNetwork (torch_cnn_linear_network.py:7-89) ---------------------- */
/* CNNLinearComprToRF: lower median over the NB breath rows of each window (torch.median(outputs, dim=1)[0], :47);
   x [B*NB][ld], out [B][F], idx [B][F] = selected row (for the backward); NB <= 64.  The mean of CNNLinearToMean
   (:25) is da_avgpool_fwd over the breath axis; the per-breath / double linear heads (:67,:87) are da_linear2_*. */
int da_window_median_fwd(const float* x, int ld, int B, int NB, int F, float* out, int* idx, da_stream_t stream);
int da_window_median_bwd(const float* dout, const int* idx, int B, int NB, int F, float* dx, int ld, da_stream_t stream);

/* ---- LSTM head of CNNLSTMNetwork (torch_cnn_lstm_combo.py:6-50): nn.LSTM(F, H, 1 layer, batch_first), gates i,f,g,o ---
   the recurrence only: the input projection gx = x W_ih^T and the weight / input gradients are 1x1-conv GEMMs */
int da_lstm_fwd(const float* gx, const float* whh, const float* bih, const float* bhh, const float* h0, const float* c0,
                float* hs, float* cs, float* gates, float* hT, float* cT, int B, int T, int H, da_stream_t stream);
int da_lstm_bwd(const float* dh_all, const float* whh, const float* hs, const float* cs, const float* gates,
                const float* h0, const float* c0, float* dgates, float* dwhh_part, int B, int T, int H,
                da_stream_t stream);
/* ---- waveform LSTM of the lstm_only networks (reference models/lstm_only.py:8-69 LSTMOnlyNetwork, :72-124
 * LSTMOnlyWithPacking): nn.LSTM(1, H, batch_first) over the T raw samples of each of N breath rows, zero initial state, gates
 * i,f,g,o.  x [N][T], w_ih [4H] (the (4H, 1) weight), w_hh [4H][H], b_ih / b_hh [4H].  H a multiple of 8 in [8, 64], T >= 1,
 * N >= 0; anything else: -1, outputs untouched.  There is no gx tensor and no stored gates: the forward keeps cs [N][T][H] and
 * lens [N] (int) beside its output hs [N][T][H]; the backward recomputes the gates with the forward's own arithmetic.
 * packed = 1 (LSTMOnlyWithPacking.pack_sequence, :100-113): step t of a row runs iff x[0] == 0 or no sample among
 * x[0 .. t-1] equals zero (-0.0 counts); lens = the steps run; hs at t >= lens is +0.0 and dhs there is never read.
 * packed = 0: lens = T.  Every sum runs in an order fixed by the shape; a sequence's hs does not depend on N or its index. */
int da_lstm_seq_block_seqs(int H);      /* sequences one block works on (tests put N around it); -1 for a refused H */
int da_lstm_seq_fwd(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int packed,
                    float* hs, float* cs, int* lens, int N, int T, int H, da_stream_t stream);
size_t da_lstm_seq_bwd_workspace(int N, int H);      /* bytes; 0 for a refused shape */
/* dhs [N][T][H] -> dw_ih [4H], dw_hh [4H][H], db [4H] (serves both biases; db2, if not NULL, receives it too), (+)= when
   accumulate; no input gradient */
int da_lstm_seq_bwd(const float* dhs, const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                    const float* hs, const float* cs, const int* lens, float* dw_ih, float* dw_hh, float* db, float* db2,
                    float* workspace, int accumulate, int N, int T, int H, da_stream_t stream);
/* the per-breath projection linear_breath_inst = Linear(K = T H -> F) over the N rows (lstm_only.py:26,65): y [N][F] =
 * hs [N][K] W [F][K]^T + bias.  K a multiple of 4, F a multiple of 16 up to 64; else -1.  The backward writes dhs [N][K] and
 * dW [F][K], dbias [F] (+)= when accumulate, partial sums over chunks of 32 rows folded in chunk order. */
int da_lstm_seq_proj_fwd(const float* hs, const float* W, const float* bias, float* y, int N, int K, int F, da_stream_t stream);
size_t da_lstm_seq_proj_bwd_workspace(int N, int K, int F);
int da_lstm_seq_proj_bwd(const float* dy, const float* hs, const float* W, float* dhs, float* dW, float* dbias, float* workspace,
                         int accumulate, int N, int K, int F, da_stream_t stream);

/* ---- nested networks: whole-patient recurrences (csrc/seq_wide.hip; reference models/cnn_to_nested_layer.py:
 * nn.RNN(128, 128) / nn.LSTM(128, 128), batch_first, zero initial state, over the W window vectors of one patient).
 * kind 0: tanh RNN (G = H), kind 1: LSTM (G = 4H, gate order i,f,g,o).  gx [S][T][G] = x W_ih^T for all steps (a GEMM outside),
 * w_hh [G][H], b_ih / b_hh [G].  One workgroup per sequence holds w_hh in registers for all T steps.  H == 128, T >= 1,
 * S >= 0; anything else: -1, outputs untouched.  Forward: hs [S][T][H]; the LSTM also keeps cs [S][T][H] and its activated
 * gates [S][T][H][4] (unit-major) for the backward.  Backward: dhs [S][T][H] -> the pre-activation gradient dz [S][T][G]
 * (torch's row order); dW_ih, dW_hh, both bias gradients and dx are GEMMs / row sums of dz the caller runs afterwards.  No
 * gradient into the initial state.  Every sum in an order fixed by H; a sequence's bits do not depend on S or its index. */
int da_seqw_shape_ok(int kind, int H, int T);          /* 1 / 0, launches nothing */
int da_seqw_rnn_fwd(const float* gx, const float* w_hh, const float* b_ih, const float* b_hh, float* hs, int S, int T, int H,
                    da_stream_t stream);
int da_seqw_rnn_bwd(const float* dhs, const float* w_hh, const float* hs, float* dz, int S, int T, int H, da_stream_t stream);
int da_seqw_lstm_fwd(const float* gx, const float* w_hh, const float* b_ih, const float* b_hh, float* hs, float* cs, float* gates,
                     int S, int T, int H, da_stream_t stream);
int da_seqw_lstm_bwd(const float* dhs, const float* w_hh, const float* cs, const float* gates, float* dz, int S, int T, int H,
                     da_stream_t stream);

/* ---- cnn_transformer head: one Block of Transformer (reference models/transformer.py:13-88; CNNTransformerNetwork
 * models/cnn_transformer.py:8-44) in three fp32 launches.  x, y [B][T][D]; `params` = the block's sixteen parameter
 * pointers in named_parameters() order (q / k / v / joint_linear weight, bias; attention_norm; ff.0; ff.2; ff_norm), each
 * 16-byte aligned; 4 heads.  T in [1, 64], D a multiple of 64 up to 2048, H a multiple of 8 in [8, 64]; else -1.
 * Dropout (transformer.py:78-79,87-88): the mask of da_dropout on the contiguous [B T][D] tensor, (seed, salt1) behind
 * the attention, (seed, salt2) behind the feed-forward; p == 0: none (seed may be NULL).
 * forward (transformer.py:34-56,86-88): saves q, k, v, hid [B][T][H], the attention weights aw [B][4][T][T] and
 * stats [B][T][4] = {mean, rstd} of attention_norm then of ff_norm */
int da_tfm_block_fwd(const float* x, const float* const* params, float* y, float* q, float* k, float* v, float* aw, float* hid,
                     float* stats, int B, int T, int D, int H, const int64_t* seed, unsigned salt1, unsigned salt2, float p,
                     da_stream_t stream);
/* the form the forward and the data backward take at (T, D, H), by the expressions their launches use: tokens a wave works
 * on per pass and bytes of dynamic LDS (at most 160 KB for every accepted shape); launches nothing; -1 for a refused shape */
int da_tfm_block_form(int T, int D, int H, int* tokens_fwd, int* tokens_bwd, size_t* lds_fwd, size_t* lds_bwd);
/* data backward: dy -> dx, and what da_tfm_block_pgrad reads: the gradients at the q / k / v / ff.0 outputs (dq, dk, dv, dhid
 * [B][T][H], dhid behind the ReLU), at the two LayerNorm inputs (da1, da2 [B][T][D]) and the re-joined heads wv [B][T][H] */
int da_tfm_block_bwd(const float* dy, const float* x, const float* const* params, const float* q, const float* k, const float* v,
                     const float* aw, const float* hid, const float* stats, float* dx, float* dq, float* dk, float* dv,
                     float* dhid, float* da1, float* da2, float* wv, int B, int T, int D, int H, const int64_t* seed,
                     unsigned salt1, unsigned salt2, float p, da_stream_t stream);
/* parameter backward: grads[16] (the order of `params`) (+)= the block's parameter gradients; every sum in a fixed order */
int da_tfm_block_pgrad(const float* dy, const float* x, const float* const* params, const float* hid, const float* stats,
                       const float* wv, const float* dq, const float* dk, const float* dv, const float* dhid, const float* da1,
                       const float* da2, float* const* grads, int accumulate, int B, int T, int D, int H, const int64_t* seed,
                       unsigned salt1, unsigned salt2, float p, da_stream_t stream);

/* out[n] (+)= column sums of m [rows][n] in a fixed order */
int da_reduce_rows(const float* m, int rows, int n, float* out, int accumulate, da_stream_t stream);

/* ---- Squeeze-and-Excitation tail of an SE-ResNet BasicBlock (senet.py:15-34 SEModule, :52-68 SEBasicBlock.forward) --------
 *     out = relu(z * s + res),  z = bn2(y2),  s = sigmoid(fc2(relu(fc1(mean_L z))))  per (row, channel)
 * float activations (rows, L, C); BatchNorm windows of R rows, mean / invstd (rows / R, C) from da_bn_stats_fused or
 * da_bn_stats_partial + da_bn_stats_merge.  z = fmaf(y2, gamma invstd, beta - mean gamma invstd) is never stored: forward and
 * backward recompute it from y2 with the same fused multiply-add.  w1 (Cr, C), b1 (Cr), w2 (C, Cr), b2 (C): fc1 / fc2 of the
 * module.  Shapes: C in {64, 128, 256, 512}, Cr a multiple of 16 dividing 256 with C Cr >= 1024 (C / 4 for the four
 * stages), any L >= 1, any rows, R dividing rows; anything else -> DA_EINVAL.  float storage only.  Every sum runs in an
 * order fixed by the shape (no atomics): the same bits every call.
 *   da_se_gate_fwd    one launch: pool (rows, C) = the affine of mean_L(y2), hid (rows, Cr), s (rows, C), kept for the backward
 *   da_se_scale_fwd   out = max(fmaf(z, s, res), 0); mask: rows L C / 8 bytes, bit (i % 8) of byte i / 8 = out[i] > 0
 *   da_se_bwd_reduce  g = dout . mask (written: the residual's gradient) and dsum[row][c] = sum_l g z
 *   da_se_gate_bwd    dpool (rows, C) and the parameter gradients dw1 / db1 / dw2 / db2 (+= when accumulate): partials over
 *                     chunks of C / 2 rows summed in row order, folded in chunk order; workspace da_se_gate_bwd_workspace() bytes
 *   da_se_bwd_scale   dz = fmaf(g, s, dpool / L): what da_bn_bwd (mask_mode 0) of bn2 takes */
int da_se_gate_fwd(const float* y2, int rows, int R, int L, int C, int Cr, const float* mean, const float* invstd,
                   const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2, const float* b2,
                   float* pool, float* hid, float* s, da_stream_t stream);
int da_se_scale_fwd(const float* y2, const float* res, float* out, void* mask, int rows, int R, int L, int C, const float* mean,
                    const float* invstd, const float* gamma, const float* beta, const float* s, da_stream_t stream);
int da_se_bwd_reduce(const float* dout, const void* mask, const float* y2, float* g, float* dsum, int rows, int R, int L, int C,
                     const float* mean, const float* invstd, const float* gamma, const float* beta, da_stream_t stream);
size_t da_se_gate_bwd_workspace(int rows, int C, int Cr);
int da_se_gate_bwd(const float* dsum, const float* s, const float* hid, const float* pool, const float* w1, const float* w2,
                   float* dpool, float* dw1, float* db1, float* dw2, float* db2, int accumulate, float* workspace, int rows, int C,
                   int Cr, da_stream_t stream);
int da_se_bwd_scale(const float* g, const float* s, const float* dpool, float* dz, int rows, int L, int C, da_stream_t stream);

/* ---- the same tail at an SE-ResNet Bottleneck's width (senet.py:15-34 SEModule, :71-95 Bottleneck.forward, :122-144
 * SEResNetBottleneck; se_resnet50 / 101 / 152 :351-372): the gate acts on 4 planes channels with reduction 16 --------------
 *     out = relu(z * s + res),  z = bn3(y3),  s = sigmoid(fc2(relu(fc1(mean_L z))))  per (row, channel)
 * Shapes: C % 64 == 0, 64 <= C <= 2048, Cr % 16 == 0, 16 <= Cr <= 128 (da_se_wide_shape_ok), any L >= 1, rows L and rows C below 2^31, R dividing
 * rows; anything else -> DA_EINVAL before any launch.  float storage only; z is never stored; no atomics, every sum in an
 * order fixed by the shape.
 *   da_se_wide_stats      one kernel over y3 (each row slice read twice by its block, the second time from the cache): rowsum (rows, C) = sum_l y3 and mean / invstd (rows / R, C) (row moments merged in
 *                         row order); workspace rows C floats.  replaces bn3's statistics and SEModule.avg_pool, senet.py:28,88
 *   da_se_wide_gate_fwd   three launches: pool = fmaf(rowsum / L, sc, sh) elementwise, then per tile of 32 rows hid = relu(pool
 *                         W1^T + b1) and s = sigmoid(hid W2^T + b2) as GEMMs on the fp32 matrix cores (senet.py:29-32), each
 *                         weight read once per row tile; the map itself is not read
 *   da_se_wide_scale_fwd, da_se_wide_bwd_scale   da_se_scale_fwd / da_se_bwd_scale's kernels at these widths (senet.py:33,93-94)
 *   da_se_wide_bwd_reduce g = dout . mask and dsum[row][c] = sum_l g z
 *   da_se_wide_gate_bwd   dpool and dw1 / db1 / dw2 / db2 (+= when accumulate): GEMMs with K = rows over chunks of
 *                         da_se_wide_chunk_rows() rows, folded in chunk order; workspace da_se_wide_gate_bwd_workspace() bytes */
int da_se_wide_shape_ok(int C, int Cr);
int da_se_wide_stats(const float* y3, int rows, int R, int L, int C, float eps, float* mean, float* invstd, float* rowsum,
                     float* workspace, da_stream_t stream);
int da_se_wide_gate_fwd(const float* rowsum, int rows, int R, int L, int C, int Cr, const float* mean, const float* invstd,
                        const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2, const float* b2,
                        float* pool, float* hid, float* s, da_stream_t stream);
int da_se_wide_scale_fwd(const float* y3, const float* res, float* out, void* mask, int rows, int R, int L, int C,
                         const float* mean, const float* invstd, const float* gamma, const float* beta, const float* s,
                         da_stream_t stream);
int da_se_wide_bwd_reduce(const float* dout, const void* mask, const float* y3, float* g, float* dsum, int rows, int R, int L,
                          int C, const float* mean, const float* invstd, const float* gamma, const float* beta, da_stream_t stream);
int da_se_wide_chunk_rows(void);
size_t da_se_wide_gate_bwd_workspace(int rows, int C, int Cr);
int da_se_wide_gate_bwd(const float* dsum, const float* s, const float* hid, const float* pool, const float* w1, const float* w2,
                        float* dpool, float* dw1, float* db1, float* dw2, float* db2, int accumulate, float* workspace, int rows,
                        int C, int Cr, da_stream_t stream);
int da_se_wide_bwd_scale(const float* g, const float* s, const float* dpool, float* dz, int rows, int L, int C, da_stream_t stream);

/* ---- the pooled stages and the feature layout of the VGG backbones (vgg.py:37-50 make_layers, :15,20-24) --------------------
 *     out[row][j][c] = max(relu(z[2j]), relu(z[2j + 1])),  z = bn(y) = fmaf(y, gamma invstd, beta - mean gamma invstd),  j < Lin / 2
 * float activations, y [rows][Lin][ldy] the stored conv output (WITHOUT the conv bias: BN(conv + b) == BN(conv)), BatchNorm
 * windows of R rows, mean / invstd (rows / R, C).  relu(z) and its gradient dz are never stored.  MaxPool1d(2, 2) floors: the
 * last position of an odd row belongs to no pair -- dz = 0 there, but dy is not (n = R Lin is the full window).  The pool gives
 * a pair's gradient to its first maximum.  Shapes: C a multiple of 32, Lin >= 2, R dividing rows, ldy >= C a multiple of 4,
 * rows Lin ldy < 2^32; anything else -> DA_EINVAL.  float storage only.  Sums in an order fixed by the shape (no atomics).
 *   da_bn_relu_maxpool2_fwd   one pass
 *   da_bn_relu_maxpool2_bwd   dout [rows][Lin / 2][C] -> dy [rows][Lin][C], ds [2][W][C] (sum dz, sum dz xhat per window, for
 *                             da_bn_param_grad_multi); workspace: da_bn_relu_maxpool2_bwd_workspace() bytes
 *   da_bn_mean_bias           mean_b[w][c] = mean[w][c] + bias[c]: the batch mean of conv + b, which da_bn_running_multi takes so
 *                             that running_mean is the reference's; dbias (or NULL): C floats set to 0, the conv bias's gradient
 *   da_adaptive_avgpool_flat_fwd / _bwd   AdaptiveAvgPool1d(Lout) + view(N, -1): feat[row][c Lout + i] = mean of
 *                             x[row][floor(i Lin / Lout) : ceil((i + 1) Lin / Lout)][c]; any Lin, Lout >= 1 (Lin < Lout repeats) */
int da_bn_relu_maxpool2_fwd(const float* y, int ldy, float* out, int rows, int R, int Lin, int C, const float* mean,
                            const float* invstd, const float* gamma, const float* beta, da_stream_t stream);
size_t da_bn_relu_maxpool2_bwd_workspace(int rows, int R, int Lin, int C);
int da_bn_relu_maxpool2_bwd(const float* dout, const float* y, int ldy, float* dy, float* ds, float* workspace, int rows, int R,
                            int Lin, int C, const float* mean, const float* invstd, const float* gamma, const float* beta,
                            da_stream_t stream);
int da_bn_mean_bias(const float* mean, const float* bias, float* mean_b, int W, int C, float* dbias, da_stream_t stream);
int da_adaptive_avgpool_flat_fwd(const float* x, float* feat, int rows, int Lin, int Lout, int C, da_stream_t stream);
int da_adaptive_avgpool_flat_bwd(const float* dfeat, float* dx, int rows, int Lin, int Lout, int C, da_stream_t stream);

/* ---- the autoencoder's own layers (csrc/autoencoder.hip; reference models/autoencoder_cnn.py): BatchNorm + MaxPool1d(2) that
 * keeps its decisions, MaxUnpool1d(2), and ConvTranspose1d(64, 1, 3, padding=1) + MSELoss.  NO ReLU anywhere.
 * float activations [rows][L][C] channels-last, float storage only.  A pool decision is one bit per pooled element, set where
 * the SECOND member of the pair is strictly greater (a tie, -0.0 against +0.0 included, keeps the first), 32 channels to a
 * uint32: word ((row Lo + j) C + c) / 32, bit c % 32.  Shapes: C a multiple of 32, Lin even and >= 2, R dividing rows, ldy >= C a
 * multiple of 4, rows Lin ldy < 2^32; anything else, or a NULL operand, -> DA_EINVAL before any launch.  Every sum runs in an
 * order fixed by the shape (no atomics); each entry launches on `stream` only, allocates nothing and never synchronises.
 *   da_bn_maxpool2_idx_fwd   z = fmaf(y, gamma invstd, beta - mean gamma invstd) (never stored); out[j] = sel ? z[2j+1] : z[2j].
 *                            sel_in NULL: decides on z and writes sel; else takes sel_in's bits (sel NULL or a copy's destination)
 *   da_bn_maxpool2_idx_plan  chunk geometry of the backward, launching nothing: a window's R Lin / 2 pairs in `chunks` runs of
 *                            `chunk_pairs` (the last shorter), and the workspace bytes
 *   da_bn_maxpool2_idx_bwd   dz[2j + sel] = dout[j], the partner 0; then BatchNorm's backward: dy [rows][Lin][C] and
 *                            ds [2][W][C] (for da_bn_param_grad_multi), the window sums as chunk partials folded in chunk order
 *   da_unpool2_fwd / _bwd    out[2j + sel] = v[j] + bias[c] (bias NULL: none), the partner exactly +0.0, every element written;
 *                            dv[j] = dout[2j + sel]
 *   da_ae_out_fwd            v [rows][L / 2][64], u = unpool(v + bias3, sel1) formed on the fly:
 *                            recon[n][l] = bias4 + sum_{c,t} u[n][l + 1 - t][c] w4[c][0][t];  dr = 2 (recon - x) / (rows L);
 *                            loss[0] = mean (recon - x)^2 from per-block partials (da_ae_out_fwd_workspace bytes) in block order
 *   da_ae_out_bwd            dv[n][j][c] = sum_t dr[n][2j + sel - 1 + t] w4[c][t] (the gradient at v + bias3),
 *                            dw4[c][t] (+)= sum_{n,j} (v + bias3)[n][j][c] dr[n][2j + sel - 1 + t],  db4 (+)= sum dr; dr outside a
 *                            row counts as 0; block records (da_ae_out_bwd_workspace bytes) folded in block order */
int da_bn_maxpool2_idx_fwd(const float* y, int ldy, float* out, uint32_t* sel, const uint32_t* sel_in, int rows, int R, int Lin,
                           int C, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           da_stream_t stream);
int da_bn_maxpool2_idx_plan(int rows, int R, int Lin, int C, int* chunks, int* chunk_pairs, size_t* workspace);
size_t da_bn_maxpool2_idx_bwd_workspace(int rows, int R, int Lin, int C);
int da_bn_maxpool2_idx_bwd(const float* dout, const uint32_t* sel, const float* y, int ldy, float* dy, float* ds, float* workspace,
                           int rows, int R, int Lin, int C, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, da_stream_t stream);
int da_unpool2_fwd(const float* v, const float* bias, const uint32_t* sel, float* out, int rows, int Lo, int C, da_stream_t stream);
int da_unpool2_bwd(const float* dout, const uint32_t* sel, float* dv, int rows, int Lo, int C, da_stream_t stream);
size_t da_ae_out_fwd_workspace(int rows, int L);
size_t da_ae_out_bwd_workspace(int rows, int L);
int da_ae_out_fwd(const float* v, const float* bias3, const uint32_t* sel1, const float* w4, const float* bias4, const float* x,
                  float* recon, float* dr, float* partials, float* loss, int rows, int L, da_stream_t stream);
int da_ae_out_bwd(const float* dr, const float* v, const float* bias3, const uint32_t* sel1, const float* w4, float* dv, float* dw4,
                  float* db4, float* workspace, int rows, int L, int accumulate, da_stream_t stream);

/* ---- the UNet's layers between its convs (csrc/unet.hip; reference models/unet.py): bias + ReLU (no BatchNorm), ReLU +
 * MaxPool1d(2) that keeps the full-resolution map as the skip, ReLU + Upsample(x2, linear, align_corners=True), Conv1d(64, 1, 1)
 * + MSELoss.  float activations [rows][L][C] channels-last, float storage only; C a multiple of 32; an operand named with a pitch
 * may be C channels of a pitched buffer (ld >= C, ld % 4 == 0, rows L ld < 2^32); anything else, or a NULL operand, ->
 * DA_EINVAL before any launch.  relu(v) = v > 0 ? v : +0.0; no pool decision is stored (the winner is re-derived from the stored
 * activation: the second member only when strictly greater).  Every sum runs in an order fixed by the shape (no atomics); each
 * entry launches on `stream` only, allocates nothing and never synchronises.
 *   da_unet_plan                 blocks (of 256 threads) and workspace bytes of entry point `op` (0 ... 7, in the order below) on
 *                                (rows, L, C) with widest pitch ld, launching nothing; L as the entry point takes it
 *   da_unet_bias_relu            y = relu(y + bias) in place
 *   da_unet_bias_relu_pool2_fwd  y = relu(y + bias) in place (L even); pooled [rows][L / 2][C][j] = max(y[2j], y[2j+1])
 *   da_unet_relu_upsample2_fwd   x = relu(y + bias) (y [rows][L][C], x never stored), D = 2 L - 1: out [rows][2 L][ld_out],
 *                                out[2j+1] = fma((L-1-j)/D, x[j+1], ((L+j)/D) x[j]);  out[2j] = fma(j/D, x[j-1], ((D-j)/D) x[j])
 *   da_unet_relu_upsample2_bwd   dy[j] = [y + bias > 0] (((L+j)/D) d[2j+1] + ((D-j)/D) d[2j] + ((L-j)/D) d[2j-1] + ((j+1)/D) d[2j+2]),
 *                                the terms in that order, those outside the row left out
 *   da_unet_pool2_skip_bwd       dy[2j+w] = [a > 0] (dskip[2j+w] + dpooled[j]), dy[2j+1-w] = [a > 0] dskip[2j+1-w]; w = a[2j+1] > a[2j]
 *   da_unet_relu_bwd             dy = [a > 0] dout (dy may be dout)
 *   da_unet_out_fwd              a [rows][L][64]: recon[n][l] = bias + sum_c a[n][l][c] w[c];  dr = 2 (recon - x) / (rows L);
 *                                loss[0] = mean (recon - x)^2 from per-block partials (the plan's workspace) in block order
 *   da_unet_out_bwd              dy = dr w [a > 0];  dw[c] (+)= sum dr a[c],  db (+)= sum dr: block records folded in block order */
int da_unet_plan(int op, int rows, int L, int C, int ld, int* blocks, size_t* workspace);
int da_unet_bias_relu(float* y, int ld, const float* bias, int rows, int L, int C, da_stream_t stream);
int da_unet_bias_relu_pool2_fwd(float* y, int ld, const float* bias, float* pooled, int rows, int L, int C, da_stream_t stream);
int da_unet_relu_upsample2_fwd(const float* y, const float* bias, float* out, int ld_out, int rows, int L, int C, da_stream_t stream);
int da_unet_relu_upsample2_bwd(const float* d, int ld, const float* y, const float* bias, float* dy, int rows, int L, int C,
                               da_stream_t stream);
int da_unet_pool2_skip_bwd(const float* dpooled, const float* dskip, int ld, const float* a, int ld_a, float* dy, int rows, int L,
                           int C, da_stream_t stream);
int da_unet_relu_bwd(const float* dout, const float* a, int ld_a, float* dy, int rows, int L, int C, da_stream_t stream);
int da_unet_out_fwd(const float* a, const float* w, const float* bias, const float* x, float* recon, float* dr, float* partials,
                    float* loss, int rows, int L, da_stream_t stream);
int da_unet_out_bwd(const float* dr, const float* a, const float* w, float* dy, float* dw, float* db, float* workspace, int rows,
                    int L, int accumulate, da_stream_t stream);

int da_gather_rows(const float* src, const int64_t* idx, float* out, int B, int width, da_stream_t stream);

/* ---- batched Grad-CAM of a cnn_linear + DenseNet model from the norm5 map alone (gradcam.py:28-205) ----------------------
 * Behind `features` the head is relu -> AvgPool1d(Lm) -> view(-1) -> linear_final, so the guided gradient is closed form,
 * d out[k] / d F[n][l][c] = (F[n][l][c] > 0) W[k][n C + c] / Lm, and every CAM is a reduction over the map:
 *     P[n][c] = (1 / Lm) sum_l max(F, 0)        logits[k] = bias[k] + sum_{n,c} W[k][n C + c] P[n][c]
 *     m[n][c] = #{l : F[n][l][c] > 0}           wr_k[n][c] = W[k][n C + c] m[n][c] / Lm^2        ww_k[c] = (1 / NB) sum_n wr_k[n][c]
 *     R_k[n][l] = sum_c wr_k[n][c] F[n][l][c]   (generate_read_cam)        A_k[l] = sum_c ww_k[c] (1 / NB) sum_n F[n][l][c]   (generate_cam)
 * F (B NB, Lm, C) float, channels-last, WITHOUT the final ReLU; W (2, NB C), bias (2); target_in (B) int: 0 / 1 (any other
 * value >= 0 counts as 1) selects the class, < 0 the arg-max of logits (the first maximum, as np.argmax).  Outputs, t = target[b]:
 *     logits (B, 2), target (B) int, A (B, 2, Lm), R (B, 2, NB, Lm)                                    float
 *     cam (B, Lm) = max(A_t, 0)                                                                       UnNormalizedCam
 *     cam_maxmin (B, Lm), read_maxmin (B, NB, Lm): u = trunc(255 (r - min r) / (max r - min r)), r = max(v, 0) over l of A_t /
 *         of each row of R_t (MaxMinNormCam.normalize); where max r == min r -- the reference divides 0 by 0 and casts the NaN,
 *         which is platform-defined -- the bytes are 0 and cam_degenerate (B) / read_degenerate (B, NB) is 1 (else 0)
 *     read_frac (B, NB, Lm): u = trunc(255 rt / (ro + rt)) of the ReLU'd target / other class read CAMs, 0 where ro + rt == 0
 *         (FracTotalNormCam.normalize)
 * Shapes (da_gradcam_shape_ok): C % 32 == 0, 32 <= C <= 1920, 1 <= NB <= 1024, 1 <= Lm <= 8, B >= 1, B NB Lm C < 2^31; anything
 * else -> DA_EINVAL before any launch.  Two launches on `stream`, no atomics, no synchronisation, no allocation: every sum runs in
 * an order fixed by (NB, Lm, C), so a window's outputs are the same bits in any batch at any position.  workspace:
 * da_gradcam_workspace() bytes, written before it is read. */
int da_gradcam_shape_ok(int NB, int Lm, int C);
size_t da_gradcam_workspace(int B, int NB, int C);
int da_gradcam(const float* F, const float* W, const float* bias, const int* target_in, int B, int NB, int Lm, int C,
               float* workspace, float* logits, int* target, float* A, float* R, float* cam, unsigned char* cam_maxmin,
               unsigned char* cam_degenerate, unsigned char* read_maxmin, unsigned char* read_degenerate,
               unsigned char* read_frac, da_stream_t stream);

/* ---- the head of the 1-D ProtoPNet (models/protopnet1d/model.py:113-354; train_ards_detector.py:1194-1247) ----------------
 * All float32; z is the map [rows][L][D] behind the add-on layers, channels innermost, rows = B NB.  No atomics: every sum
 * runs in an order fixed by the shape, so a row's outputs are the same bits in any batch at any position.  Every entry returns
 * DA_EINVAL on a shape it does not take, before any launch.
 *
 * da_bias_act_fwd   y[m][n] = act(x[m][n] + bias[n]); act 0: ReLU, 1: sigmoid; N % 4 == 0, N <= 4096 (the add-on layers'
 *                   1x1 convolutions themselves are da_conv_gemm / da_conv_wgrad).  y may be x.
 * da_bias_act_bwd   dx = dy act'(y) from the stored y (dx null: skipped; dx may be dy), dbias[n] (+)= sum_m dx[m][n] (null:
 *                   skipped) through `workspace` (da_bias_act_bwd_workspace bytes, written before it is read).
 * da_proto_fwd      dist[row][p][l] = sum_c (z[row][l][c] - protos[p][c])^2 in the DIRECT form (never negative; exactly 0 for a
 *                   prototype that is bitwise a patch) -- null: not stored; min_d[row][p] = min_l, arg[row][p] the lowest l
 *                   attaining it, sim = log((min_d + 1) / (min_d + 1e-4)).  D % 32 == 0 up to 512, 2 <= P <= 64, 1 <= L <= 64,
 *                   rows >= 1, prototype kernel size 1.  da_proto_row_tile: the rows one block takes at (L, P).
 * da_proto_bwd      g = dmin + dsim * d sim / d min_d (either of dsim, dmin [rows][P] may be null, not both: the similarity's
 *                   derivative is folded in HERE, the loss's own min_d term comes in as dmin);
 *                   dz[row][l][c] = sum_p 2 g (z - protos[p]) at l == arg[row][p], 0 elsewhere -- every element written (null:
 *                   skipped); dprotos[p][c] (+)= sum_row 2 g (protos[p] - z[row][arg]) (null: skipped) through `workspace`
 *                   (da_proto_bwd_workspace bytes).
 * da_ppnet_loss     calc_loss without its l1 term: logits, target [B][2], min_d [B][NB P]; out[5] = total, cls, cluster,
 *                   separation, 0; dlogits [B][2], dmin_d [B][NB P] (null: skipped; every element written); P even; gscale on
 *                   the gradients only.  One launch. */
int da_bias_act_fwd(const float* x, const float* bias, float* y, int M, int N, int act, da_stream_t stream);
size_t da_bias_act_bwd_workspace(int M, int N);
int da_bias_act_bwd(const float* dy, const float* y, float* dx, float* dbias, int accumulate, float* workspace, int M, int N,
                    int act, da_stream_t stream);
int da_proto_shape_ok(int rows, int L, int D, int P);
int da_proto_row_tile(int L, int P);
int da_proto_fwd(const float* z, const float* protos, float* dist, float* min_d, int* arg, float* sim, int rows, int L, int D,
                 int P, da_stream_t stream);
size_t da_proto_bwd_workspace(int rows, int D, int P);
int da_proto_bwd(const float* dsim, const float* dmin, const float* min_d, const int* arg, const float* z, const float* protos,
                 float* dz, float* dprotos, int accumulate, float* workspace, int rows, int L, int D, int P,
                 da_stream_t stream);
int da_ppnet_loss(const float* logits, const float* target, const float* min_d, int B, int NB, int P, float max_dist,
                  float clust_lambda, float sep_lambda, float gscale, float* out, float* dlogits, float* dmin_d,
                  da_stream_t stream);
/* g[i] += weight_decay * p[i]: the L2 term torch.optim.Adam(weight_decay=...) adds to the gradient in front of its moments
 * (da_clamp_adam* take no weight decay; the ProtoPNet optimisers, train_ards_detector.py:1163-1191, give Adam one). */
int da_grad_add_decay(float* g, const float* p, size_t n, float weight_decay, da_stream_t stream);

/* ---- test epoch on the device: window predictions + per-patient vote table --------------------------------
 * CNNLinearModel._process_test_batch_results train_ards_detector.py:932-936 (outputs.argmax) and
 * DeepARDSResults.perform_patient_predictions metrics.py:572-604 (votes per pathology, pred_frac, majority). */
int da_vote_counts(const float* logits, const int64_t* group, int B, int n_groups, int* votes, int* pred,
                   da_stream_t stream);

/* _DenseLayer's dropout fused into its neighbours (densenet.py:38-41): concat with dropout on the new features, and
   the backward's slice of the concatenated gradient with the same mask (that of da_dropout on a contiguous tensor) */
int da_concat2_dropout(const float* a, int lda, int C1, const float* b, int ldb, int C2, float* out, int ldo, size_t npos,
                       const int64_t* seed, unsigned salt, float p, da_stream_t stream);
int da_slice_dropout(const float* src, int lds, int off, float* dst, int ldd, int C, size_t npos, const int64_t* seed,
                     unsigned salt, float p, da_stream_t stream);
/* ---- densenet helpers: torch.cat([x, new], 1) and F.dropout  densenet.py:36-40 -------------- */
int da_concat2(const float* a, int lda, int C1, const float* b, int ldb, int C2, float* out, int ldo, size_t npos,
               da_stream_t stream);
int da_slice_copy(const float* src, int lds, int off, float* dst, int ldd, int C, size_t npos, int accumulate,
                  da_stream_t stream);
int da_dropout(const float* x, float* y, size_t n, const int64_t* seed, unsigned salt, float p,
               da_stream_t stream);

/* ---- siamese pretraining (csrc/siamese.hip): the triplet draw and the |a - c| head ------------------------------------
 * models/siamese.py:56-83 (and its LSTM / Transformer siblings), dataset.py:1586-1591 (SiameseNetworkDataset.__getitem__).
 * da_siamese_draw   anchor [B] int64 absolute window indices into a store whose windows are sorted so that a patient's
 *                   windows are contiguous; pat_start / pat_count [N] int32 per WINDOW: first index and number of windows of
 *                   that window's patient (2 <= count < N).  out int64: [anchor | pos | anchor | neg] (4 B, literal != 0) or
 *                   [anchor | pos | neg] (3 B).  pos = anchor + 1, or anchor - 1 for the patient's last window;
 *                   r = mix32(mix32(seed, step), slot), off = (r M) >> 32 with M = N - count,
 *                   neg = off < start ? off : off + count -- uniform over the other patients' windows up to a relative bias of
 *                   M / 2^32.  Every index written lies in [0, N).  DA_EINVAL for N < 2, B < 1, a null pointer.
 * da_siamese_head_fwd   fa_pos, fc_pos, fa_neg, fc_neg [B NB][D] float rows of pitch ld (fa_pos == fa_neg: one shared
 *                   anchor); W1 [2][D], b1 [2], W2 [2][2 NB], b2 [2].  u [2][B NB][2] = W1 |fc - fa| + b1 per pair (pos, neg);
 *                   z [2][B][2] = W2 vec(u) + b2; loss[0] = mean BCE(z_pos, [0, 1]) + mean BCE(z_neg, [1, 0]) in the stable
 *                   max(z, 0) - z t + log1p(exp(-|z|)) form, each mean over 2 B elements.  Any D, NB, B >= 1; 16-byte loads when
 *                   D, ld are multiples of 4 and the pointers 16-byte aligned.  Two launches.
 * da_siamese_head_bwd   from the forward's u and z: dfc_* = sign(fc - fa) W1^T du (sign(0) = 0), dfa_* = -dfc_* -- with a shared
 *                   anchor dfa_pos = (-dfc_pos) + (-dfc_neg) and dfa_neg is not written (may be null); rows of pitch ldg, every
 *                   element of the D columns written.  dW1, db1, dW2, db2 (+)= with `accumulate`.  gscale multiplies the
 *                   gradients only.  `workspace`: da_siamese_head_bwd_workspace bytes, written before it is read.  No float
 *                   atomics: every sum's order depends on (B, NB, D) alone.  Two launches.
 * da_siamese_head_rows_per_block   rows of [B NB] one block of the two row kernels takes (tests place B NB around it). */
int da_siamese_draw(const int64_t* anchor, const int* pat_start, const int* pat_count, int64_t* out, int B, int N, unsigned seed,
                    unsigned step, int literal, da_stream_t stream);
int da_siamese_head_rows_per_block(void);
int da_siamese_head_fwd(const float* fa_pos, const float* fc_pos, const float* fa_neg, const float* fc_neg, int ld, const float* W1,
                        const float* b1, const float* W2, const float* b2, float* u, float* z, float* loss, int B, int NB, int D,
                        da_stream_t stream);
size_t da_siamese_head_bwd_workspace(int B, int NB, int D);
int da_siamese_head_bwd(const float* fa_pos, const float* fc_pos, const float* fa_neg, const float* fc_neg, int ld, const float* W1,
                        const float* W2, const float* u, const float* z, float* dfa_pos, float* dfc_pos, float* dfa_neg,
                        float* dfc_neg, int ldg, float* dW1, float* db1, float* dW2, float* db2, float* workspace, float gscale,
                        int accumulate, int B, int NB, int D, da_stream_t stream);

/* ---- grouped k3 convolution (csrc/conv_grouped.hip): conv2 of the SE-ResNeXt 32x4d bottleneck, models/senet.py:147-168 ----
 *     y[r][lo][co] = sum_{k < 3, j < cg} w[co][j][k] x[r][lo stride + k - 1][(co / cg) cg + j],   cg = C / 32, pad 1
 * float32, channels-last maps x (rows, L, C), y (rows, Lo, C) with Lo = (L - 1) / stride + 1, without a channel pitch; the
 * weight in torch's layout (C, cg, 3), no pack.  Shapes (da_gconv3_shape_ok): groups == 32, C in {128, 256, 512, 1024},
 * stride 1 / 2; any rows >= 1, L >= 1 with rows L C < 2^31.  Every pointer 16-byte aligned.  Pads are predicated, nothing
 * outside a map is read or written.  Each entry launches on `stream` only, allocates nothing and never synchronises.
 *   da_gconv3_plan    which = 0 forward, 1 data gradient, 2 weight gradient: grid[3], block[3], static LDS bytes and workspace
 *                     bytes of the launch, from the expressions the launch itself uses; launches nothing.  DA_EINVAL -- and
 *                     from the launch entries too, before anything is launched -- for a shape without a legal launch (not
 *                     shape_ok, rows or L < 1, a map of 2^31 elements or more, a grid dimension or LDS over the limits).
 *   da_gconv3_tiling  the same plan's tiles: positions of the destination map per tile (of one row), tiles a block walks (for
 *                     which = 2: tiles per partial chunk), tiles in all (rows * ceil(Ldst / positions)).
 *   da_gconv3_fwd     y, every element written.
 *   da_gconv3_dgrad   dx (rows, Lin, C) from dy (rows, Lo, C): every element written (zero where no tap reaches), or -- accumulate
 *                     -- added to.
 *   da_gconv3_wgrad   dw (C, cg, 3) (+)= sum over rows Lo positions: one partial per chunk of tiles into `workspace` (plan bytes,
 *                     written before it is read), folded by a second launch in an order fixed by the chunk count.  No atomics: the order is a function
 *                     of (rows, Lin, C, stride) alone, the same input gives the same bits. */
int da_gconv3_shape_ok(int C, int groups, int stride);
int da_gconv3_plan(int which, int rows, int L, int C, int stride, int* grid, int* block, size_t* lds, size_t* workspace);
int da_gconv3_tiling(int which, int rows, int L, int C, int stride, int* tile_positions, int* tiles_per_block, int* tiles);
int da_gconv3_fwd(const float* x, const float* w, float* y, int rows, int L, int C, int stride, da_stream_t stream);
int da_gconv3_dgrad(const float* dy, const float* w, float* dx, int rows, int Lin, int C, int stride, int accumulate,
                    da_stream_t stream);
int da_gconv3_wgrad(const float* dy, const float* x, float* dw, float* workspace, int rows, int Lin, int C, int stride,
                    int accumulate, da_stream_t stream);

/* ---- breath-metadata regression (csrc/regress.hip): the head of CNNRegressor, models/torch_cnn_bm_regressor.py -----------
 *     feat[r][c] = (sum_{p < 7} x[r][p][c]) / 7 (form 1: the map [R][7][F], position pitch ld) | x[r][c] (form 0: [R][F], row pitch ld)
 *     out[r][m]  = bias[m] + sum_c W[m][c] feat[r][c];    loss[0] = sum (out - target)^2 / (R M)
 *     d = 2 (out - target) gscale / (R M);  dfeat = W^T d (m rising) -> dx = dfeat / 7 at the seven positions | dflat;
 *     dW[m][c] (+)= sum_r d[r][m] feat[r][c];  db[m] (+)= sum_r d[r][m]
 * All float32; W [M][F], bias [M], target / out [R][M].  Shapes (da_regress_shape_ok): R in [1, 2^24], F in [1, 2^20], M in
 * [1, 16], form 0 / 1, 7 R F < 2^40; anything else, ld / ldf / ldg < F or a NULL operand -> DA_EINVAL before any launch.
 * 16-byte loads and stores when F and the pitches are multiples of 4 and the pointers 16-byte aligned; a scalar path
 * otherwise.  No float atomics: every sum's order is a function of (R, F, M, form) and of that path, the same bits every
 * call.  Each entry launches on `stream` only (two launches), allocates nothing and never synchronises.
 *   da_regress_fwd    form 1 writes feat [R][F] (what the backward reads instead of the map); form 0 writes none (feat may be
 *                     NULL: the backward takes x itself).  out and loss written.
 *   da_regress_bwd    feat: the forward's (ldf = F) or the flat operand (ldf = ld).  dx rows of pitch ldg (form 1: position
 *                     pitch), every element of the F columns written; dW, db (+)= with `accumulate`; gscale multiplies the
 *                     gradients only.  workspace: da_regress_workspace bytes (one partial [M][F] per row block), written before
 *                     it is read.
 *   da_regress_rows_per_block   rows one block of the two row kernels takes (tests place R around it). */
int da_regress_rows_per_block(void);
int da_regress_shape_ok(int R, int F, int M, int form);
size_t da_regress_workspace(int R, int F, int M);
int da_regress_fwd(const float* x, int ld, int form, const float* W, const float* bias, const float* target, float* feat,
                   float* out, float* loss, int R, int F, int M, da_stream_t stream);
int da_regress_bwd(const float* feat, int ldf, const float* W, const float* out, const float* target, float* dx, int ldg,
                   int form, float* dW, float* db, float* workspace, float gscale, int accumulate, int R, int F, int M,
                   da_stream_t stream);

/* ---- dynamic time warping (csrc/dtw.hip): dtw_lib.py's `dtw(x, y)` (dtwco's defaults as its documentation states them; never
 * compared with dtwco itself), P pairs per launch, and the ordered means dtw_lib takes of the distances --------------------
 *     c(i,j) = |x[i] - y[j]| (metric 0) | (x[i] - y[j])^2 (metric 1, the product rounded on its own);  +inf where band >= 0
 *              and |i - j| > band
 *     D(i,j) = c(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1)),  D(-1,-1) = 0, every other missing neighbour +inf;  dtw = D(n-1,m-1)
 * in the accumulation type (acc 0: float, 1: double), one IEEE operation per line: the result is defined bit for bit, does not
 * depend on the order of the cells, dtw(x,y) == dtw(y,x), dtw(x,x) == +0.  NaN input: unspecified.
 * Operands: two tables of rows, ta [Sa][lda] with n used columns and tb [Sb][ldb] with m (the same table is fine), each float
 * (a64 / b64 = 0) or double (1), pitches in elements and >= the length; pair p is row ia[p] of ta against row ib[p] of tb
 * (int32, device).  acc 0 takes float tables only; acc 1 widens float elements exactly.  Shapes (da_dtw_shape_ok):
 * 1 <= n, m <= da_dtw_max_len() = 4608; anything else, a pitch below the length, P < 1 or a NULL operand -> DA_EINVAL before
 * any launch, never truncated.  An index outside [0, Sa) / [0, Sb) gives NaN for its pair and reads nothing.  out [P] in the
 * accumulation type, every element written; a pair's result does not depend on P, on its position or on the other pairs.  No
 * atomics.  Each entry launches on `stream` only (one launch), allocates nothing and never synchronises.
 *   da_dtw_plan          out[7] = lanes of the 64 that hold columns, columns per lane (the class of m), steps of the wavefront
 *                        (n + lanes - 1), pairs (waves) per block, grid, threads per block, LDS bytes -- from the expressions
 *                        the launch itself uses; launches nothing.
 *   da_dtw_segment_mean  out[g] = (((0 + d[off[g]]) + d[off[g] + 1]) + ...) / (off[g+1] - off[g]) in double, index order, for the
 *                        G segments of the offsets [G + 1] (int32, device) over the distances d [P] (float, d64 = 0, or double);
 *                        an empty segment, or one that leaves [0, P], gives NaN.  One thread per segment. */
int da_dtw_max_len(void);
int da_dtw_shape_ok(int n, int m, int acc, int a64, int b64);
int da_dtw_plan(int n, int m, int P, int acc, int* out);
int da_dtw_pairs(const void* ta, int a64, int lda, int Sa, int n, const void* tb, int b64, int ldb, int Sb, int m, const int* ia,
                 const int* ib, int P, int acc, int metric, int band, void* out, da_stream_t stream);
int da_dtw_segment_mean(const void* dist, int d64, int P, const int* offsets, int G, double* out, da_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPARDS_HIP_H */
