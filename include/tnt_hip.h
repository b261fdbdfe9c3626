/*
 * tnt_hip.h -- C ABI of the MI355X (gfx950) kernel library for the fMRI->caption
 * training hot path ("Think and Tell", seang123/Masters-Thesis).
 *
 * The reference has no FFI: its arithmetic is TensorFlow/Keras called from Python
 * (SURVEY.md 8b).  Each entry point below replaces the Keras op(s) at the cited
 * reference lines (paths relative to the reference repo root).  The reference-side
 * binding a maintainer would add is a ctypes stub; see INTEGRATION.md.
 *
 * Conventions
 *   - all tensors float32 unless noted; token ids int32; plain device pointers;
 *     the caller owns every buffer and workspace; no allocation, no global state
 *     (one documented exception: the two vendor-library A/B entry points tnt_gemm_blas_f32 /
 *     tnt_gemm_lt_f32 keep a process-wide rocBLAS / hipBLASLt handle and per-shape plans behind a
 *     mutex, csrc/blas.hip; no default training path calls them);
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work;
 *   - return 0 on success, a negative hipError_t on launch failure, -1000-k for
 *     an argument the kernels do not support (k = argument position);
 *   - matrices are row-major with an explicit leading dimension (in floats);
 *   - sequence activations are time-major: row = t*B + b;
 *   - LSTM tensors use the gate-interleaved axis order [.., U, 4] (i,f,c~,o
 *     innermost) instead of keras' [.., 4U] blocks; the host layer converts in
 *     get_weights/set_weights;
 *   - dropout masks come from the Philox4x32-10 stream of csrc/tnt_rng.h:
 *     element e of the *logical* tensor, (seed, site, step) identify the mask.
 */
#ifndef TNT_HIP_H
#define TNT_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TNT_ACT_NONE 0
#define TNT_ACT_LEAKY 1 /* x>0 ? x : slope*x   (LeakyReLU(0.2): lc_NIC.py:87,98,142) */
#define TNT_ACT_RELU 2
#define TNT_ACT_TANH 3

int32_t tnt_version(void);

/* ---- GEMM: C[M,N] (+)= act(op(A)[M,K] * op(B)[K,N] + bias[N]) -------------------
 * transA=0: A is [M][lda]; transA=1: A is stored [K][lda] (A^T), i.e. m contiguous.
 * transB=0: B is [K][ldb]; transB=1: B is stored [N][ldb] (B^T), i.e. k contiguous.
 * Replaces keras Dense / TimeDistributed(Dense) forward and the matmuls of
 * tape.gradient: layers.py:33, attention.py:21-23, lc_NIC.py:140-157,261,386-387,
 * NIC.py:64-69,92-96,143,248-249.  `pre` (nullable) receives the pre-activation.
 * accumulate=1: C += result (bias/act must then be none).
 * splitk>1: `work` must hold splitk*M*N floats; partials are reduced by a second
 * launch that applies bias/act (fixed order: bitwise reproducible). */
int32_t tnt_gemm_f32(const float* A, const float* B, float* C, const float* bias, float* pre,
                     int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc,
                     int32_t transA, int32_t transB, int32_t act, float slope,
                     int32_t accumulate, int32_t splitk, float* work, void* stream);
/* Plain library GEMM (rocBLAS sgemm, exact f32, atomics disabled => bitwise reproducible), same operand conventions as
 * tnt_gemm_f32 without the epilogue arguments: C = op(A) op(B) (+ C if accumulate).  For the matmuls that carry no
 * fused epilogue (weight / input gradients); the fused ones use tnt_gemm_f32.  The first call creates the process-wide
 * rocBLAS handle, and the first call of each shape loads its kernel -- make those outside a stream capture. */
int32_t tnt_gemm_blas_f32(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K,
                          int32_t lda, int32_t ldb, int32_t ldc, int32_t transA, int32_t transB,
                          int32_t accumulate, void* stream);

/* The same product (no accumulate) through hipBLASLt in full FP32 (HIPBLAS_COMPUTE_32F), optional bias [N] added to every
 * row of C (the Dense layers' bias, NIC.py:143).  The algorithm is the heuristic's first workspace-free candidate for the
 * shape (reproducible); TNT_LT_TUNE=1 in the environment times the candidates at the first un-captured call instead. */
int32_t tnt_gemm_lt_f32(const float* A, const float* B, float* C, const float* bias, int32_t M, int32_t N, int32_t K,
                        int32_t lda, int32_t ldb, int32_t ldc, int32_t transA, int32_t transB, void* stream);

/* One-round GEMM family for the products that carry no activation epilogue -- the weight / input gradients that
 * tape.gradient derives from the Dense / LSTM layers (lc_NIC.py:386-387, NIC.py:248-249) and the LSTM input projection
 * (NIC.py:138-140): C = op(A) op(B) (+ bias[N]), operand conventions of tnt_gemm_f32.  The workgroup tile is picked so
 * that the whole output is ONE round of at most 256 workgroups (one per CU); FP32 MFMA 16x16x4, exact f32, a fixed
 * summation order (bitwise reproducible).  Fused riders:
 *   colsum (nullable; transA=1, transB=0 only): colsum[n] = sum_k B[k][n] -- the bias gradient of the layer whose
 *     kernel gradient this product is (B = dY), computed from the B tiles the first row of workgroups loads anyway;
 *   A2 / C2 (both or neither): a second product C2 = op(A2) op(B) with the same dims and strides in the same launch
 *     (the LSTM's kernel and recurrent-kernel gradients share dZ).
 * cfg = 0: automatic; > 0: force configuration `cfg` of the table in csrc/gemm.hip (tools/gemm_cfg_scan.py).
 * Returns a negative code when no one-round configuration exists for the shape (the caller then uses tnt_gemm_f32). */
int32_t tnt_gemm_fused_f32(const float* A, const float* B, float* C, const float* bias, float* colsum,
                           const float* A2, float* C2, int32_t M, int32_t N, int32_t K, int32_t lda,
                           int32_t ldb, int32_t ldc, int32_t transA, int32_t transB, int32_t cfg, void* stream);
/* the configuration tnt_gemm_fused_f32 would pick (0 = none) */
int32_t tnt_gemm_fused_cfg(int32_t M, int32_t N, int32_t K, int32_t transA, int32_t transB, int32_t batch);

/* ---- gemm3 (round 3): the hand-written FP32-MFMA family that carries the step's large products by default --
 * the vocabulary head forward (NIC.py:143, lc_NIC.py:261) and, under tape.gradient (NIC.py:248-249, lc_NIC.py:386-387),
 * its kernel / input gradients, the LSTM input projection (NIC.py:138-140) and the LSTM kernel / recurrent-kernel / input
 * gradients.  C = op(A) op(B) (+ bias[N]); operand conventions of tnt_gemm_f32; A, B, C 16-byte aligned, lda / ldb / ldc
 * multiples of 4; a K-contiguous operand (A with transA = 0, B with transB = 1) whose K is not a multiple of 4 must have
 * zeros in the pad columns [K, roundup4(K)) (the layout contract of every buffer of this library), and the floats that follow
 * them up to the next multiple of the tile's stage depth (32 or 64 floats of k) -- the rest of a row stride above roundup4(K)
 * and the beginning of the following rows included -- must be FINITE: a row's last stage is fetched whole and what lies past
 * K is multiplied by zeros, so a NaN or an Inf there (in a view into an uninitialised buffer, say) lands in C.  Floats behind
 * the last row of the operand are not read.  Around an M/N-contiguous operand anything may stand: what is read there only
 * reaches rows / columns of C past M / N, which are not stored (with splitk > 1 it must not be the bit pattern 0x7FC5EED5, the
 * exchange buffer's "not written yet" word, for which an owner would wait until it gives up and sets `sync`).  Exact f32
 * (v_mfma_f32_16x16x4_f32), fixed summation order: bitwise reproducible.  cfg selects the workgroup tile (table in
 * csrc/gemm3.hip; tools/gemm3_scan.py). */
int32_t tnt_gemm3_f32(const float* A, const float* B, float* C, const float* bias, float* colsum, const float* A2,
                      float* C2, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc, int32_t transA,
                      int32_t transB, int32_t tile, int32_t splitk, float* work, uint32_t* sync, const int32_t* live,
                      int32_t live_mode, void* stream);
/* Riders (all nullable): bias [N] added to every row; colsum [N] = sum_k B[k][n] (transA = 1, transB = 0, splitk = 1 only:
 * B = dY, so this is the bias gradient of the layer whose kernel gradient the product is); A2 / C2 (both or neither): a
 * second product C2 = op(A2) op(B) with the same dims and strides in the same launch (the LSTM's kernel and
 * recurrent-kernel gradients share dZ).
 * splitk > 1: K is split over `splitk` workgroups per output tile, which reduce inside the launch (fixed order).  `work`:
 * tnt_gemm3_work_floats(M, N, tile, splitk, batch) floats, ARMED once with tnt_gemm3_work_arm (every word = the "not
 * written yet" pattern) -- every launch leaves it armed, so launches of any shape may share one buffer as long as they run
 * one after the other; `sync`: tnt_gemm3_sync_words(...) uint32 words (one: an error flag, zero before the first use;
 * nonzero afterwards means a workgroup gave up waiting for a peer -- the launch did not fit the device in one round -- and
 * C is invalid).
 * batch = 2 with A2 / C2, else 1.
 * live (nullable; null: the launch is bit-identical to one without it): ONE int32 word in device memory, read by every
 * workgroup when the launch runs -- an extent only the device knows (the number of distinct rows of tnt_stage_batch_map_f32),
 * so that a recorded launch replays with whatever the word holds then.  The value is clamped to [0, extent].
 *   live_mode = 1 (transA = 0): only rows [0, *live) of A and C exist.  The grid is that of M; a workgroup whose tile starts
 *     at or past *live returns at once, rows of A past it read as zero, rows of C at or past it are NOT written.
 *   live_mode = 2 (transA = 1, transB = 0, splitk = 1): only rows [0, *live) of the contraction (of A and B as stored) exist:
 *     C = sum over k < *live, colsum likewise; *live = 0 gives C = bias or 0 and colsum = 0.
 *   live_mode = 3 (transA = 0): live_mode 1, and with splitk > 1 and fewer live row tiles than M has, the launch deals the
 *     SAME grid over the live row tiles only, with the largest split S' that fits it (S' <= the grid's units / live tiles,
 *     S' <= the stage count, never below splitk): equal, smaller shares of K instead of idle workgroups.  The summation
 *     order of C then depends on the word (a deterministic function of operands and word; the same launch twice gives the
 *     same bits); for *live >= M, or a word that leaves the row-tile count at M's, the launch is that of live_mode 1.
 *   Any other combination: TNT_BADARG.  To get a tile that suits the live extent, ask tnt_gemm3_plan for the shape with the
 *   EXPECTED extent in place of M (the result stays correct for any value of the word: the grid always covers M). */
/* The (tile, splitk) the library's cost model picks for a shape (batch = 2 for a dual launch; allow_split = 0 restricts
 * the choice to splitk = 1, which the colsum rider needs). */
int32_t tnt_gemm3_plan(int32_t M, int32_t N, int32_t K, int32_t transA, int32_t transB, int32_t batch,
                       int32_t allow_split, int32_t* tile, int32_t* splitk);
int32_t tnt_gemm3_work_floats(int32_t M, int32_t N, int32_t tile, int32_t splitk, int32_t batch);
int32_t tnt_gemm3_sync_words(int32_t M, int32_t N, int32_t tile, int32_t batch);
int32_t tnt_gemm3_work_arm(float* work, int64_t floats, void* stream);

/* Two INDEPENDENT products in one launch (the second one's workgroups start on the CUs the first one's tail leaves idle;
 * a launch boundary costs a 25-50 us GEMM 4-6 us of ramp-up and drain): fields = the arguments of tnt_gemm3_f32.  The
 * backward pass has such pairs back to back: the head's kernel gradient + input gradient (both read dlogits; NIC.py:143
 * under tape.gradient), the LSTM's kernel gradients + input gradient (both read dZ; NIC.py:138-140).  Supported
 * combinations: tnt_gemm3_pair_supported (else TNT_BADARG: issue two tnt_gemm3_f32 calls).  Two split products need
 * distinct `work` buffers. */
typedef struct tnt_gemm3_desc {
  const float* A; const float* B; float* C; const float* bias; float* colsum; const float* A2; float* C2;
  int32_t M, N, K, lda, ldb, ldc, transA, transB, tile, splitk;
  float* work; uint32_t* sync;
  const int32_t* live; int32_t live_mode;      /* as tnt_gemm3_f32; several products may share one word */
} tnt_gemm3_desc;
int32_t tnt_gemm3_pair_supported(int32_t tile1, int32_t transA1, int32_t transB1, int32_t tile2, int32_t transA2,
                                 int32_t transB2);
int32_t tnt_gemm3_pair_f32(const tnt_gemm3_desc* p, const tnt_gemm3_desc* q, void* stream);
/* The joint plan of a pair launch.  p1, p2: eight int32 each = {M, N, K, transA, transB, batch, live, flags}: the shape as the
 * descriptor will carry it, the extent to EXPECT in the product's live word (rows of A / C, or of the contraction for
 * transA = 1; 0: no live word) and flags (1: no split -- the colsum rider; 2: the launch will use live_mode 3; 4: a 64-deep
 * pick is launched as its 32-deep twin, as the step does for a small product that rides along).  The model deals the
 * workgroups of both products over 256 CUs in launch order, at the workgroups per CU the pair kernel's registers and LDS
 * allow, prices each by the K stages it will really run and minimises the busiest CU.  A launch with a split product keeps
 * all its workgroups resident together.  out: eight int32 = {tile1, splitk1, units1, tile2, splitk2, units2, workgroups
 * per CU, 0}; span (nullable; two doubles): {modelled us of this plan, of the two independent tnt_gemm3_plan picks}, span[0] <= span[1]
 * by construction (the independent picks are the incumbent).  TNT_BADARG where the independent picks have no pair form. */
int32_t tnt_gemm3_plan_pair(const int32_t* p1, const int32_t* p2, int32_t* out, void* span);

/* ---- the optimizer step without a finalize launch (single-process step; optimizer.apply_gradients with clipnorm + Adam,
 * main.py:97, lc_NIC.py:389).  tnt_step_finalize_f32 -- per-variable norms from the span partials, the step's scalar totals,
 * the counter tick -- was one dependent launch in front of the update: 12 us of a 500 us step.  Here
 *   tnt_span_sqnorm_lr_f32 / tnt_dense_gram_norm_spans_lr_f32: the norm launches, with one thread also writing Adam's step
 *       size lr_t = lr sqrt(1-b2^t)/(1-b1^t), t = *adam_t + 1, for the update that follows.  `sq_override` (may be NULL:
 *       everything is read): the per-variable table of externally supplied clip norms the update launches take; a variable
 *       with sq_override[seg] >= 0 (the Embedding: IndexedSlices norm, lc_NIC.py:386-389) gets no pass over its gradient,
 *       and sum theta^2 -- consumed only as lambda * sum theta^2 of the L2 metric -- is left 0 where seg_l2[seg] == 0;
 *   tnt_dense_dw_adam_fin_f32: tnt_dense_dw_adam_f32 with the kernel's clip norm summed from partial[2k], k0 <= k < k1, by
 *       the launch itself;
 *   tnt_adam_fin_f32: tnt_adam_ring_f32 over spans whose variables' clip norms are summed from `fin->partial` by every
 *       workgroup that needs one (same order everywhere); ONE extra workgroup files everything tnt_step_finalize_f32 wrote
 *       (fields of tnt_finalize_desc = its arguments; extra_seg = the variable whose norm is sum(extra_part), -1: none;
 *       `arrive`: one zeroed uint32, left zero) beside the update; *adam_t and *drop_step advance when the LAST workgroup
 *       of the launch is done (unless *guard != 0).  Issue order: norm launch, tnt_dense_dw_adam_fin_f32, tnt_adam_fin_f32. */
typedef struct tnt_finalize_desc {
  const float* partial; const int32_t* seg_first; const float* seg_l2; float* sq; float* wsq; float* l2_out; int32_t nseg;
  const float* x0; float* out0; const float* x1; float* out1; int32_t n; float scale;
  const float* extra_part; float* extra; int32_t n_extra; int32_t extra_seg;
  const int32_t* ids_src; int32_t* ids_dst; int32_t n_ids;
  const float* x2; float* out2; int32_t n2; float scale2;
  int64_t* adam_t; uint32_t* drop_step; const float* lr; float* lr_t; float beta1, beta2; const uint32_t* guard;
  uint32_t* arrive;
} tnt_finalize_desc;
int32_t tnt_span_sqnorm_lr_f32(const float* theta, const float* grad, const int32_t* span_seg, const int64_t* span_off,
                               const int32_t* span_len, const float* seg_l2, float* partial, int32_t nspan,
                               const int64_t* adam_t, const float* lr, float* lr_t, float beta1, float beta2,
                               const float* sq_override, void* stream);
int32_t tnt_dense_gram_norm_spans_lr_f32(const float* dpre, const float* pre, const float* bias, const float* gx_part,
                                         int32_t nsplit, const float* w2_part, int32_t nw2, float l2, float* partial,
                                         int32_t nslot, int32_t Bk, int32_t E, const float* theta, const float* grad,
                                         const int32_t* span_seg, const int64_t* span_off, const int32_t* span_len,
                                         const float* seg_l2, float* span_partial, int32_t nspan, const int64_t* adam_t,
                                         const float* lr, float* lr_t, float beta1, float beta2, const float* sq_override,
                                         void* stream);
int32_t tnt_dense_dw_adam_fin_f32(const float* x, const float* dpre, float* theta, float* m, float* v, float l2,
                                  const float* partial, int32_t k0, int32_t k1, const float* sq_override,
                                  const float* lr_t_dev, float beta1, float beta2, float eps, float clipnorm,
                                  const uint32_t* guard, int32_t N, int32_t E, int32_t Bk, int32_t ldx, void* stream);
int32_t tnt_adam_fin_f32(float* theta, float* m, float* v, const float* grad, const int32_t* span_seg,
                         const int64_t* span_off, const int32_t* span_len, const float* sq_override, int32_t nspan, float eps,
                         float clipnorm, const tnt_finalize_desc* fin, const float* met, int32_t nmet, float* ring,
                         int32_t ring_rows, uint32_t* ring_t, void* stream);

/* tuning entry point: tnt_gemm_f32 with the workgroup tile forced to bm x bn (each 64 or 128; anything else =
 * the library's own choice).  Used by tools/gemm_bench.py / gemm_scan.py to calibrate the tile heuristic. */
int32_t tnt_gemm_f32_tile(const float* A, const float* B, float* C, const float* bias, float* pre,
                          int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc,
                          int32_t transA, int32_t transB, int32_t act, float slope,
                          int32_t accumulate, int32_t splitk, float* work, int32_t bm, int32_t bn,
                          void* stream);

/* ---- dropout (keras Dropout, inverted; lc_NIC.py:51-55,94; LSTM dropout= :122) ---
 * y[r][c] = keep ? x[r][c]/(1-rate) : 0 for r<rows, c<cols (ld = row stride of x,y).
 * logical element index e = lrow*lwidth + lcol0 + c, with
 *   lrow = r                      if tmajor_B == 0
 *   lrow = (r % B)*T + r / B      if tmajor_B == B > 0 (buffer time-major, logical (B,T,..)),
 * where T = rows / B.  In-place (y == x) allowed.  Backward = same call on dy.
 * rows_per_site > 0 (requires tmajor_B == 0): the buffer is a stack of independent
 * (rows_per_site x cols) tensors, block k using site + k and local rows -- one launch for
 * the T per-timestep masks of lc_NIC.py:255-256.
 * The stream step is step + *step_dev (step_dev nullable): a device-resident counter
 * lets a captured hipGraph replay with a fresh mask each time (see tnt_step_tick).
 * rows <= 0 or cols <= 0 is a no-op.  TNT_BADARG, and no launch, for ld < cols and for a rate outside [0, 1) (in
 * tnt_dropout_f32, tnt_dropout_metric_f32, tnt_dropout2_f32 -- whose rates lie in (0, 1) -- and tnt_dropout_mask4_u8). */
/* Keep-masks only (no data pass): out[nsites][n/4] bytes, bit j of byte g of block k = element 4g+j of site site0+k is
 * kept -- the same Philox stream (seed, site, step + *step_dev, element) as tnt_dropout_f32, n % 4 == 0.  One launch
 * produces the attention-dropout masks of all T timesteps (attention.py:36, sites S_ATTN + t) off the serial chain;
 * tnt_attention_step_{fwd,bwd}_f32 take them through `keep4`. */
int32_t tnt_dropout_mask4_u8(uint8_t* out, int64_t n, int32_t nsites, float rate, uint64_t seed, uint32_t site0,
                             uint32_t step, const uint32_t* step_dev, void* stream);
int32_t tnt_dropout_f32(const float* x, float* y, int32_t rows, int32_t cols, int32_t ld,
                        int32_t tmajor_B, int32_t lwidth, int32_t lcol0, int32_t rows_per_site,
                        float rate, uint64_t seed, uint32_t site, uint32_t step,
                        const uint32_t* step_dev, void* stream);
/* tnt_dropout_f32 (vector form only: cols, ld, lwidth, lcol0 % 4 == 0, 16-byte aligned x / y) with the partials of
 * tnt_attention_metric_f32(out = NULL) as extra workgroups of the same launch: partial[tnt_attention_metric_parts(T, R)]
 * from alpha [T][B][R] (lc_NIC.py:365-367). */
int32_t tnt_dropout_metric_f32(const float* x, float* y, int32_t rows, int32_t cols, int32_t ld, int32_t tmajor_B,
                               int32_t lwidth, int32_t lcol0, int32_t rows_per_site, float rate, uint64_t seed,
                               uint32_t site, uint32_t step, const uint32_t* step_dev, const float* alpha,
                               float* partial, int32_t T, int32_t B, int32_t R, void* stream);
/* y = mask_b(mask_a(x)): two Dropout masks over the same matrix in one launch, each with its own logical layout, rate and
 * site (arguments as in tnt_dropout_f32, suffix _a / _b), same seed and step -- bit-identical to the two tnt_dropout_f32
 * calls it replaces (the LSTM input mask and the Embedding Dropout of the text rows in the backward pass,
 * lc_NIC.py:233-234,255).  Both rates in (0, 1); cols, ld, lwidth_*, lcol0_* % 4 == 0, x / y 16-byte aligned. */
int32_t tnt_dropout2_f32(const float* x, float* y, int32_t rows, int32_t cols, int32_t ld, int32_t tmajor_B_a,
                         int32_t lwidth_a, int32_t lcol0_a, int32_t rows_per_site_a, float rate_a, uint32_t site_a,
                         int32_t tmajor_B_b, int32_t lwidth_b, int32_t lcol0_b, int32_t rows_per_site_b, float rate_b,
                         uint32_t site_b, uint64_t seed, uint32_t step, const uint32_t* step_dev, void* stream);

/* ---- activation backward: dx = dy * act'(pre)  ---------------------------------- */
int32_t tnt_act_bwd_f32(const float* pre, const float* dy, float* dx, int64_t n, int32_t act,
                        float slope, void* stream);
/* Backward of y = Dropout(act(pre)) of a layer applied to rows <= 2048 rows, up to its bias gradient, in one launch:
 * dx = dropout'(dy) * act'(pre) (dx may alias dy), dbias[c] = sum_r dx[r][c].  The dropout stream / logical layout
 * arguments are those of tnt_dropout_f32 for the forward's mask (rate 0: no dropout).  cols, ld, lwidth, lcol0 % 4 == 0,
 * 16-byte aligned, ld >= cols, rate in [0, 1): anything else is TNT_BADARG and no launch.  Optional second job in the same launch: out1 = column sums of x1 [rows1 <= 2048][C1] (x1 NULL: none).
 * (TimeDistributed(Dense) + Dropout of the caption head, lc_NIC.py:271-275, and its bias gradients.) */
int32_t tnt_bias_act_drop_bwd_f32(const float* dy, const float* pre, float* dx, float* dbias, int32_t rows, int32_t cols,
                                  int32_t ld, int32_t act, float slope, int32_t tmajor_B, int32_t lwidth, int32_t lcol0,
                                  float rate, uint64_t seed, uint32_t site, const uint32_t* step_dev, const float* x1,
                                  float* out1, int32_t rows1, int32_t C1, int32_t ld1, void* stream);

/* ---- BatchNormalization, axis=-1, non-fused keras semantics ---------------------
 * (layers.py:40,50; NIC.py:62,128; fullyConnected.py:18,24)
 * x is [rows][C] (ld = C).  training=1: biased batch statistics over rows;
 * moving <- moving*momentum + batch*(1-momentum) (updated in place).
 * Outputs: y, xhat (saved for backward), inv_std[C].  work: C*(2*nchunk+1) floats
 * (nchunk = tnt_bn_nchunk(rows)), same size for the backward and for LayerNorm bwd.
 * xhat and dx are dense ([rows][C]); only y (ldy) and dy (lddy) carry a row stride.
 * Every BatchNorm / LayerNorm entry point below returns TNT_BADARG, before any launch, for rows <= 0, C <= 0 and a row
 * stride (ldy, lddy) smaller than C. */
int32_t tnt_bn_nchunk(int32_t rows);
int32_t tnt_batchnorm_fwd_f32(const float* x, const float* gamma, const float* beta,
                              float* mov_mean, float* mov_var, float* y, float* xhat,
                              float* inv_std, int32_t rows, int32_t C, int32_t ldy,
                              int32_t training, float eps, float momentum, float* work,
                              void* stream);
/* ... with the keras Dropout that follows the normalisation (layers.py:50-51) applied to y in the same pass: element
 * r*C + c of stream (seed, site, *step_dev); xhat stays the un-dropped normalised value.  rate 0 = tnt_batchnorm_fwd_f32. */
int32_t tnt_batchnorm_fwd_drop_f32(const float* x, const float* gamma, const float* beta,
                                   float* mov_mean, float* mov_var, float* y, float* xhat,
                                   float* inv_std, int32_t rows, int32_t C, int32_t ldy,
                                   int32_t training, float eps, float momentum, float* work,
                                   float rate, uint64_t seed, uint32_t site, const uint32_t* step_dev,
                                   void* stream);
/* dx (nullable), dgamma[C], dbeta[C] from dy (row stride lddy), xhat, inv_std.  dgamma and dbeta come as a pair (with
 * work) or are both NULL.  Both NULL is valid only for training = 0, where dx = gamma * inv_std * dy needs no sums; with
 * training != 0 the input gradient reads both sums, so dx != NULL without them is TNT_BADARG (nothing is launched).
 * dx == NULL with the sums given (the local sums of synchronised BatchNorm) is valid in either mode. */
int32_t tnt_batchnorm_bwd_f32(const float* dy, const float* xhat, const float* gamma,
                              const float* inv_std, float* dx, float* dgamma, float* dbeta,
                              int32_t rows, int32_t C, int32_t lddy, int32_t training,
                              float* work, void* stream);
/* ... with dx further multiplied by LeakyReLU'(act_pre [rows][C], slope): the backward of the activation in front of the
 * normalisation (layers.py:48-50) in the same pass.  act_pre NULL = tnt_batchnorm_bwd_f32. */
int32_t tnt_batchnorm_bwd_act_f32(const float* dy, const float* xhat, const float* gamma,
                              const float* inv_std, float* dx, float* dgamma, float* dbeta,
                              int32_t rows, int32_t C, int32_t lddy, int32_t training,
                              float* work, const float* act_pre, float slope, void* stream);

/* Synchronised BatchNorm (data parallel, opt-in; the reference trains on one device, so this is what makes G replicas x
 * local batch equal ONE process on the concatenated batch when the encoder uses BatchNorm): the pieces of the two
 * functions above around the caller's collectives.
 *   stats        part = this replica's row-chunk partials, tnt_bn_nchunk(rows) * 2 * C floats;
 *   apply_stats  part_all = nrep replicas' partials back to back (all-gathered, every replica `rows` rows): statistics over
 *                nrep * rows rows, moving statistics updated, y / xhat / inv_std written; mean_work: C floats of scratch;
 *   dx           input gradient from dgamma_sum / dbeta_sum taken over all n_total rows (all-reduced local sums of
 *                tnt_batchnorm_bwd_f32 called with dx = NULL). */
int32_t tnt_batchnorm_stats_f32(const float* x, int32_t rows, int32_t C, float* part, void* stream);
int32_t tnt_batchnorm_apply_stats_f32(const float* part_all, int32_t nrep, const float* x, const float* gamma,
                                      const float* beta, float* mov_mean, float* mov_var, float* y, float* xhat,
                                      float* inv_std, int32_t rows, int32_t C, int32_t ldy, float eps, float momentum,
                                      float* mean_work, void* stream);
int32_t tnt_batchnorm_dx_f32(const float* dy, int32_t lddy, const float* xhat, const float* gamma, const float* inv_std,
                             const float* dgamma_sum, const float* dbeta_sum, float* dx, int32_t rows, int32_t C,
                             int32_t n_total, void* stream);

/* Split mode of the two entry points above: the launch runs over PIECES of at most `piece` voxels of a region's index
 * list, so that one large region does not set the kernel time (regions span 8..400+ voxels; measured 39 -> ~12 us
 * at 360 regions of 18..240 voxels).  Tables (host-built from goff): vgoff[NV+1] CSR range of each piece, vreg[NV] its
 * region, vfirst[NV] 1 for a region's first piece, rfirst[R+1] first piece of each region.  Forward = piece partials
 * (partial: NV*64*D floats) + a combine launch; results equal the unsplit ones up to f32 summation order.
 * x_voxel_major = 1: x is stored [n_voxels][ldx] (ldx >= B, ldx % 4 == 0): a voxel's batch values are contiguous, the
 * gather reads whole 256-byte rows and every byte of the betas is fetched once per piece -- the layout to stage at
 * full-cortex width, where the batch-major gather re-fetches each 128-byte line once per region that shares it. */
int32_t tnt_locally_dense_fwd_split_f32(const float* x, int32_t ldx, const int32_t* idx, const int32_t* vgoff,
                                        const int32_t* vreg, const int32_t* rfirst, int32_t NV,
                                        const float* W, const float* bias, float* pre, float* y,
                                        float* partial, int32_t B, int32_t R, int32_t D, float slope,
                                        int32_t x_voxel_major, void* stream);
int32_t tnt_locally_dense_bwd_split_f32(const float* x, int32_t ldx, const int32_t* idx, const int32_t* vgoff,
                                        const int32_t* vreg, const int32_t* vfirst, int32_t NV,
                                        const float* dpre, float* dW, float* db, int32_t B, int32_t R,
                                        int32_t D, int32_t x_voxel_major, void* stream);

/* ---- forward of the dense voxel encoder at small batch, as K-split partials ---------------------------
 * part[s][B][E] = x[B][K slice s] @ w[K slice s][E], s < nsplit; x [B][ldx] (K % 4 == 0, ldx % 4 == 0), w [K][ldw]
 * keras (in, out) kernel, E % 32 == 0, nsplit <= 64, all 16-byte aligned.  (NIC.py:64-69,125; ThinkAndTell
 * model.py:22-33.)  The sum over s (+ bias + LeakyReLU) is taken by tnt_enc_tail_fwd_sk_f32. */
int32_t tnt_dense_fwd_stream_f32(const float* x, const float* w, float* part, int32_t B, int32_t E, int32_t K,
                                 int32_t ldx, int32_t ldw, int32_t nsplit, void* stream);

/* Training variant with the two by-products the optimizer step needs to clip this kernel's gradient without forming
 * it (one row block: B <= 64, K % 16 == 0, E >= 512): gx_part [nsplit][64][64] K-split partials of x x^T (rows/columns
 * >= B undefined), w2_part [nsplit * E / 32] parts of sum w^2. */
int32_t tnt_dense_fwd_stream_gram_f32(const float* x, const float* w, float* part, float* gx_part, float* w2_part,
                                      int32_t B, int32_t E, int32_t K, int32_t ldx, int32_t ldw, int32_t nsplit,
                                      void* stream);
/* tnt_dense_fwd_stream_gram_f32 on the caller's own batch x [B][N] (contiguous rows: ldx = K = N) with ALL of
 * tnt_stage_batch_map_f32's job riding in the same launch, as extra workgroups beside the forward's: the copy of x into
 * x_dst [B][ldx_dst] (which the end of the step reads), cap, tgt (time-major), a0 -> h0, c0 -> c0_dst, and the row map
 * (pos, row_weight, tgt_compact, live, loss_row, corr_row; the last two nullable).  Every output is bit-identical to
 * tnt_stage_batch_map_f32 followed by tnt_dense_fwd_stream_gram_f32 on the staged copy; neither role reads what the other
 * writes.  B <= 64, N % 16 == 0, E % 32 == 0, E >= 512, x, w, part (and x_dst when ldx_dst % 4 == 0) 16-byte aligned:
 * anything else is refused (non-zero) before any launch, and the caller takes the two launches instead. */
int32_t tnt_dense_fwd_stream_gram_stage_f32(const float* x, const float* w, float* part, float* gx_part, float* w2_part,
                                            int32_t B, int32_t E, int32_t N, int32_t ldw, int32_t nsplit, float* x_dst,
                                            int32_t ldx_dst, const int32_t* cap, int32_t* cap_dst, const int32_t* tgt,
                                            int32_t* tgt_tmajor, const float* a0, float* h0, const float* c0,
                                            float* c0_dst, int32_t T, int32_t U, int32_t* pos, float* row_weight,
                                            int32_t* tgt_compact, int32_t* live, float* loss_row, float* corr_row,
                                            void* stream);
/* ... and the finish, after the backward pass produced dpre [Bk][E] (gradient w.r.t. the pre-activation pre [Bk][E]
 * = x w + bias): for g = x^T dpre (NIC.py:248-249) the clipnorm input sum (g + 2 l2 w)^2 = ||g||^2 + 4 l2 <g, w> +
 * 4 l2^2 ||w||^2 with ||g||^2 = sum (x x^T) o (dpre dpre^T) and <g, w> = sum dpre o (pre - bias), written as span
 * partials (partial[2k] parts of the norm, partial[2k+1] parts of sum w^2, every k < nslot written; nslot >= 4 Bk + nw2)
 * in the layout tnt_span_sqnorm_f32 / tnt_step_finalize_f32 use for this variable. */
int32_t tnt_dense_gram_norm_f32(const float* dpre, const float* pre, const float* bias, const float* gx_part,
                                int32_t nsplit, const float* w2_part, int32_t nw2, float l2, float* partial,
                                int32_t nslot, int32_t Bk, int32_t E, void* stream);
/* ... with tnt_span_sqnorm_f32's job for the other variables (same arguments: the span tables and partial buffer of the
 * nspan spans that are NOT this variable's) riding in the same launch */
int32_t tnt_dense_gram_norm_spans_f32(const float* dpre, const float* pre, const float* bias, const float* gx_part,
                                      int32_t nsplit, const float* w2_part, int32_t nw2, float l2, float* partial,
                                      int32_t nslot, int32_t Bk, int32_t E, const float* theta, const float* grad,
                                      const int32_t* span_seg, const int64_t* span_off, const int32_t* span_len,
                                      const float* seg_l2, float* span_partial, int32_t nspan, void* stream);

/* ---- weight gradient of the dense voxel encoder at small batch:  dw[N][E] = x^T @ dpre --------------
 * x [Bk][ldx] (the betas, Bk <= 64 rows), dpre [Bk][E] (E % 32 == 0, E <= 512, 16-byte aligned), dw [N][E].
 * (NIC.py:64-69,248-249; ThinkAndTell model.py:22-33.)  Same result as tnt_gemm_f32(transA=1) up to f32
 * summation order; a persistent, write-bound kernel instead of 2504 two-chunk tiles. */
int32_t tnt_dense_dw_skinny_f32(const float* x, const float* dpre, float* dw, int32_t N, int32_t E,
                                int32_t Bk, int32_t ldx, void* stream);

/* ---- the same weight gradient, consumed in place by the single-process optimizer step (clipnorm + Adam of
 * optimizer.apply_gradients, NIC.py:250-251, main.py:97) instead of being written out: E % 512 == 0, Bk <= 64.
 * sqnorm: partial[2k] = part of sum (g + 2 l2 theta)^2, partial[2k+1] = part of sum theta^2, k < nslot -- the span-partial
 *         layout of tnt_span_sqnorm_f32 for this variable's nslot >= 256 * E / 512 (or N/16 * E / 512) spans; every slot
 *         is written.
 * adam:   theta, m, v of the variable ([N][E]) updated exactly as tnt_adam_f32 does with grad = x^T dpre, clip factor
 *         from sq[0] (sq_override[0] >= 0 wins), lr_t from *lr_t_dev; skipped when *guard != 0. */
int32_t tnt_dense_dw_sqnorm_f32(const float* x, const float* dpre, const float* theta, float l2, float* partial,
                                int32_t nslot, int32_t N, int32_t E, int32_t Bk, int32_t ldx, void* stream);
int32_t tnt_dense_dw_adam_f32(const float* x, const float* dpre, float* theta, float* m, float* v, float l2,
                              const float* sq, const float* sq_override, const float* lr_t_dev, float beta1,
                              float beta2, float eps, float clipnorm, const uint32_t* guard, int32_t N, int32_t E,
                              int32_t Bk, int32_t ldx, void* stream);

/* ---- fused tail of the dense voxel encoder at small batch (rows <= 256, C % 4 == 0, 16-byte aligned
 * operands), NIC.py:126-128,138 ------------------------------------------------------------------
 * fwd: out = lstm_in_dropout( BatchNorm( feature_dropout(y) ) ), training statistics over the rows (moving
 *      statistics updated), or the moving statistics when training=0 (dropouts off).  Saves xhat, inv_std.
 *      Dropout element index = r*C + c in streams (seed, site_feat | site_lstm, *step_dev).
 * bwd: dout (gradient w.r.t. out, row stride ldo) -> lstm-in dropout' -> BatchNorm' (dgamma, dbeta) ->
 *      feature dropout' -> LeakyReLU'(pre, slope) -> dpre [rows][C]; dbias[c] = sum_r dpre.
 * One launch each, replacing 5 / 7 dependent launches of the generic entry points above (same arithmetic).
 * TNT_BADARG, and no launch, for rows outside 1 .. 256, C <= 0 or C % 4 != 0, ldo < C or ldo % 4 != 0, r_feat or r_lstm
 * outside [0, 1) and an operand off 16-byte alignment (forward and backward entry points alike). */
int32_t tnt_enc_tail_fwd_f32(const float* y, const float* gamma, const float* beta, float* mov_mean,
                             float* mov_var, float* out, float* xhat, float* inv_std, int32_t rows,
                             int32_t C, int32_t ldo, int32_t training, float eps, float momentum,
                             float r_feat, float r_lstm, uint64_t seed, uint32_t site_feat,
                             uint32_t site_lstm, const uint32_t* step_dev, void* stream);
/* fwd from the K-split partials of tnt_dense_fwd_stream_f32: y = LeakyReLU(sum_s part[s] + bias, slope) in split
 * order (the Dense layer's output, NIC.py:125; pre-activation stored to pre [rows][C] for the backward), then as above. */
int32_t tnt_enc_tail_fwd_sk_f32(const float* part, int32_t nsplit, const float* bias, float* pre, float slope,
                                const float* gamma, const float* beta, float* mov_mean, float* mov_var, float* out,
                                float* xhat, float* inv_std, int32_t rows, int32_t C, int32_t ldo, int32_t training,
                                float eps, float momentum, float r_feat, float r_lstm, uint64_t seed,
                                uint32_t site_feat, uint32_t site_lstm, const uint32_t* step_dev, void* stream);
/* ... with the Embedding gather + input dropout of the text rows (tnt_embedding_fwd_drop_f32 with out = NULL: table
 * [emb_V][C], ids [emb_B][emb_T], emb_out rows t*B + b with row stride ldo, stream (seed, emb_site, *step_dev), rate 0 =
 * plain gather) riding in the same launch: both feed the same LSTM input buffer (NIC.py:131,138-140) */
int32_t tnt_enc_tail_fwd_sk_emb_f32(const float* part, int32_t nsplit, const float* bias, float* pre, float slope,
                                    const float* gamma, const float* beta, float* mov_mean, float* mov_var, float* out,
                                    float* xhat, float* inv_std, int32_t rows, int32_t C, int32_t ldo, int32_t training,
                                    float eps, float momentum, float r_feat, float r_lstm, uint64_t seed,
                                    uint32_t site_feat, uint32_t site_lstm, const uint32_t* step_dev,
                                    const float* emb_table, const int32_t* emb_ids, float* emb_out, int32_t emb_B,
                                    int32_t emb_T, int32_t emb_V, float emb_rate, uint32_t emb_site, void* stream);
int32_t tnt_enc_tail_bwd_f32(const float* dout, const float* xhat, const float* gamma, const float* inv_std,
                             const float* pre, float* dpre, float* dgamma, float* dbeta, float* dbias,
                             int32_t rows, int32_t C, int32_t ldo, float r_feat, float r_lstm, float slope,
                             uint64_t seed, uint32_t site_feat, uint32_t site_lstm,
                             const uint32_t* step_dev, void* stream);
/* bwd with an independent in-place dropout' job in the same launch: drop_x [drop_rows][drop_cols] (row stride drop_ld) gets
 * the keep mask of stream (seed, drop_site, *step_dev) in the logical layout arguments of tnt_dropout_f32 -- the text
 * call's LSTM-input dropout over the other rows of the same gradient buffer (NIC.py:131,140).  All % 4 == 0,
 * drop_ld >= drop_cols, drop_rate in [0, 1). */
int32_t tnt_enc_tail_bwd_drop_f32(const float* dout, const float* xhat, const float* gamma, const float* inv_std,
                                  const float* pre, float* dpre, float* dgamma, float* dbeta, float* dbias, int32_t rows,
                                  int32_t C, int32_t ldo, float r_feat, float r_lstm, float slope, uint64_t seed,
                                  uint32_t site_feat, uint32_t site_lstm, const uint32_t* step_dev, float* drop_x,
                                  int32_t drop_rows, int32_t drop_cols, int32_t drop_ld, int32_t drop_tmajor_B,
                                  int32_t drop_lwidth, int32_t drop_lcol0, float drop_rate, uint32_t drop_site,
                                  void* stream);

/* ---- LayerNormalization(axis=-1) (layers.py:41 alternative; BASELINE north_star) - */
int32_t tnt_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y,
                              float* xhat, float* inv_std, int32_t rows, int32_t C,
                              int32_t ldy, float eps, void* stream);
int32_t tnt_layernorm_bwd_f32(const float* dy, const float* xhat, const float* gamma,
                              const float* inv_std, float* dx, float* dgamma, float* dbeta,
                              int32_t rows, int32_t C, int32_t lddy, float* work, void* stream);

/* ---- column sums: out[c] = sum_r x[r][c]  (bias gradients of every Dense) -------
 * work: C*tnt_bn_nchunk(rows) floats. */
int32_t tnt_colsum_f32(const float* x, float* out, int32_t rows, int32_t C, int32_t ld,
                       float* work, void* stream);
/* two / up to four independent matrices of <= 2048 rows each in one launch (same results as separate tnt_colsum_f32
 * calls; in tnt_colsum4_f32 a job with x == NULL is skipped) */
int32_t tnt_colsum4_f32(const float* x0, float* out0, int32_t rows0, int32_t C0, int32_t ld0, const float* x1, float* out1,
                        int32_t rows1, int32_t C1, int32_t ld1, const float* x2, float* out2, int32_t rows2, int32_t C2,
                        int32_t ld2, const float* x3, float* out3, int32_t rows3, int32_t C3, int32_t ld3, void* stream);
int32_t tnt_colsum2_f32(const float* x0, float* out0, int32_t rows0, int32_t C0, int32_t ld0, const float* x1,
                        float* out1, int32_t rows1, int32_t C1, int32_t ld1, void* stream);

/* ---- Embedding (lc_NIC.py:105-112,233; NIC.py:75-79,131) ------------------------
 * fwd: out[(t*B+b)][:] = table[ids[b*T+t]][:]   (ids is the keras (B,T) int32 array)
 * bwd: dtable[v][:] = sum over (b,t) with ids[b*T+t]==v of drows[(t*B+b)][:] (every row
 *      of dtable is written: unreferenced rows are zeroed by the call itself);
 *      sq_norm[0] = sum of squares of the un-merged rows (IndexedSlices clipnorm
 *      quirk), overwritten (nullable: no norm, rowsq_work unused); rowsq_work: B*T floats.
 * Ids outside [0, V): every embedding entry point (fwd, fwd_drop, fwd_drop2, bwd, bwd_sparse) treats an id as
 *      clip(id, 0, V-1).  The backward scatters a row to the table row the forward gathered it from and counts it in the
 *      norm; in prev_ids of tnt_embedding_bwd_sparse_f32 an entry >= V stands for row V-1 and every negative entry -- the
 *      "none" sentinel -1 cannot be told from a stray id -- for row 0.
 * Deterministic (no atomics): a launch zero-fills dtable, then one workgroup per (b,t) position k = b*T+t and column
 *      chunk (64 columns; 256 when E % 4 == 0, ldd % 4 == 0 and drows, dtable are 16-byte aligned) looks for an earlier
 *      occurrence of its id.  The FIRST occurrence owns the vocabulary row: its 4 waves scan the later positions 64 at a
 *      time (wave w the windows k+1+64w, +256, ...), sum the duplicates' rows in position order, 16 (8 in the 256-column
 *      form) row loads in flight, and the 4 partial sums are added in wave order.  Fixed partition, fixed order: the same
 *      bits on every run. */
int32_t tnt_embedding_fwd_f32(const float* table, const int32_t* ids, float* out, int32_t B,
                              int32_t T, int32_t E, int32_t ldo, int32_t V, void* stream);
/* fwd + keras Dropout over the logical (B,T,E) tensor in the same pass (NIC.py:131,140): out_drop gets the
 * masked rows (stream (seed, site, step + *step_dev), element (b*T+t)*E + j); out (nullable) the plain ones.
 * E % 4 == 0, ldo % 4 == 0, 16-byte aligned. */
int32_t tnt_embedding_fwd_drop_f32(const float* table, const int32_t* ids, float* out, float* out_drop,
                                   int32_t B, int32_t T, int32_t E, int32_t ldo, int32_t V, float rate,
                                   uint64_t seed, uint32_t site, uint32_t step, const uint32_t* step_dev,
                                   void* stream);
/* ... followed, when rate2 > 0, by a second mask in the same pass: the LSTM layer's per-call input dropout, whose call of
 * timestep t draws one mask over its (B, lwidth2) input from site2 + t; the text rows are its columns lcol0_2 .. lcol0_2 + E
 * (lc_NIC.py:255).  Bit-identical to tnt_embedding_fwd_drop_f32 + tnt_dropout_f32(rows_per_site = B).
 * lwidth2, lcol0_2 % 4 == 0. */
int32_t tnt_embedding_fwd_drop2_f32(const float* table, const int32_t* ids, float* out, float* out_drop,
                                    int32_t B, int32_t T, int32_t E, int32_t ldo, int32_t V, float rate,
                                    uint64_t seed, uint32_t site, uint32_t step, const uint32_t* step_dev,
                                    float rate2, uint32_t site2, int32_t lwidth2, int32_t lcol0_2, void* stream);
/* Single-process form of tnt_embedding_bwd_f32 without the table-wide zero fill and the row-norm launches: the first
 * occurrence of an id sums its rows into dtable[id] (deterministic, as above) and leaves its share of the IndexedSlices
 * squared norm in sq_part[k * ny + y] (ny = ceil(E / 256); tnt_embedding_bwd_parts(B, T, E) floats; their sum is the
 * norm of the un-deduplicated rows); rows that only the PREVIOUS step touched (prev_ids [B*T], -1 = none) are zeroed.
 * Contract: dtable starts zeroed and is written by nothing else between calls (no gradient all-reduce), prev_ids holds
 * the ids of the previous call (tnt_step_finalize_f32 copies them).  E % 4 == 0, 16-byte aligned rows.
 * drop_rate > 0: drows is the gradient w.r.t. the dropped-out Embedding output (the LSTM layer's input dropout of the
 * text call, NIC.py:131,140); the keep mask tnt_embedding_fwd_drop_f32 applied (element (b*T + t) * E + e of stream
 * (drop_seed, drop_site, *drop_step_dev)) is applied to the rows as they are read.
 * zero_id >= 0 (-1: none): the caller guarantees that every row of drows whose id is zero_id is zero -- Embedding(mask_zero=True)
 * in front of an LSTM that honours the mask (NIC.py:77,131,140: a masked step passes no gradient to its input); those rows
 * (~40 % of a padded caption batch, all of ONE id) are not read, dtable[zero_id] is written as zeros. */
int32_t tnt_embedding_bwd_parts(int32_t B, int32_t T, int32_t E);
int32_t tnt_embedding_bwd_sparse_f32(const float* drows, const int32_t* ids, const int32_t* prev_ids, float* dtable,
                                     float* sq_part, int32_t B, int32_t T, int32_t E, int32_t ldd, int32_t V,
                                     float drop_rate, uint64_t drop_seed, uint32_t drop_site,
                                     const uint32_t* drop_step_dev, int32_t zero_id, void* stream);
int32_t tnt_embedding_bwd_f32(const float* drows, const int32_t* ids, float* dtable,
                              float* sq_norm, float* rowsq_work, int32_t B, int32_t T,
                              int32_t E, int32_t ldd, int32_t V, void* stream);

/* ---- LSTM cell step, keras LSTM v2 semantics (lc_NIC.py:118-124,255; NIC.py:82-88,
 * 138-140), gate-interleaved layouts.
 * fwd:  z = xz[B][U][4] + h_prev[B][U] @ Ur[U][U][4] (+ ctx[B][D] @ Wc[D][U][4])
 *       i,f,o = sigmoid, g = tanh; c = f*c_prev + i*g; h = o*tanh(c)
 *       mask (nullable, int32 ids[B*T], column `mask_t`): rows with id==0 keep
 *       (h_prev,c_prev) and repeat out_prev (zeros if out_prev is null).
 *       Saves gates[B][U][4] (post-activation).  out (nullable) receives the
 *       sequence output of this step.  xz_bias (nullable, [U][4]) is added to xz inside the kernel, so that
 *       the input projection of all timesteps can be an epilogue-free GEMM. */
int32_t tnt_lstm_step_fwd_f32(const float* xz, const float* h_prev, const float* c_prev,
                              const float* Ur, const float* ctx, const float* Wc, int32_t D,
                              const int32_t* mask_ids, int32_t mask_T, int32_t mask_t,
                              const float* out_prev, float* h, float* c, float* out,
                              float* gates, int32_t B, int32_t U, const float* xz_bias, void* stream);
/* ---- LayerNormLSTMCell (tensorflow_addons 0.15 rnn.LayerNormLSTMCell; the use_layer_norm branch of lc_NIC.py:126-136):
 *   z = LN_kernel(x W) + LN_recurrent(h U) + b;  c' = LN_state(sig(f) c + sig(i) tanh(c~));  h' = sig(o) tanh(c')
 * The two 4U-wide LayerNorms are tnt_layernorm_fwd/bwd_f32 launches (dgamma = dbeta = NULL there: input gradient only)
 * around the matmuls; these two entry points are the cell: gate math + the state LayerNorm over U, and the reverse.
 * Gate-interleaved tensors [B][U][4] (zk, zr, gates, dz; bias [U][4]); chat = the normalised pre-affine state, istd [B].
 * bwd: dh = dh_a + dh_b + dh_c (each nullable), dcn_in (nullable) = gradient wrt the normalised state carried to the
 * next step; writes dz, dc_prev (gradient wrt the previous step's normalised state; may alias dcn_in) and dcnt = the
 * total gradient at the normalised state (its products with chat / its column sums over all steps are the state
 * norm's gamma / beta gradients).  U <= 4096. */
int32_t tnt_ln_lstm_cell_fwd_f32(const float* zk, const float* zr, const float* bias, const float* c_prev,
                                 const float* gamma_s, const float* beta_s, float* gates, float* chat,
                                 float* istd, float* c, float* h, int32_t B, int32_t U, float eps, void* stream);
int32_t tnt_ln_lstm_cell_bwd_f32(const float* dh_a, const float* dh_b, const float* dh_c, const float* dcn_in,
                                 const float* gates, const float* c_prev, const float* c, const float* chat,
                                 const float* istd, const float* gamma_s, float* dz, float* dc_prev,
                                 float* dcnt, int32_t B, int32_t U, void* stream);
/* Persistent form of the masked sequence forward of NIC.py:138-140: ONE launch runs the S dependent steps
 * (step s reads hs[s], cs[s], xz[s] and writes hs[s+1], cs[s+1], gates[s]; steps s >= mask_s0 write the sequence
 * output out[s - mask_s0] (out nullable) and, if mask_ids[B][mask_T] is given, are masked by its column s - mask_s0;
 * pass mask_s0 = S for neither).  hs/cs: [S+1][B][U] with slab 0 = the initial state; xz: [S][B][U][4]; gates: [S][B][U][4];
 * sync: 1025 uint32 of scratch owned by the caller, zeroed before first use and after an error, never in between (the
 * kernel re-arms its own counters when it ends, so a captured launch replays without any reset node; protocol in
 * csrc/tnt_seq_sync.h).  Word 1024 is the sticky error word: 1 = a barrier timed out, 2 = a launch did not place 32
 * workgroups on each XCD; results are invalid from then on.  guard_out (nullable): one float the kernel sets to the error
 * code when it sees the error word set (never cleared by the device), so the caller can carry the check along with
 * the metrics it reads anyway; tnt_step_tick / tnt_adam_f32 / tnt_sgd_f32 take the error word as `guard` and leave the
 * model state untouched when it is set.  S <= 64.  Same arithmetic as S calls of tnt_lstm_step_fwd_f32.  A step pays one XCD-local barrier instead of a
 * dependent kernel launch and the recurrent weights stay in VGPRs; needs U == 512, B <= 128 and a 256-CU device on
 * which a 256-workgroup launch places 32 workgroups on each of the 8 XCDs: tnt_lstm_seq_supported() tests exactly that
 * (one synchronising probe launch per process, so call it outside any graph capture) and returns 1 or 0.
 * out_pos (nullable; null: bit-identical to the call without it): the row map of tnt_stage_batch_map_f32, [S - mask_s0][B]
 * int32.  Sequence position (t, b) then writes its output to row out_pos[t*B + b] of `out` instead of row t*B + b, and
 * writes nothing where that is negative. */
int32_t tnt_lstm_seq_supported(int32_t B, int32_t U);
int32_t tnt_lstm_seq_fwd_f32(const float* xz, float* hs, float* cs, const float* Ur, const float* xz_bias,
                             const int32_t* mask_ids, int32_t mask_T, int32_t mask_s0, float* out,
                             float* gates, int32_t S, int32_t B, int32_t U, uint32_t* sync, float* guard_out,
                             const int32_t* out_pos, void* stream);
/* Persistent form of the BPTT chain of the same sequence (the S calls of tnt_lstm_step_bwd_f32 that nic.NIC makes, in
 * ONE launch): step s = S-1 .. 0 reads gates[s], cs[s+1], cs[s] and writes dz[s] ([S][B][U][4]); steps s >= mask_s0
 * add dout_seq[s - mask_s0] (gradient of the sequence output, nullable) and are masked by column s - mask_s0 of
 * mask_ids (nullable) exactly like the per-step kernel (masked row: dz = 0, the carried da / dc / dout pass through);
 * the carried output gradient is dropped below mask_s0 (NIC.py:138: the feature step's output is not part of the
 * sequence).  Weights stay in registers, the recurrent product is "pushed" as partial tiles through `work`
 * (tnt_lstm_seq_bwd_work_floats(B, U) floats, 16-byte aligned) inside one XCD per 16-row block; sync / guard_out and the
 * device requirements as tnt_lstm_seq_fwd_f32 (same sync buffer, launches on one stream).  Deterministic.
 * dout_pos (nullable; null: bit-identical to the call without it): the same row map; position (t, b) reads its output
 * gradient from row dout_pos[t*B + b] of dout_seq and takes zero where that is negative (the row it was merged into carries
 * its share: the chain hands a masked step's output gradient on to the last live step anyway). */
int32_t tnt_lstm_seq_bwd_work_floats(int32_t B, int32_t U);
int32_t tnt_lstm_seq_bwd_f32(const float* Ur, const float* dout_seq, const int32_t* mask_ids, int32_t mask_T,
                             int32_t mask_s0, const float* gates, const float* cs, float* dz, float* work,
                             int64_t work_floats, int32_t S, int32_t B, int32_t U, uint32_t* sync,
                             float* guard_out, const int32_t* dout_pos, void* stream);
/* bwd of one step, fused with the recurrent matmul of the step after it:
 *   da = da_pass_in + dh_ext + (dz_next ? dz_next[B][U][4] @ Ur^T : 0)
 *   dout = dout_in + dout_t ; masked rows pass (da, dc, dout) through, dz = 0
 *   unmasked rows: dh = da + dout, standard LSTM cell backward -> dz[B][U][4],
 *   dc_out = dc*f, da_pass_out = 0, dout_out = 0.
 * Any of dz_next, da_pass_in, dh_ext, dc_in, dout_in, dout_t, mask_ids may be null.
 * dctx_part (nullable; attention model): [U/16][B][D] partial context gradients of this step,
 *   dctx_part[ub][b][d] = sum over the 16 units of block ub and the 4 gates of dz[b][u][g] * Wc[d][u][g]
 *   (Wc = the context rows of the LSTM kernel, [D][U][4], D <= 64); tnt_attention_step_bwd_f32 sums the parts. */
int32_t tnt_lstm_step_bwd_f32(const float* dz_next, const float* Ur, const float* da_pass_in,
                              const float* dh_ext, const float* dc_in, const float* dout_in,
                              const float* dout_t, const int32_t* mask_ids, int32_t mask_T,
                              int32_t mask_t, const float* gates, const float* c,
                              const float* c_prev, float* dz, float* da_pass_out,
                              float* dc_out, float* dout_out, int32_t B, int32_t U,
                              const float* Wc, int32_t D, float* dctx_part, void* stream);

/* ---- GRU cell step, keras GRU v2 semantics (reset_after=True): the decoder of ThinkAndTell/att_model.py
 * (att_model.py:84-93,118).  Gate-interleaved layouts [..][U][4] with slots (z, r, h, 0 pad).
 * fwd:  rec = h_prev[B][U] @ Uk[U][U][4] + br[U][4];  z = sigmoid(xz_z + rec_z), r = sigmoid(xz_r + rec_r),
 *       hh = tanh(xz_h + r*rec_h);  h = z*h_prev + (1-z)*hh.   xz[B][U][4] = x @ W + b_i (one GEMM for all steps).
 *       Saves gates[B][U][4] = (z, r, hh, rec_h).
 * bwd:  dh = dh_ext + dh_pass_in + (drec_next ? drec_next[B][U][4] @ Uk^T : 0);
 *       dxz = (da_z, da_r, da_h, 0)  [input side: kernel / input-bias gradients, dX],
 *       drec = (da_z, da_r, da_h*r, 0)  [recurrent side: recurrent-kernel / recurrent-bias gradients, and the
 *       matmul the call of the step before applies];  dh_pass_out = dh*z.  Nullable: drec_next, dh_pass_in, dh_ext,
 *       dh_pass_out. */
int32_t tnt_gru_step_fwd_f32(const float* xz, const float* h_prev, const float* Uk, const float* br, float* h,
                             float* gates, int32_t B, int32_t U, void* stream);
int32_t tnt_gru_step_bwd_f32(const float* drec_next, const float* Uk, const float* dh_pass_in,
                             const float* dh_ext, const float* gates, const float* h_prev, float* dxz,
                             float* drec, float* dh_pass_out, int32_t B, int32_t U, void* stream);

/* ---- softmax + CategoricalCrossentropy(from_logits=False) + accuracy ------------
 * (lc_NIC.py:153,370-376,461-486; NIC.py:93,234-240; main.py:107-110)
 * logits [rows][ld], V valid columns.  target ids int32[rows] (argmax of the one-hot).
 * probs (nullable, may alias logits): softmax.  loss_row/correct_row [rows]:
 * -log(clip(p_y/sum p, 1e-7, 1-1e-7)) and (argmax p == y).  dlogits (nullable, may
 * alias logits): (p - onehot)*gscale, zero rows where the clip is active.
 * from_logits=1: tf SparseCategoricalCrossentropy(from_logits=True) (ThinkAndTell/train.py:262-263):
 * loss = logsumexp - x_y, no clipping.  mask_zero=1: rows whose target id is 0 give zero loss
 * and zero gradient (CaptionGenerator.loss_function, ThinkAndTell/model.py:319-334).
 * Pad columns [V, ld) of logits are ignored; those of an output are either left as they were or written
 * as zero (seqops.hip: softmax_cce_reg_kernel).  rows == 0 is a no-op; TNT_BADARG for rows < 0, V <= 0,
 * ld < V, null logits. */
int32_t tnt_softmax_cce_f32(const float* logits, const int32_t* target, float* probs,
                            float* loss_row, float* correct_row, float* dlogits,
                            int32_t rows, int32_t V, int32_t ld, float gscale,
                            int32_t from_logits, int32_t mask_zero, void* stream);
/* tnt_softmax_cce_f32(from_logits = 0, mask_zero = 0) over the distinct rows of a row map (tnt_stage_batch_map_f32): rows at
 * or past live[0] (one int32 in device memory, read when the launch runs) are neither read nor written; row r stands for
 * row_weight[r] identical positions, so loss_row[r], correct_row[r] and dlogits[r] are the plain values times row_weight[r].
 * `rows` is the size of the grid and must cover the largest value live[0] can take.  live and row_weight must be given. */
int32_t tnt_softmax_cce_live_f32(const float* logits, const int32_t* target, float* probs,
                                 float* loss_row, float* correct_row, float* dlogits,
                                 int32_t rows, int32_t V, int32_t ld, float gscale,
                                 const int32_t* live, const float* row_weight, void* stream);
/* ---- the same head with label smoothing: tf.keras.losses.CategoricalCrossentropy(from_logits=False,
 * label_smoothing=eps), one launch (smooth.hip).  With V classes, p = softmax(x) and target id y:
 *   ys_v      = (1 - eps) [v == y] + eps / V
 *   loss      = -sum_v ys_v log(clip(p_v, 1e-7, 1 - 1e-7))
 *   m_v       = 1 where the clip is inactive for class v (1e-7 <= p_v <= 1 - 1e-7), else 0;  c = sum_v m_v ys_v
 *   dlogits_v = gscale (c p_v - m_v ys_v)            (the gradient through keras's element-wise clip)
 * A target id outside [0, V) matches no class (ys_v = eps / V).  correct_row = (argmax == y), first maximum wins.
 * label_smoothing = 0 is tnt_softmax_cce_f32(from_logits=0, mask_zero=0) up to rounding.  No from_logits / mask_zero form.
 * Shared with tnt_softmax_cce_f32: every output is nullable (target null: probs only, loss_row / correct_row are not
 * written and dlogits, if given, is zero); probs or dlogits may alias logits; pad columns [V, ld) of logits are ignored
 * and those of an output are left as they were or written as zero (inside the register kernel's window); rows == 0 is
 * a no-op; TNT_BADARG for rows < 0, V <= 0, ld < V, null logits -- and for label_smoothing outside [0, 1) or not
 * finite. */
int32_t tnt_softmax_cce_smooth_f32(const float* logits, const int32_t* target, float* probs,
                                   float* loss_row, float* correct_row, float* dlogits,
                                   int32_t rows, int32_t V, int32_t ld, float gscale,
                                   float label_smoothing, void* stream);
/* ---- the same head with token-level unlikelihood (Welleck et al. 2020, "Neural Text Generation with Unlikelihood
 * Training"), one launch (unlikely.hip): besides raising p of the target word, every position lowers p of the words
 * that occurred earlier in the same caption.
 * Layout: logits [rows][ld], rows = T * B in t-major order: row r is position t = r / B of caption b = r % B; target
 *   int32[T * B] in the same order; V valid columns; p = softmax(x) over them.
 * Negative candidates of row (t, b): C = { target[j * B + b] : 0 <= j < t } taken as a set (a word that occurred twice
 *   counts once), without y = target[t * B + b], without id 0 (the padding) and without ids outside [0, V).  Row t = 0
 *   has none.  A padding position (y = 0) behind the end of a caption keeps its candidates.  The prefix is always what
 *   `target` holds, whatever ids were fed to the model.
 *   ce        = -log(clip(p_y, 1e-7, 1 - 1e-7))          exactly tnt_softmax_cce_f32(from_logits=0, mask_zero=0)
 *   ul        = -sum_{c in C} log(max(1 - p_c, 1e-7))
 *   loss_row  = ce + alpha ul
 *   m_y       = 1 where the clip of ce is inactive, else 0;   m_c = 1 where 1 - p_c >= 1e-7, else 0
 *   q_c       = m_c p_c / (1 - p_c);   Q = sum_{c in C} q_c
 *   dlogits_v = gscale (m_y (p_v - [v == y]) + alpha ([v in C] q_v - p_v Q))
 * A target id outside [0, V) matches no class (p_y = 0: ce = -log(1e-7), m_y = 0).
 * correct_row and probs as in tnt_softmax_cce_f32 (first maximum wins).  A row without candidates, or alpha = 0, is
 * tnt_softmax_cce_f32 up to rounding.  Shared with it: every output is nullable (target null: probs only, loss_row /
 * correct_row are not written and dlogits, if given, is zero); probs or dlogits may alias logits; pad columns [V, ld)
 * of logits are ignored and those of an output are left as they were or written as zero (inside the register kernel's
 * window).  alpha is finite and >= 0; 1 <= T <= 64 (one wave holds a caption's prefix); B == 0 is a no-op.  TNT_BADARG
 * for B < 0, T < 1 or T > 64, V <= 0, ld < V, null logits, alpha negative or not finite: a rejected call launches
 * nothing. */
int32_t tnt_softmax_cce_unlikely_f32(const float* logits, const int32_t* target, float* probs,
                                     float* loss_row, float* correct_row, float* dlogits,
                                     int32_t B, int32_t T, int32_t V, int32_t ld, float gscale,
                                     float alpha, void* stream);
/* ---- the same head with per-class token weights (keras fit(class_weight=)), the focal factor (Lin et al. 2017, "Focal
 * Loss for Dense Object Detection"; keras CategoricalFocalCrossentropy) and an optional normalisation by the weight sum
 * (the padding-masked, length-normalised caption loss), one launch (weighted.hip).  class_weight: float32[V] in device
 * memory, nullable (every weight 1), read when the launch runs.  With p = softmax(x) over the V valid columns and
 * y = target[r]:
 *   w_r       = class_weight[y] if class_weight is given and 0 <= y < V, else 1
 *   pc        = clip(p_y, 1e-7, 1 - 1e-7), p_y = 0 for y outside [0, V);   ce = -log pc
 *   m_y       = 1 where that clip is inactive, else 0          (these three: tnt_softmax_cce_f32(from_logits=0, mask_zero=0))
 *   f         = (1 - pc)^gamma;   g = f + gamma pc (1 - pc)^(gamma - 1) ce;   gamma == 0: f = g = 1 exactly (a branch, no powf)
 *               (computed as q = (1 - pc)^(gamma - 1), f = q (1 - pc); q is 1 resp. 1 - pc for gamma 1 and 2, without powf)
 *   W         = sum_r w_r over all `rows`;   k = 1 if normalise == 0, else rows / W, or 0 if W == 0
 *   loss_row[r]    = k w_r f ce
 *   correct_row[r] = [argmax == y] if normalise == 0, else k w_r [argmax == y]         (first maximum wins)
 *   dlogits[r][v]  = gscale k w_r m_y g (p_v - [v == y])
 * so the mean of loss_row over the rows is sum(w l) / rows (normalise = 0, keras's class_weight rule) or sum(w l) / sum(w)
 * (normalise = 1), and in the latter the mean of correct_row is the accuracy over the weighted tokens.  A row with w_r == 0
 * gives exactly 0 in loss_row, correct_row (normalise = 1) and dlogits, whatever k and its logits are.
 * W is float32, formed inside the launch in a fixed order that is part of the definition: accumulator t of 256 adds
 * w_t, w_(t+256), ... in ascending order starting from 0; the 64 accumulators of a wave (t / 64) are combined by the
 * butterfly lane ^ 32, 16, 8, 4, 2, 1; the four waves as (W0 + W1) + (W2 + W3).  k = (float)rows / W.  Without
 * class_weight W = rows and k = 1 exactly.  A weight is expected finite and >= 0 (the host checks; the kernel does not).
 * Shared with tnt_softmax_cce_f32: every output is nullable (target null: probs only, loss_row / correct_row are not
 * written and dlogits, if given, is zero); probs or dlogits may alias logits; pad columns [V, ld) of logits are ignored
 * and those of an output are left as they were or written as zero (inside the register kernel's window); rows == 0 is a
 * no-op.  TNT_BADARG for rows < 0, V <= 0, ld < V, null logits, gamma negative or not finite, normalise outside {0, 1}: a
 * rejected call launches nothing. */
int32_t tnt_softmax_cce_weighted_f32(const float* logits, const int32_t* target, const float* class_weight,
                                     float* probs, float* loss_row, float* correct_row, float* dlogits,
                                     int32_t rows, int32_t V, int32_t ld, float gscale,
                                     float gamma, int32_t normalise, void* stream);
/* ---- the same head mixed with knowledge distillation (Hinton et al. 2015, "Distilling the Knowledge in a Neural
 * Network"), one launch (distill.hip): a frozen teacher's temperature-softened distribution is a second target of every
 * row.  logits [rows][ld] (student x), teacher [rows][ld_teacher] (teacher logits u), V valid columns in both,
 * y = target[r], a = alpha in [0, 1], t = temperature > 0.  Per row:
 *   ce, m_y, p = softmax(x)   as tnt_softmax_cce_f32(from_logits=0, mask_zero=0): ce = -log(clip(p_y, 1e-7, 1 - 1e-7)),
 *                             m_y = 1 where that clip is inactive, else 0; a target id outside [0, V) matches no class
 *                             (p_y = 0: ce = -log(1e-7), m_y = 0)
 *   pt = softmax(x / t),  qt = softmax(u / t)   over the V valid columns
 *   kl        = sum_v qt_v (log qt_v - log pt_v), the logs taken from the logits ((u_v - max u) / t - log Zu, likewise
 *               for x), not from clipped probabilities: no clip in this term; a class with qt_v == 0 contributes exactly 0
 *   loss_row  = (1 - a) ce + a t^2 kl
 *   kl_row    = kl                                                   (unscaled)
 *   correct_row = (first argmax of x == y)
 *   dlogits_v = gscale ((1 - a) m_y (p_v - [v == y]) + a t (pt_v - qt_v))
 * alpha = 0 gives tnt_softmax_cce_f32's outputs up to rounding.  The teacher must be finite in the valid columns.
 * dlogits may alias logits.  teacher may not alias any output: TNT_BADARG when the pointers are equal.  Pad columns
 * [V, ld) of logits are ignored; pad columns [V, ld_teacher) of teacher are never read, not even as part of a float4; pad
 * columns of dlogits are left as they were or written as zero (inside the register kernel's window, which needs both
 * rows float4-addressable: ld % 4 == 0, ld_teacher % 4 == 0, 16-byte aligned pointers).  Every output is nullable.
 * rows == 0 is a no-op.  TNT_BADARG for rows < 0, V <= 0, ld < V, ld_teacher < V, null logits / teacher / target, alpha
 * outside [0, 1] or NaN, temperature not finite or <= 0: a rejected call launches nothing. */
int32_t tnt_softmax_cce_distill_f32(const float* logits, const float* teacher, const int32_t* target,
                                    float* loss_row, float* kl_row, float* correct_row, float* dlogits,
                                    int32_t rows, int32_t V, int32_t ld, int32_t ld_teacher,
                                    float gscale, float alpha, float temperature, void* stream);
/* target ids from a dense one-hot (B,T,V) float array: ids[t*B+b] = argmax_v (first max wins).
 * B == 0 or T == 0 is a no-op; TNT_BADARG for B < 0, T < 0, V <= 0, null pointers. */
int32_t tnt_onehot_argmax_f32(const float* onehot, int32_t* ids_tmajor, int32_t B, int32_t T,
                              int32_t V, void* stream);
/* Beam-search expansion (beam search is only sketched in the reference: lc_NIC.py:640-692,
 * ThinkAndTell/evaluate.py:203-228).  Rows b*k .. b*k+k-1 of probs [B*k][ld] are the k beams of sample b; candidate
 * (beam j, token v) scores score_in[j] + log(max(p, 1e-30)); a finished beam (fin_in != 0: it has emitted end_id)
 * only continues with token 0 at its own score.  The k best become the new beams (ties: lower j*V + v):
 * score_out, parent (global row of the extended beam), token, fin_out -- all [B*k].  k <= 16. */
int32_t tnt_beam_topk_f32(const float* probs, const float* score_in, const int32_t* fin_in, int32_t B,
                          int32_t V, int32_t ld, int32_t k, int32_t end_id, float* score_out,
                          int32_t* parent, int32_t* token, int32_t* fin_out, void* stream);
/* One beam-search step: the expansion of tnt_beam_topk_f32 and the reorder of the LSTM state by parent, in one launch
 * (restated by tests/dense_beam_oracle.py).  Definition:
 *  - Expansion: score_out, parent, token, fin_out [B*k] are exactly those of tnt_beam_topk_f32 for the same
 *    (probs, score_in, fin_in, B, V, ld, k, end_id), bit for bit for every finite score_in: candidate (beam j, token v)
 *    is the float32 value score_in[j] + logf(fmaxf(p, 1e-30f)); a finished beam (fin_in != 0) has one candidate, token
 *    0 at its own score; ties go to the lower flat index j*V + v; output in rank order, best first.
 *  - Reorder: h_out[r][0..U) = h_in[parent[r]][0..U) for every r < B*k, likewise c; plain bit copies, row stride ldh.
 *    U == 0 skips the reorder (the state pointers are then not read).  h_out / c_out must not overlap h_in / c_in:
 *    callers ping-pong the buffers.
 *  - k <= 16, any V.  One workgroup of 16 waves per sample, 16 / k waves per beam row; each workgroup touches only its
 *    own sample's rows.  Deterministic, no scratch memory, no host sync.
 * TNT_BADARG for B <= 0, V <= 0, k < 1, k > 16, ld < V, U < 0, ldh < U, score_out == score_in, fin_out == fin_in, and
 * (U > 0) a null state pointer or an output state buffer that overlaps an input one. */
int32_t tnt_beam_step_f32(const float* probs, int32_t ld, const float* score_in, const int32_t* fin_in, int32_t B,
                          int32_t V, int32_t k, int32_t end_id, float* score_out, int32_t* parent, int32_t* token,
                          int32_t* fin_out, const float* h_in, const float* c_in, int32_t ldh, int32_t U,
                          float* h_out, float* c_out, void* stream);
/* One step of diverse (group) beam search with Hamming diversity (Vijayakumar et al. 2016/2018; num_beam_groups /
 * diversity_penalty in the common toolkits), in one launch (restated by tests/diverse_beam_oracle.py).  Library-defined:
 *  - Layout.  The k beams of a sample are `groups` = Gd groups of k' = k / Gd: group g of sample b owns rows
 *    b*k + g*k' + j, j < k', of every [B*k] buffer.
 *  - Order.  Within the step the groups of a sample choose in ascending g.
 *  - Candidates of group g: (beam j of the group, token v).  Its score is the float32 s = score_in[j] +
 *    logf(fmaxf(p, 1e-30f)), exactly as in tnt_beam_step_f32; its selection key is the float32 s - lambda * (float)n_v
 *    (a rounded product, then a rounded difference), where n_v counts the new beams already chosen at this step by the
 *    groups < g of the same sample whose token is v and whose parent was live (fin_in == 0).
 *  - A finished beam (fin_in != 0) has one candidate, token 0 at its own score, key = score; it adds to no n_v.
 *  - Selection.  The k' best keys of the group become its new beams, best first, at the group's rows; ties go to the
 *    lower j*V + v.
 *  - Outputs.  score_out is the unpenalised s: carried scores stay sums of log-probabilities and the penalty steers the
 *    selection only.  parent is the global row of the extended beam; token and fin_out as in tnt_beam_step_f32.
 *  - Reorder: h_out[r][0..U) = h_in[parent[r]][0..U), likewise c; U == 0 skips it; aliasing rules of tnt_beam_step_f32.
 * Consequences: with lambda == 0 the launch is tnt_beam_step_f32(B*Gd, k') on the same buffers, bit for bit (the row
 * layouts coincide); with Gd == 1 it is tnt_beam_step_f32(B, k), bit for bit, for any lambda; for any lambda group 0 is
 * a plain beam search of width k'.
 * k <= 16, any V.  One workgroup of 16 waves per sample: every row's (g+1)*k' best values are prepared once for all groups
 * (the penalty only lowers keys, so a group's k' best keys are among them), then the groups rank their prepared
 * candidates in LDS in turn.  Deterministic, no scratch memory, no host sync.
 * TNT_BADARG for everything tnt_beam_step_f32 refuses, groups < 1, k % groups != 0, lambda < 0 or not finite. */
int32_t tnt_beam_step_diverse_f32(const float* probs, int32_t ld, const float* score_in, const int32_t* fin_in,
                                  int32_t B, int32_t V, int32_t k, int32_t end_id, float* score_out, int32_t* parent,
                                  int32_t* token, int32_t* fin_out, const float* h_in, const float* c_in, int32_t ldh,
                                  int32_t U, float* h_out, float* c_out, int32_t groups, float lambda, void* stream);
/* Constrained decoding: the repetition penalty and the bans of one decode step, applied to the step's logits in place,
 * in front of the softmax launch (restated by tests/constrain_oracle.py).  Library-defined:
 *  - Step and history.  logits [rows][ld], V valid columns, are the logits of step i (0-based: the step chooses the token
 *    at position i).  The history h_0 .. h_{i-1} of row r is the tokens chosen so far on the row's path, the start token
 *    not among them.  The caller owns two [rows][ldh] int32 buffers used in ping-pong: this launch forms
 *      hist_out[r][0..i) = hist_in[parent[r]][0..i-1) ++ last_token[r]
 *    (last_token[r]: the token chosen at step i-1; parent[r]: the global row that r continues, as tnt_beam_step_f32 /
 *    tnt_beam_topk_f32 write it; parent == NULL: r itself; a parent outside [0, rows) counts as r) and applies the rules
 *    from it.  Two dependent loads per row; the beam reorder of the history happens in this launch.  hist_out is written
 *    for every row, finished ones included.  i == 0: no history, hist_in / last_token are not read.  The two buffers
 *    must not overlap anywhere in their [rows][ldh] extents: one row's wave reads hist_in[parent[r]] while another's
 *    writes its hist_out row.
 *  - Rules, in this order, on each logit x_v as a float32:
 *    1. repetition penalty theta >= 1 (1 = off): for every DISTINCT v in the history, x_v <- x_v / theta if x_v > 0,
 *       else x_v * theta: once per distinct token, one correctly rounded float32 operation (NaN stays NaN);
 *    2. bans, x_v <- -inf, overriding 1:
 *       - every v of bad_ids [n_bad], at every step;
 *       - v == end_id while i < m (the minimum length);
 *       - no-repeat n-gram, n >= 1 (0 = off): for every s with s + n - 1 <= i - 1 whose h_s .. h_{s+n-2} equal the last
 *         n - 1 tokens h_{i-n+1} .. h_{i-1}, the token h_{s+n-1}.  n == 1 bans every history token; i < n bans nothing.
 *         The ids are compared as stored.
 *    The ban value is -inf: tnt_softmax_cce_f32 turns it into probability exactly 0.0f (checked by
 *    tests/test_gpu_constrain.py).
 *  - A row with fin[r] != 0 (fin nullable: beam search's finished flags) keeps its logits.  Columns [V, ld) are never
 *    written; no other logit changes.  An id outside [0, V), in the history, in bad_ids or as end_id, is ignored: nothing
 *    is read or written for it (in the history it still takes part in the n-gram comparison).
 *  - One wave per row, lane j holding h_j: i <= 64, n_bad <= 64.  First occurrences by wave shuffles; every address is
 *    stored by a lane that has decided its final value and every store to one address carries the same value, so no
 *    order between lanes is relied on.  No atomics, no LDS, no scratch memory; deterministic.
 * TNT_BADARG for rows <= 0, V <= 0, ld < V, ldh < max(i, 1), i < 0, i > 64, theta < 1 or not finite, n < 0, m < 0, m > 0
 * with end_id < 0, n_bad outside [0, 64], null logits, null hist_in or last_token with i > 0, null hist_out, null bad_ids
 * with n_bad > 0, hist_in == hist_out or any overlap of their [rows][ldh] extents; nothing is launched then. */
int32_t tnt_decode_constrain_f32(float* logits, int32_t ld, int32_t V, int32_t rows, int32_t i, const int32_t* hist_in,
                                 int32_t* hist_out, int32_t ldh, const int32_t* last_token, const int32_t* parent,
                                 const int32_t* fin, float theta, int32_t n, int32_t m, int32_t end_id,
                                 const int32_t* bad_ids, int32_t n_bad, void* stream);
/* Consensus decoding: the next-word distributions of the G member rows of one mixed row -- several scans of the same
 * image, or the subjects of the multi-subject model -- combined into one, where softmax + argmax sit in a plain decode
 * (restated by tests/consensus_oracle.py).  Library-defined:
 *  - Layout.  Member-major: logits [G*Rm][ld], V valid columns, are the step's logits (behind tnt_decode_constrain_f32,
 *    if any); member g of mixed row r is row g*Rm + r.  mix [Rm][ldm] receives the mixture; columns [V, ldm) are never
 *    written.  w [G] are the member weights, positive and summing to 1 (the caller's duty); NULL: 1/G each.
 *  - Per member row, in float32: m_g = max_v x_gv, s_g = sum_v exp(x_gv - m_g).  A member row with nothing above -inf
 *    counts as m_g = 0, s_g = 1: each of its columns is then -inf like any banned one.
 *  - mode 0 (mean of softmaxes):  p_v = sum_g w_g * exp(x_gv - m_g) / s_g, accumulated in ascending g.
 *    mode 1 (logmean, the renormalised geometric mean):  l_v = sum_g w_g * ((x_gv - m_g) - log s_g) in ascending g,
 *    p_v = exp(l_v - L) / sum_v exp(l_v - L), L = max_v l_v.
 *    A -inf logit gives probability exactly 0.0f: in mean only when every member bans the column, in logmean when any
 *    does.  A logmean row whose every l_v is -inf gets p = 0 everywhere and token 0.
 *  - token (nullable) [G*Rm]: the argmax of p_r under the rules of tnt_argmax_rows_f32 (first max wins, NaN entries are
 *    ignored, nothing above -inf gives 0), written to all G member rows g*Rm + r: the word fed back to every member.
 *  - One workgroup per mixed row, 1 <= G <= 16; fixed summation orders, no atomics, no scratch memory: deterministic.
 * TNT_BADARG for Rm <= 0, V <= 0, ld < V, ldm < V, G outside [1, 16], mode other than 0 or 1, null logits or mix, mix
 * overlapping logits anywhere in their extents; nothing is launched then. */
int32_t tnt_consensus_mix_f32(const float* logits, int32_t ld, int32_t V, int32_t Rm, int32_t G, const float* w,
                              int32_t mode, float* mix, int32_t ldm, int32_t* token, void* stream);
/* What a step chose on the Rm mixed rows (tnt_sample_topkp_f32 / tnt_sample_rows_f32 / tnt_beam_topk_f32 /
 * tnt_beam_step_f32) carried to the G*Rm member rows: token_out[g*Rm + r] = token[r] (the fed-back word),
 * parent_out[g*Rm + r] = parent[r] + g*Rm (the member's row of the parent beam: the state gather and the history gather
 * of tnt_decode_constrain_f32), fin_out[g*Rm + r] = fin[r].  Each of token / parent / fin is nullable and skipped then
 * (all three null: no launch).  TNT_BADARG for Rm <= 0, G outside [1, 16], an input without its output. */
int32_t tnt_consensus_spread_i32(const int32_t* token, const int32_t* parent, const int32_t* fin, int32_t Rm, int32_t G,
                                 int32_t* token_out, int32_t* parent_out, int32_t* fin_out, void* stream);
/* Classifier-free guidance (context-aware / contrastive decoding) for caption decoding: the next-word distribution
 * given the scan contrasted with the one the same model gives for a null scan, where softmax + argmax sit in a plain
 * decode (restated by tests/guidance_oracle.py).  Library-defined:
 *  - Layout.  The consensus layout with G = 2, member-major: logits [2*Rm][ld], V valid columns, are the step's logits
 *    (behind tnt_decode_constrain_f32, if any); row r is the conditional row (the scan), row Rm + r its null row.  mix
 *    [Rm][ldm] receives the guided distribution; columns [V, ldm) are never written and logits is read only.
 *  - Per row, in float32: m = max_v x_v, s = sum_v exp(x_v - m), l_v = (x_v - m) - log s; lc the conditional row's
 *    values, ln the null row's.  A row with nothing above -inf counts as m = 0, s = 1: each of its l_v is then -inf.
 *  - Guided logit: g_v = lc_v + scale * (lc_v - ln_v) where both are finite, as one fused multiply-add
 *    fma(scale, lc_v - ln_v, lc_v).  lc_v = -inf gives g_v = -inf (a ban stays a ban; inf - inf is never formed);
 *    ln_v = -inf with lc_v finite gives g_v = lc_v (the contrast term is dropped).
 *  - Plausibility mask (Li et al. 2022): with plaus > 0 every v with lc_v < log(plaus) + max_v lc_v gets g_v = -inf;
 *    max_v lc_v is the conditional maximum's own value 0 - log s, so the conditional row's first maximum is always
 *    kept.  plaus == 0: no mask.
 *  - p_v = exp(g_v - Gm) / sum_v exp(g_v - Gm), Gm = max_v g_v.  A -inf guided logit gives exactly 0.0f; a row whose
 *    every g_v is -inf gets p = 0 everywhere and token 0.
 *  - token (nullable) [2*Rm]: the argmax of p_r under the rules of tnt_argmax_rows_f32 (first max wins, nothing above
 *    -inf gives 0), written to both r and Rm + r: the word fed back to the scan's row and to the null row.
 *  - One workgroup per mixed row, both member rows read once; fixed summation orders, no atomics, no scratch memory:
 *    deterministic.
 * TNT_BADARG for Rm <= 0, V <= 0, ld < V, ldm < V, scale not finite or < 0, plaus not finite or outside [0, 1), null
 * logits or mix, mix overlapping logits anywhere in their extents; nothing is launched then. */
int32_t tnt_guidance_mix_f32(const float* logits, int32_t ld, int32_t V, int32_t Rm, float scale, float plaus,
                             float* mix, int32_t ldm, int32_t* token, void* stream);
/* Minimum Bayes risk caption selection (Eikema & Aziz 2020, sampling-based MBR): of the Nc candidate captions of a scan
 * the one with the highest expected n-gram utility against the first Nr of them, the pseudo-references (restated by
 * tests/mbr_oracle.py).  Library-defined:
 *  - Layout.  ids [Nc][L][ld] int32: candidate c of scan b at position t is ids[(c*L + t)*ld + b], the (max_len, rows)
 *    layout of a decode's ids stacked Nc times; B scans, ld >= B, columns [B, ld) are never read (the member rows of a
 *    consensus or guided decode).  ids is read only.  Tokens are only compared: any int32 value is safe.
 *  - Caption.  A candidate's caption is its tokens before the first end_id or 0 (SelfCritical.truncate's rule); end_id < 0:
 *    only 0 terminates.  What follows the terminator is ignored.  Its length is len, 0 <= len <= L.
 *  - Match counts, exact integers.  For k = 1..order: c_k(h, r) = sum over the distinct k-grams g of h of
 *    min(count_h(g), count_r(g)), and tot_k(x) = max(len_x - k + 1, 0).
 *  - kind 0 ("ngram-f"):  F_k = 2*c_k / (tot_k(h) + tot_k(r)), one float32 division of the two integers, 0 when the
 *    denominator is 0; u(h, r) = (F_1 + ... + F_order) / order, summed in ascending k in float32.  Symmetric bit for bit.
 *  - kind 1 ("bleu"):  u(h, r) = evaluate.sentence_bleu([r], h, weights=(1/order,)*order), method-1 smoothing with epsilon
 *    0.1, in float32: 0 for an empty h or c_1 = 0; else s = sum_k (1/order) * log(n_k / max(1, tot_k(h))) in ascending k,
 *    n_k = c_k or 0.1 where c_k = 0, and u = bp * exp(s), bp = exp(1 - len_r/len_h) when len_h <= len_r, else 1.
 *  - Expected utility.  All Nc candidates are hypotheses, 1 <= Nr <= Nc: E[b][i] = (sum_{j < Nr} u(i, j)) / Nr, the float32
 *    utilities accumulated in ascending j in float64 and rounded to float32 once, behind the division.  The self term is
 *    included when i < Nr, so that two identical hypotheses get bit-identical E.
 *  - best [B]: the first maximum of E[b][:] (the smallest index wins).
 *  - Outputs: expected [B][Nc] float32; best [B] int32; out_ids (nullable) [L][ldo] int32, ldo >= B: column b receives the
 *    chosen candidate's L tokens verbatim, columns [B, ldo) are untouched; match (nullable) [B][Nc][Nr][order] int32, the
 *    c_k; util (nullable) [B][Nc][Nr] float32.
 *  - One workgroup per scan, the scan's tokens staged once in LDS, the pairs dealt over the threads; integer compares
 *    only in the inner loop; no atomics, no scratch memory, fixed summation orders: deterministic.
 * TNT_BADARG for B <= 0, ld < B, Nc outside [1, 64], Nr outside [1, Nc], L outside [1, 64], order outside [1, 4], kind other
 * than 0 or 1, null ids / expected / best, ldo < B with out_ids, any output overlapping ids anywhere in their extents;
 * nothing is launched then. */
int32_t tnt_mbr_select_f32(const int32_t* ids, int32_t ld, int32_t B, int32_t Nc, int32_t Nr, int32_t L, int32_t end_id,
                           int32_t order, int32_t kind, float* expected, int32_t* best, int32_t* out_ids, int32_t ldo,
                           int32_t* match, float* util, void* stream);
/* Caption rewards of the self-critical step, scored on the device (nic.NIC(self_critical=SelfCritical(score_on="device")));
 * restated by tests/reward_oracle.py): the CIDEr-D or BLEU-4 score of the K sampled captions of each of B scans (and of its
 * greedy caption) against the scan's references, and the advantages tnt_scst_cce_f32 reads.  Library-defined:
 *  - Candidates.  R = B*K samples, row b*K + k = sample k of scan b: its T tokens are fed[r*T + 1 .. r*T + T-1] and then
 *    last[r] (the layout tnt_scst_cce_f32 reads; fed[r*T] is never read).  baseline 0 ("greedy") adds candidate K of scan
 *    b, greedy[t*ldg + b], t < T, ldg >= B; greedy is not read with baseline 1.
 *  - References.  refs [B][M][Lr] int32, zero padded: reference j < n_refs[b] of scan b at position t is
 *    refs[(b*M + j)*Lr + t]; n_refs[b] is clamped to [0, M]; the rows j >= n_refs[b] are never read.
 *  - Caption.  A candidate's or a reference's caption is its tokens before the first end_id or 0 (SelfCritical.truncate's
 *    rule); end_id < 0: only 0 terminates.  Its length is len.  counted[r] = min(len_r + 1, T): the positions up to and
 *    including the first terminator (SelfCritical.counted).
 *  - Tokens are only compared, or packed into a key: any int32 value is safe.  tf_x(g): the number of times the k-gram g
 *    (k = 1..4) occurs in caption x, an exact integer, full int32 words compared.
 *  - Table (kind 0).  The k-gram w0..w(k-1) of words in [1, 65535] has the key w0 | w1<<16 | w2<<32 | w3<<48 (missing high
 *    words zero).  keys [n_keys] uint64, strictly ascending; idf [n_keys] float64; params = {log(ndoc), sigma} float64.
 *    idf(g) = idf[i] where keys[i] is g's key, and log(ndoc) for a gram that is not in the table or holds a word outside
 *    [1, 65535].  n_keys = 0 is legal (keys and idf are not read then).  evaluate.RewardTable builds it.
 *  - kind 0 (CIDEr-D, evaluate.CiderD._score with the table's frequencies), all float64.  For candidate c, reference j,
 *    order k: num = sum over the distinct k-grams g of c, in the order of their first positions, of
 *    min(tf_c(g)*idf(g), tf_j(g)*idf(g)) * tf_j(g)*idf(g); nrm_x = sum over the distinct k-grams of x of (tf_x(g)*idf(g))^2;
 *    sim(c, j) = (sum_k (nrm_c*nrm_j != 0 ? num / sqrt(nrm_c*nrm_j) : 0) * exp(-(len_c - len_j)^2 / (2 sigma^2))) / 4;
 *    score(c) = 10 * (sum_j sim(c, j)) / n_refs in ascending j; 0 with no references.
 *  - kind 1 (BLEU-4, evaluate.sentence_bleu(refs, c, weights=(0.25,)*4, smoothing="method1", epsilon=0.1)), float64:
 *    n_k = sum over the distinct k-grams g of c of min(tf_c(g), max_j tf_j(g)); 0 for an empty c, n_1 = 0 or no references;
 *    else bp * exp(sum_k 0.25 * log((n_k or 0.1 where n_k = 0) / max(1, len_c - k + 1))), bp = 1 when len_c > rl, else
 *    exp(1 - rl/len_c), rl the reference length closest to len_c, the shorter on a tie.
 *  - adv [R] float32: adv[b*K + k] = float32(score(k) - base): base = score(greedy) with baseline 0; with baseline 1
 *    ("mean") ((sum of the scan's K sample scores in ascending k) - score(k)) / (K - 1), K >= 2.
 *  - score (nullable) [B][K+1] float64: the K sample scores, then the greedy caption's (0 with baseline 1).
 *  - One workgroup per scan, its rows staged once in LDS; counting, first-occurrence detection and the binary search of
 *    keys are integer work, everything floating-point is float64 and only adv is rounded; no atomics, no scratch memory,
 *    fixed summation orders: deterministic.
 * TNT_BADARG for B <= 0, T or Lr outside [1, 64], K outside [1, 16] (or K < 2 with baseline 1), M outside [1, 8], kind or
 * baseline other than 0 or 1, n_keys < 0, null fed / last / refs / n_refs / adv / counted, null greedy or ldg < B with
 * baseline 0, null params with kind 0, null keys / idf with kind 0 and n_keys > 0, any output overlapping an input or
 * another output anywhere in their extents; nothing is launched then. */
int32_t tnt_caption_reward_f32(const int32_t* fed, int32_t T, const int32_t* last, const int32_t* greedy, int32_t ldg,
                               const int32_t* refs, const int32_t* n_refs, int32_t M, int32_t Lr, const uint64_t* keys,
                               const double* idf, int32_t n_keys, const double* params, int32_t B, int32_t K,
                               int32_t end_id, int32_t kind, int32_t baseline, float* adv, double* score,
                               int32_t* counted, void* stream);
/* ROUGE-L of captions on the device (Lin 2004; the self-critical reward "rouge-l", evaluate.device_scores(kind="rouge-l")
 * and the validation metric of fit(validation_captions=...); restated by tests/rouge_oracle.py): the longest common
 * subsequence of the K sampled captions of each of B scans (and of its greedy caption) with the scan's references, the
 * F-score of pycocoevalcap's Rouge.calc_score, and the advantages tnt_scst_cce_f32 reads.  Library-defined:
 *  - Candidates, references, captions and counted: word for word as tnt_caption_reward_f32 defines them.  R = B*K samples,
 *    row b*K + k = sample k of scan b: its T tokens are fed[r*T + 1 .. r*T + T-1] and then last[r] (fed[r*T] is never
 *    read).  baseline 0 ("greedy") adds candidate K of scan b, greedy[t*ldg + b], t < T, ldg >= B; greedy is not read with
 *    baseline 1.  refs [B][M][Lr] int32, zero padded: reference j < n_refs[b] of scan b at position t is
 *    refs[(b*M + j)*Lr + t]; n_refs[b] is clamped to [0, M]; the rows j >= n_refs[b] are never read.  A candidate's or a
 *    reference's caption is its tokens before the first end_id or 0; end_id < 0: only 0 terminates.  Its length is len.
 *    counted[r] = min(len_r + 1, T).
 *  - Tokens are only compared, full int32 words: any int32 value is safe.
 *  - lcs(c, j): the length of the longest common subsequence of the captions of candidate c and reference j, an exact
 *    integer in [0, min(len_c, len_j)].  lcs (nullable) [B][K+1][M] int32: lcs[(b*(K+1) + c)*M + j]; the rows
 *    j >= n_refs[b] get 0, and with baseline 1 the row c = K gets 0.
 *  - score(c), float64, every operation below rounded on its own (no fused multiply-add), in this order:
 *      P = R = 0; for j = 0 .. n_refs-1 with len_j > 0, ascending:  P = max(P, lcs(c, j) / len_c), R = max(R, lcs(c, j) / len_j)
 *      (the two maxima are taken separately: they may come from different references);
 *      b2 = beta * beta;  num = ((1 + b2) * P) * R;  den = R + b2 * P;  score = num / den.
 *    The score is 0 for an empty candidate (len_c = 0), with no reference that holds a word, or when P == 0 (then R == 0
 *    too).  It lies in [0, 1]; beta = 1.2 is pycocoevalcap's.  beta is a HOST pointer to one float64, read during the call
 *    (a float64 travels by address in this ABI, as tnt_weight_average_f32's momentum does), so that the entry can check it.
 *  - adv [R] float32, score (nullable) [B][K+1] float64: as tnt_caption_reward_f32 forms them from the scores:
 *    adv[b*K + k] = float32(score(k) - base), base = score(greedy) with baseline 0; with baseline 1 ("mean") ((sum of the
 *    scan's K sample scores in ascending k) - score(k)) / (K - 1), K >= 2.  score holds the K sample scores, then the
 *    greedy caption's (0 with baseline 1).
 *  - One workgroup per scan, its rows staged once in LDS, one wave per (candidate, reference) pair: lane i holds the
 *    candidate's token i, the match vector of a reference word is one 64-lane ballot, and the LCS follows from the
 *    bit-vector recurrence V <- (V + (V & M)) | (V - (V & M)) over the reference's words (Allison & Dix 1986, Hyyro 2004)
 *    as the number of zero bits of V below len_c.  Integer work only up to the score; no atomics, no scratch memory, fixed
 *    order: deterministic.
 * TNT_BADARG for B <= 0, T or Lr outside [1, 64], K outside [1, 16] (or K < 2 with baseline 1), M outside [1, 8], baseline
 * other than 0 or 1, null beta, *beta (or its square) not finite or *beta <= 0, null fed / last / refs / n_refs / adv / counted, null
 * greedy or ldg < B with baseline 0, any output (adv, score, counted, lcs) overlapping an input or another output anywhere
 * in their extents; nothing is launched then. */
int32_t tnt_caption_rouge_f32(const int32_t* fed, int32_t T, const int32_t* last, const int32_t* greedy, int32_t ldg,
                              const int32_t* refs, const int32_t* n_refs, int32_t M, int32_t Lr, int32_t B, int32_t K,
                              int32_t end_id, const double* beta, int32_t baseline, float* adv, double* score,
                              int32_t* counted, int32_t* lcs, void* stream);
/* row argmax (first max wins; NaN entries are ignored, a row with no value above -inf gives 0), out int32[rows].
 * rows == 0 is a no-op; TNT_BADARG for rows < 0, V <= 0, ld < V, null pointers. */
int32_t tnt_argmax_rows_f32(const float* x, int32_t* out, int32_t rows, int32_t V, int32_t ld,
                            void* stream);
/* Greedy feedback step of the free-running decoder (lc_NIC.call_naive_attention, lc_NIC.py:175-221), one launch per
 * step with no host round trip.  logits [B][ld] (V valid columns, ld >= V) are step i's output rows; table [V][E] the
 * Embedding; w [E][ldw] (N columns) the text rows of the LSTM input kernel (gate-interleaved layout).
 *   fed[b*T + col] = id_b = argmax over the row's V logits: ties go to the lowest index, NaN never wins, and the id is
 *                    always in [0, V) (a row without a winner, e.g. all NaN, gives 0);
 *   text[b][0..E)  = table[id_b] * keep / (1 - rate): the LSTM layer's per-call input mask of step col, i.e. the decision
 *                    tnt_dropout_f32(rows_per_site = B) makes for row b, columns lcol0 .. lcol0 + E of the logical
 *                    (B, lwidth) input, stream (seed, site, step + *step_dev); rate 0: no mask;
 *   xz[b][0..N)    = text[b] . w  (no bias).
 * The argmax is over the logits, not the probabilities the reference takes it over: the two differ only where two
 * distinct logits round to the same float32 probability.  E % 4 == 0, E <= 1016, ldt % 4 == 0, table / text 16-byte
 * aligned; rate > 0 needs lwidth, lcol0 % 4 == 0. */
int32_t tnt_greedy_feedback_f32(const float* logits, int32_t ld, int32_t V, const float* table, int32_t E,
                                const float* w, int32_t ldw, int32_t N, int32_t* fed, int32_t T, int32_t col,
                                float* text, int32_t ldt, float* xz, int32_t ldz, int32_t B, float rate,
                                uint64_t seed, uint32_t site, uint32_t step, const uint32_t* step_dev,
                                int32_t lwidth, int32_t lcol0, void* stream);
/* Scheduled sampling (Bengio et al. 2015) for the dense caption model's training step (nic.NIC(scheduled_sampling=...)),
 * one launch per LSTM step, no host sync; restated by tests/ss_oracle.py.  This library's definition:
 *  - Schedule.  i = *counter (int64: the updates applied so far, the model's adam_t) and sched[0..3) (float64) are
 *    read on the device when the launch runs, so a recorded plan or a hipGraph replays with the live values.  kind 0,
 *    linear(p0 = sched[0], slope = sched[1], p_max = sched[2]): p = clip(p0 + slope * i, 0, p_max); kind 1,
 *    inverse_sigmoid(k = sched[0], p_max = sched[2]): p = p_max * (1 - k / (k + exp(i / k))).  p is computed in float64
 *    and rounded once to float32.  The parameters are the caller's to validate (finite, p0 and p_max in [0, 1], k >= 1:
 *    model_base.ScheduledSampling).
 *  - Step.  LSTM step t = j + 1 consumes token position j and its logits row predicts position j + 1; this launch is the
 *    one for col = j + 1 (1 <= col < T), logits [B][ld] (V valid columns) being step t's rows.
 *  - Coin.  Row b feeds the model's token iff element b of the Philox stream (seed, coin_site, step + *step_dev) is
 *    dropped at rate p by tnt_keep's rule: (w >> 8) < ceil(p * 2^24).  p = 0 never feeds the model's token, p = 1 always.
 *  - Model token.  mode 0 (greedy): the argmax of the logits row, ties to the lowest index, NaN never wins (the rule of
 *    tnt_greedy_feedback_f32).  mode 1 (sample): the draw of tnt_sample_rows_f32 on the logits at temperature 1, with the
 *    uniform of element b of the stream (seed, draw_site, step + *step_dev); the same id as that kernel.  The id is always
 *    in [0, V) (a row without a winner gives 0).
 *  - Write-back.  A model row writes its id to fed[b*T + col]; a ground-truth row leaves fed as it is and uses fed[b*T + col]
 *    (clamped to [0, V)).  text[b] = table[id] through the LSTM input mask of tnt_greedy_feedback_f32 (site, lwidth, lcol0,
 *    rate; the teacher-forced mask of (b, col) is lwidth = T*E, lcol0 = col*E), xz[b][0..N) = text[b] . w (no bias), for
 *    every row; the projection is the same code, and the same bits, as tnt_greedy_feedback_f32's.
 *  - Rows whose coin picks the ground truth do not read their logits.  Workgroups of 16 rows x 128 columns; deterministic,
 *    no scratch memory.
 * TNT_BADARG for the conditions of tnt_greedy_feedback_f32, col < 1, null pointers, an unknown kind or mode. */
int32_t tnt_scheduled_feedback_f32(const float* logits, int32_t ld, int32_t V, const float* table, int32_t E,
                                   const float* w, int32_t ldw, int32_t N, int32_t* fed, int32_t T, int32_t col,
                                   float* text, int32_t ldt, float* xz, int32_t ldz, int32_t B, float rate,
                                   uint64_t seed, uint32_t site, uint32_t step, const uint32_t* step_dev,
                                   int32_t lwidth, int32_t lcol0, int32_t kind, int32_t mode, const double* sched,
                                   const int64_t* counter, uint32_t coin_site, uint32_t draw_site,
                                   void* stream);
/* Scheduled sampling for the attention caption model's training step (lc_nic.NIC(scheduled_sampling=...)); restated by
 * tests/ss_att_oracle.py.  tnt_scheduled_feedback_f32 with one more mask: the gathered row table[id] is multiplied first by
 * the keep / scale of element b*lwidth_t + lcol0_t + e of the stream (seed, site_t, step + *step_dev) at rate_t, then by
 * the LSTM input mask of tnt_scheduled_feedback_f32 (rate, site, lwidth, lcol0).  Both are tnt_keep's rule, each a
 * multiplication by 1 / (1 - rate) where kept and 0 where dropped, in this order: the order and the arithmetic of
 * tnt_embedding_fwd_drop2_f32, so a row gets the same bits as that kernel's row (b, col) when
 *   rate_t = the text Dropout's rate, site_t = its site, lwidth_t = T*E, lcol0_t = col*E  (element (b*T + col)*E + e of the
 *     logical (B, T, E) caption tensor), and
 *   rate = the LSTM's input rate, site = site2 + col, lwidth = lwidth2, lcol0 = lcol0_2  (the per-call mask of step col).
 * The model's definition, for LSTM step t (token position t; its logits row predicts position t + 1) and col = 1 .. T-1:
 *  - p from the live counter (float64, rounded once to float32); row b's coin is element b of (seed, S_SS_COIN + col - 1,
 *    step + drop_step) and it feeds the model's token iff (w >> 8) < ceil(p * 2^24);
 *  - the model's token is the argmax of step col-1's logits (ties to the lowest index, NaN never wins), or in sample mode
 *    tnt_sample_rows_f32's draw at temperature 1 on (seed, S_SS_DRAW + col - 1, step + drop_step);
 *  - otherwise the row keeps cap[b, col] (clamped to [0, V)), not written back, its logits not read;
 *  - text = table[id] x the text Dropout (S_TEXT, lwidth_t = T*E, lcol0_t = col*E) x the LSTM input mask (S_LSTM_IN + col,
 *    lwidth = D + E, lcol0 = D); xz = text . W_lstm[D:] (no bias), the projection code of tnt_scheduled_feedback_f32.
 * Everything else in the step is the teacher-forced step applied to the fed ids (attention, LSTM-output and output Dropouts,
 * metric, loss, backward, the Embedding gradient scattered to the fed ids).  At p = 0 it is the teacher-forced step (to
 * float32 rounding: the forward runs per step); at p = 1 it is not call_naive_attention, whose Dropouts differ.
 * rate_t = 0 gives the bits of tnt_scheduled_feedback_f32.  No scratch memory.
 * TNT_BADARG for the conditions of tnt_scheduled_feedback_f32, rate_t outside [0, 1), and (rate_t > 0) lwidth_t or
 * lcol0_t not a multiple of 4, lcol0_t < 0 or lcol0_t + E > lwidth_t. */
int32_t tnt_scheduled_feedback2_f32(const float* logits, int32_t ld, int32_t V, const float* table, int32_t E,
                                    const float* w, int32_t ldw, int32_t N, int32_t* fed, int32_t T, int32_t col,
                                    float* text, int32_t ldt, float* xz, int32_t ldz, int32_t B, float rate,
                                    uint64_t seed, uint32_t site, uint32_t step, const uint32_t* step_dev,
                                    int32_t lwidth, int32_t lcol0, int32_t kind, int32_t mode, const double* sched,
                                    const int64_t* counter, uint32_t coin_site, uint32_t draw_site, float rate_t,
                                    uint32_t site_t, int32_t lwidth_t, int32_t lcol0_t, void* stream);
/* Self-critical sequence training loss (Rennie et al. 2017) of the dense caption model's SCST step
 * (nic.NIC(self_critical=...)); restated by tests/scst_oracle.py.  R sampled captions of T tokens; logits [T*R][ld], V valid
 * columns, row (t-1)*R + r holding LSTM step t's logits of caption r (t = 1..T).  For that row:
 *  - sampled token: w = fed[r*T + t] for t < T, last[r] for t = T;
 *  - mask: m = 1 iff no terminator (end_id or 0) occurs among fed[r*T + 1 .. r*T + t-1]: the tokens up to and including
 *    the first terminator count (end_id < 0: only 0 terminates);
 *  - lp = x_w - logsumexp(x) (no clip); loss_row[row] = -adv[r] * m * lp, lp_row[row] = m * lp (both nullable; a row
 *    with m = 0 or adv[r] = 0 has loss_row 0);
 *  - dlogits[row][j] = gscale * adv[r] * m * (softmax(x)_j - [j == w]) for j < V (dlogits may alias logits); a row with
 *    m = 0 or adv[r] = 0 is written as zeros, and a row with m = 0 does not read its logits.  Columns [V, ld) are not
 *    written.
 * The step's loss is gscale * sum of loss_row with gscale = 1/R.  The ids are device data: a counted row (m = 1) whose w is
 * outside [0, V) writes NaN to loss_row and lp_row and a zero gradient row.  One 256-thread workgroup per row, float32,
 * deterministic, no scratch memory.
 * TNT_BADARG for null logits / fed / last / adv / dlogits, V < 1, ld < V, T < 1, R < 1, end_id >= V. */
int32_t tnt_scst_cce_f32(const float* logits, int32_t ld, int32_t V, const int32_t* fed, int32_t T, const int32_t* last,
                         const float* adv, int32_t end_id, float* loss_row, float* lp_row, float* dlogits, int32_t R,
                         float gscale, void* stream);
/* Caption log-likelihood scoring (nic.NIC.score_captions, lc_nic.NIC.score_captions; library-defined, restated by
 * tests/score_oracle.py): log p(caption | scan) of R captions from the logits of the teacher-forced inference forward,
 * read-only.  cap [R][T] holds a caption's ids w_0 .. w_{T-1} (w_0 the start token); logits [steps*R][ld], V valid columns,
 * row (j-1)*R + r = the logits x_j that the step fed with w_{j-1} yields for position j of caption r, j = 1 .. steps
 * (steps in 1 .. T-1).
 *  - lp_j = x_j[w_j] - logsumexp(x_j): no clip at 1e-7, no renormalisation (a log-likelihood, not Keras'
 *    CategoricalCrossentropy);
 *  - position j is counted iff none of w_1 .. w_{j-1} is end_id or 0, and w_j != 0: the terminator itself counts, padding
 *    never does; end_id = -1: up to the first 0;
 *  - tok_lp[(j-1)*R + r] (nullable) = lp_j at counted positions, 0 elsewhere; cap_len[r] (nullable) = the number of
 *    counted positions; cap_lp[r] = the sum of lp_j over the counted positions, added in ascending j in float32 (0 for a
 *    caption without counted positions).
 * The ids are device data: a counted id outside [0, V) gives NaN for that position and that caption, and no read.  The
 * logits of a row that is not counted, and the pad columns [V, ld), are never read; nothing is written to the logits.
 * With tok_lp: one 256-thread workgroup per logits row, then one thread per caption adds that caption's tok_lp entries;
 * without: one workgroup per caption walks its rows.  Same bits either way and run to run (no atomics), no scratch memory.
 * TNT_BADARG for null logits / cap / cap_lp, V < 1, ld < V, T < 2, R < 1, end_id >= V, steps outside 1 .. T-1. */
int32_t tnt_caption_score_f32(const float* logits, int32_t ld, int32_t V, const int32_t* cap, int32_t T, int32_t steps,
                              int32_t R, int32_t end_id, float* tok_lp, float* cap_lp, int32_t* cap_len, void* stream);
/* out[0] = scale * sum_i x[i]  (fixed-order, one workgroup). */
/* Categorical sampling per row (tf.random.categorical(logits / temperature, 1): ThinkAndTell/evaluate.py:223,278;
 * lc_NIC.sample_choice lc_NIC.py:571-575 samples from log(probs)).  x: logits (from_logits=1) or probabilities.
 * out[row] = first j with  w_0+..+w_j > u*sum(w),  w_j = exp((l_j - max l)/temperature),  u = the Philox
 * uniform of element `row` in stream (seed, site, step + *step_dev).  Deterministic; restated by the oracle. */
int32_t tnt_sample_rows_f32(const float* x, int32_t* out, int32_t rows, int32_t V, int32_t ld,
                            float temperature, int32_t from_logits, uint64_t seed, uint32_t site,
                            uint32_t step, const uint32_t* step_dev, void* stream);
/* Top-k / nucleus (top-p) categorical sampling per row (lc_NIC.select_nucleus2 lc_NIC.py:694-710, img_NIC
 * select_topk / select_nucleus img_NIC.py:510-539, defined in rank order; restated in float64 by
 * tests/topkp_oracle.py).  Definition, per row:
 *  - l_j = x_j (from_logits) or log(x_j) (probabilities; log 0 = -inf).  Let m = max_j l_j and
 *    w_j = exp((l_j - m) / temperature).  These are the weights of tnt_sample_rows_f32.
 *  - Rank order: w descending, ties broken by the lower index.
 *  - Top-k: with K = min(top_k, V) when top_k >= 1, else K = V, the candidates are the first K tokens in rank
 *    order.  S_K is their total weight.
 *  - Nucleus: when top_p < 1, a candidate of rank r is kept iff the weight of the candidates ranked before it is
 *    < top_p * S_K.  This keeps the shortest rank prefix whose mass reaches top_p * S_K, and rank 0 is always kept.
 *    top_p >= 1 switches the filter off; no comparison is made.
 *  - Draw: u is the Philox uniform of element `row` in stream (seed, site, step + *step_dev), exactly as in
 *    tnt_sample_rows_f32.  out[row] is the first index j, in ascending index order, at which the running sum of kept
 *    weights exceeds u * sum(kept).
 *  - The written id is always in [0, V), whatever the input, NaN rows included.
 * Implementation notes: a NaN weight counts as 0; the nucleus masses are summed in 2^-38 fixed point (deterministic;
 * off by < V * 2^-39 <= 3e-8 of S_K); the draw keeps tnt_sample_rows_f32's 256 contiguous chunks and serial prefix
 * over the chunk sums, so top_k = 0, top_p = 1 returns that kernel's ids; if rounding leaves no index past the target,
 * the id is the last kept index of positive weight (0 if there is none).  One workgroup per row, the row's weights
 * in LDS: V <= 16384.  TNT_BADARG for rows <= 0 or V <= 0, temperature <= 0, top_p <= 0, V > 16384. */
int32_t tnt_sample_topkp_f32(const float* x, int32_t* out, int32_t rows, int32_t V, int32_t ld,
                             float temperature, int32_t top_k, float top_p, int32_t from_logits,
                             uint64_t seed, uint32_t site, uint32_t step, const uint32_t* step_dev, void* stream);
/* out[0] = mean_i (c - x[i])^2 (MeanSquaredError against a constant target, lc_NIC.py:813-814) */
int32_t tnt_sqdiff_mean_f32(const float* x, float* out, int64_t n, float c, void* stream);
int32_t tnt_sum_f32(const float* x, float* out, int32_t n, float scale, void* stream);
/* two of them in one launch: out0[0] = scale*sum(x0[0..n)), out1[0] = scale*sum(x1[0..n))  (loss + accuracy) */
int32_t tnt_sum2_f32(const float* x0, float* out0, const float* x1, float* out1, int32_t n, float scale,
                     void* stream);
/* Input staging of one device-resident batch in one launch (the generator tuple of
 * data_generator_guse.py:156-171 -> the static buffers of the captured step): x (B,N) -> x_dst (B,ldx);
 * cap (B,T) int32 -> cap_dst; tgt (B,T) int32 ids (nullable) -> tgt_tmajor (T,B); a0, c0 (B,U) -> h0, c0_dst.
 * xT_dst (nullable): additionally the voxel-major copy xT[N][ldt] (ldt >= B) the region-wise encoder gathers from. */
int32_t tnt_stage_batch_f32(const float* x, float* x_dst, const int32_t* cap, int32_t* cap_dst,
                            const int32_t* tgt, int32_t* tgt_tmajor, const float* a0, float* h0,
                            const float* c0, float* c0_dst, int32_t B, int32_t T, int32_t N, int32_t ldx,
                            int32_t U, float* xT_dst, int32_t ldt, void* stream);
/* tnt_stage_batch_f32 with the row map of the vocabulary head riding in the same launch (one extra workgroup).  The text LSTM
 * carries its output through a step that is fed id 0 (mask_zero), so position (t, b), t >= 1, with cap[b][t] == 0 holds
 * the output row of the nearest earlier position of caption b that has a row; where its target equals that row's target
 * as well, its logits, loss and dlogits are repeats.  Such a position is MERGED: pos[t*B + b] = -1.  Every other position
 * gets a row of its own, pos[t*B + b] = 0 .. live-1 in time-major order.  row_weight[r] = 1 + the number of positions merged
 * into row r (float, exact), tgt_compact[r] = the row's target, live[0] = the number of rows.  row_weight, tgt_compact and
 * (nullable) loss_row, corr_row are zeroed in [live, B*T).  tgt is required.  Padded captions (<start>, L words, <end>,
 * 0 ...; tgt[t] = cap[t+1]) have L + 2 rows each. */
int32_t tnt_stage_batch_map_f32(const float* x, float* x_dst, const int32_t* cap, int32_t* cap_dst,
                                const int32_t* tgt, int32_t* tgt_tmajor, const float* a0, float* h0,
                                const float* c0, float* c0_dst, int32_t B, int32_t T, int32_t N, int32_t ldx,
                                int32_t U, float* xT_dst, int32_t ldt, int32_t* pos, float* row_weight,
                                int32_t* tgt_compact, int32_t* live, float* loss_row, float* corr_row, void* stream);
/* tnt_stage_batch_f32 with tnt_dropout_mask4_u8's job riding in the same launch: keep_out [keep_sites][keep_n / 4] bytes, the
 * keep masks of sites keep_site0 .. of stream (keep_seed, *keep_step_dev) -- the attention-dropout masks of the training
 * step this batch feeds (attention.py:36).  The Philox-bound mask blocks and the memory-bound copies share the chip; the
 * captured step then starts without its own mask launch. */
int32_t tnt_stage_batch_masks_f32(const float* x, float* x_dst, const int32_t* cap, int32_t* cap_dst,
                            const int32_t* tgt, int32_t* tgt_tmajor, const float* a0, float* h0,
                            const float* c0, float* c0_dst, int32_t B, int32_t T, int32_t N, int32_t ldx,
                            int32_t U, float* xT_dst, int32_t ldt, uint8_t* keep_out, int64_t keep_n,
                                  int32_t keep_sites, float keep_rate, uint64_t keep_seed, uint32_t keep_site0,
                                  const uint32_t* keep_step_dev, void* stream);
/* Same staging for betas that crossed PCIe as IEEE half (x_half: (B,N) uint16 bit patterns, 8-byte aligned when
 * N % 4 == 0): widened to float in the same pass.  Opt-in "fp16 on-wire" input of data.PinnedPrefetcher
 * (at full-cortex width, N = 327 684, the 84 MB float batch is what bounds the step). */
int32_t tnt_stage_batch_h16(const uint16_t* x_half, float* x_dst, const int32_t* cap, int32_t* cap_dst,
                            const int32_t* tgt, int32_t* tgt_tmajor, const float* a0, float* h0,
                            const float* c0, float* c0_dst, int32_t B, int32_t T, int32_t N, int32_t ldx,
                            int32_t U, float* xT_dst, int32_t ldt, void* stream);
/* Training-time corruption of a staged batch, in place and in one launch of its own behind whichever staging entry ran:
 * scan dropout (the condition dropout of classifier-free guidance) and word dropout (Bowman et al. 2016).
 * step = *step_dev, read on the device when the launch runs.  u(e, site) is the 24-bit uniform of logical element e of the
 * Philox stream (seed, site, step) -- csrc/tnt_rng.h, oracle.philox.uniform24 --, and an element FIRES when u < rate, the
 * negation of the Dropout kernels' keep decision.
 *   scan part (scan_rate > 0): row b fires on element e = b of site_scan.  A fired row gets
 *     x[b * ldx + c] = null_scan ? null_scan[c] : 0.0f for c < N, and, when xT is given (the voxel-major copy [N][ldt]),
 *     xT[c * ldt + b] the same value.  Nothing else is written: not the rows that did not fire, not the columns [N, ldx)
 *     of x, not the columns >= B of xT.
 *   word part (word_rate > 0): position (b, t) with 1 <= t < T and cap[b * T + t] != 0 fires on element e = b * T + t of
 *     site_word; a fired position gets cap[b * T + t] = unk_id.  Column 0 (the start token) and id 0 (padding, the mask
 *     id) are never changed; nothing else is written.
 * rate == 1 fires wherever it may; rate == 0 switches the part off, and its pointers (x, xT, null_scan / cap) may then be
 * null.  Both rates 0: success without a launch.  TNT_BADARG, with nothing launched: a rate outside [0, 1] or NaN;
 * word_rate > 0 with unk_id outside [1, V); B, T or N < 0; ldx < N; xT with ldt < B; a null step_dev; a null x or cap
 * for a part that is switched on.
 * A row is cut into pieces of 1024 columns, one workgroup each; a workgroup makes one Philox call for its row (none per
 * element) and returns at once when the row did not fire: the traffic is that of the fired rows.  float4 stores where N % 4 == ldx % 4 == 0 and x and null_scan are 16-byte aligned, scalar stores
 * otherwise (no refusal).  Deterministic: every address is stored by one thread; no atomics, LDS or scratch. */
int32_t tnt_input_corrupt_f32(float* x, int32_t ldx, float* xT, int32_t ldt, int32_t* cap, int32_t B, int32_t T,
                              int32_t N, int32_t V, float scan_rate, const float* null_scan, float word_rate,
                              int32_t unk_id, uint64_t seed, uint32_t site_scan, uint32_t site_word,
                              const uint32_t* step_dev, void* stream);

/* ---- optimizer: per-variable clipnorm + Adam / SGD over a flat parameter arena --
 * (main.py:97,100-102; lc_NIC.py:389).  The arena is cut by the host into
 * spans of one variable ("segment") each: span_seg[k], span_off[k] (arena offset in
 * floats, multiple of 4), span_len[k]; seg_first[s..s+1] = spans of segment s;
 * seg_l2[s] = L2 lambda (the gradient gets + 2*lambda*theta, lc_NIC.py:47-50).
 * sqnorm: sq[s] = sum (g + 2 lambda theta)^2, wsq[s] = sum theta^2 (L2 metric);
 * partial: 2*nspan floats; l2_out (nullable) = sum_s lambda_s*wsq[s] (the 'L2' metric,
 * tf.add_n(self.losses), lc_NIC.py:379).  If sq_override[s] >= 0 it replaces sq[s] for clipping
 * (Embedding IndexedSlices norm).  clipnorm <= 0 disables clipping.
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t) is read from lr_t_dev when non-null. */
int32_t tnt_seg_sqnorm_f32(const float* theta, const float* grad, const int32_t* span_seg,
                           const int64_t* span_off, const int32_t* span_len,
                           const int32_t* seg_first, const float* seg_l2, float* partial,
                           float* sq, float* wsq, float* l2_out, int32_t nspan, int32_t nseg,
                           void* stream);
/* The scalar tail of a training step in ONE launch (each piece used to be its own dependent launch):
 * span partials (tnt_span_sqnorm_f32: the first kernel of tnt_seg_sqnorm_f32 alone) -> sq / wsq per variable;
 * l2_out = sum_s seg_l2[s]*wsq[s]; out0 = scale*sum x0[0..n), out1 = scale*sum x1[0..n) (loss / accuracy totals,
 * lc_NIC.py:370-376; x1 nullable); extra[0] = sum extra_part[0..n_extra) (the Embedding's IndexedSlices squared norm
 * from the per-block partials of the scatter); ids_dst[0..n_ids) = ids_src (this step's token ids become the
 * prev_ids of tnt_embedding_bwd_sparse_f32); out2 = scale2*sum x2[0..n2) (one more scaled total: the per-timestep partials
 * of tnt_attention_metric_f32 called with out = NULL); then the step state of tnt_step_tick advances (same arguments,
 * same guard rule).  Every piece is optional: nseg = 0, n = 0, n_extra = 0, n2 = 0, null state pointers.  Fixed summation
 * order. */
int32_t tnt_span_sqnorm_f32(const float* theta, const float* grad, const int32_t* span_seg,
                            const int64_t* span_off, const int32_t* span_len, const float* seg_l2,
                            float* partial, int32_t nspan, void* stream);
int32_t tnt_step_finalize_f32(const float* partial, const int32_t* seg_first, const float* seg_l2, float* sq,
                              float* wsq, float* l2_out, int32_t nseg, const float* x0, float* out0,
                              const float* x1, float* out1, int32_t n, float scale, const float* extra_part,
                              float* extra, int32_t n_extra, const int32_t* ids_src, int32_t* ids_dst,
                              int32_t n_ids, const float* x2, float* out2, int32_t n2, float scale2,
                              int64_t* adam_t, uint32_t* drop_step, const float* lr,
                              float* lr_t, float beta1, float beta2, const uint32_t* guard, void* stream);
/* out[0] = sum_s seg_l2[s]*wsq[s]; for callers that run tnt_seg_sqnorm_f32 on slices of the span
 * table (offset pointers, slice-local seg_first; the pipelined data-parallel update) and need the
 * total afterwards. */
int32_t tnt_l2_total_f32(const float* wsq, const float* seg_l2, int32_t nseg, float* out, void* stream);
int32_t tnt_adam_f32(float* theta, float* m, float* v, const float* grad,
                     const int32_t* span_seg, const int64_t* span_off, const int32_t* span_len,
                     const float* seg_l2, const float* sq, const float* sq_override,
                     int32_t nspan, float lr_t, const float* lr_t_dev, float beta1, float beta2,
                     float eps, float clipnorm, const uint32_t* guard, void* stream);
/* tnt_adam_f32 that also files the step's metrics vector in a ring (one wave of the launch, before the guard check): met
 * [nmet <= 62] is copied to row (*ring_t % ring_rows) of ring [ring_rows][nmet + 1], column nmet = the launch number *ring_t
 * (low 24 bits, as a float), and *ring_t advances -- the host reads that row when it wants the step's metrics instead of
 * copying `met` behind every step (a 5 us launch on a 0.55 ms step).  ring NULL = tnt_adam_f32. */
int32_t tnt_adam_ring_f32(float* theta, float* m, float* v, const float* grad,
                     const int32_t* span_seg, const int64_t* span_off, const int32_t* span_len,
                     const float* seg_l2, const float* sq, const float* sq_override,
                     int32_t nspan, float lr_t, const float* lr_t_dev, float beta1, float beta2,
                     float eps, float clipnorm, const uint32_t* guard, const float* met, int32_t nmet, float* ring,
                          int32_t ring_rows, uint32_t* ring_t, void* stream);
int32_t tnt_sgd_f32(float* theta, float* mom, const float* grad, const int32_t* span_seg,
                    const int64_t* span_off, const int32_t* span_len, const float* seg_l2,
                    const float* sq, const float* sq_override, int32_t nspan, float lr,
                    const float* lr_dev, float momentum, float clipnorm, const uint32_t* guard, void* stream);
/* ---- decoupled weight decay (tf.keras.optimizers.AdamW and the `weight_decay=` argument of every keras >= 2.11
 * optimizer; the rule of torch.optim.AdamW) inside the update launches.  For a variable s with decay wd_s >= 0 and the
 * current learning rate lr (the float32 at `lr`, written by tnt_lr_schedule_f32 or by the host) one update does
 *     g  = (grad + 2 lambda_s theta) * clip_scale            unchanged: the coupled L2 stays, and stays in the clip norm
 *     m, v as in tnt_adam_f32
 *     theta' = (theta - (lr * wd_s) * theta) - lr_t * m / (sqrt(v) + eps)      Adam; lr_t as in tnt_adam_f32
 *     theta' = (theta - (lr * wd_s) * theta) + (mu * mom - lr * g)             SGD with momentum mu
 * lr * wd_s is one float32 product formed per workgroup; the decay uses the theta the gradient was taken at (what the
 * kernel has loaded) and enters neither the clip norm, nor m / v, nor the L2 metric; wd_s == 0 leaves the variable's update
 * bit for bit what the plain entry computes; a tripped guard word leaves everything untouched; `lr` is read on the device
 * when the launch runs, so a replayed launch plan or hipGraph decays with the live, scheduled rate.  Each entry is its
 * plain counterpart's kernel with the decay switched on at compile time, and takes the counterpart's arguments plus
 *     tnt_adamw_ring_f32          lr, seg_wd [one float per variable, indexed like seg_l2]     (ring NULL: no metrics ring)
 *     tnt_adamw_fin_f32           seg_wd; lr is fin->lr, which the descriptor already carries
 *     tnt_sgdw_f32                seg_wd; `lr` is tnt_sgd_f32's lr_dev and must be given (there is no host-side lr)
 *     tnt_dense_dw_adamw_f32, tnt_dense_dw_adamw_fin_f32      lr, wd: the one variable's decay, a finite float >= 0
 * TNT_BADARG, and no launch, for a null lr or seg_wd and for a negative or non-finite wd. */
int32_t tnt_adamw_ring_f32(float* theta, float* m, float* v, const float* grad,
                           const int32_t* span_seg, const int64_t* span_off, const int32_t* span_len,
                           const float* seg_l2, const float* sq, const float* sq_override,
                           int32_t nspan, float lr_t, const float* lr_t_dev, float beta1, float beta2,
                           float eps, float clipnorm, const uint32_t* guard, const float* met, int32_t nmet, float* ring,
                           int32_t ring_rows, uint32_t* ring_t, const float* lr, const float* seg_wd, void* stream);
int32_t tnt_adamw_fin_f32(float* theta, float* m, float* v, const float* grad, const int32_t* span_seg,
                          const int64_t* span_off, const int32_t* span_len, const float* sq_override, int32_t nspan, float eps,
                          float clipnorm, const tnt_finalize_desc* fin, const float* met, int32_t nmet, float* ring,
                          int32_t ring_rows, uint32_t* ring_t, const float* seg_wd, void* stream);
int32_t tnt_sgdw_f32(float* theta, float* mom, const float* grad, const int32_t* span_seg,
                     const int64_t* span_off, const int32_t* span_len, const float* seg_l2,
                     const float* sq, const float* sq_override, int32_t nspan, const float* lr, float momentum,
                     float clipnorm, const uint32_t* guard, const float* seg_wd, void* stream);
int32_t tnt_dense_dw_adamw_f32(const float* x, const float* dpre, float* theta, float* m, float* v, float l2,
                               const float* sq, const float* sq_override, const float* lr_t_dev, float beta1,
                               float beta2, float eps, float clipnorm, const uint32_t* guard, int32_t N, int32_t E,
                               int32_t Bk, int32_t ldx, const float* lr, float wd, void* stream);
int32_t tnt_dense_dw_adamw_fin_f32(const float* x, const float* dpre, float* theta, float* m, float* v, float l2,
                                   const float* partial, int32_t k0, int32_t k1, const float* sq_override,
                                   const float* lr_t_dev, float beta1, float beta2, float eps, float clipnorm,
                                   const uint32_t* guard, int32_t N, int32_t E, int32_t Bk, int32_t ldx, const float* lr,
                                   float wd, void* stream);
/* ---- global-norm gradient clipping (tf.clip_by_global_norm; keras `global_clipnorm=`) inside the update launches.
 * Per variable s, q_s is the squared clip-norm input that the per-variable clip of the same route uses:
 *     fin form   (partial != NULL, in front of tnt_adam_fin_gclip_f32; the rule of tnt_adam_fin_f32's span workgroups)
 *         s == extra_seg and n_extra > 0:  sum of extra_part[0..n_extra), lanes of a wave striding by 64, then the
 *                                          wave tree -- the Embedding's un-deduplicated IndexedSlices norm, which is
 *                                          also what tf.linalg.global_norm takes
 *         else sq_override[s] >= 0:        sq_override[s]
 *         else                             the sum over the variable's spans of partial[2 k] = sum (g + 2 lambda theta)^2,
 *                                          in the order of tnt_step_finalize_f32 (<= 8 spans serially, more lane-strided)
 *     table form (sq != NULL, behind tnt_step_finalize_f32 or tnt_seg_sqnorm_f32, which filed sq)
 *         sq_override[s] >= 0 ? sq_override[s] : sq[s]
 * G = sum_s q_s in float32, in ONE fixed order for both forms: 256 accumulators A_t = ((q_t + q_{t+256}) + q_{t+512}) + ...,
 * each 64 of them summed by the library's wave tree (offsets 32, 16, 8, 4, 2, 1) into W_0..W_3, and
 * G = (W_0 + W_1) + (W_2 + W_3).  No atomics: two launches on the same inputs write the same bits, and so do the two
 * forms where sq[s] is the span sum.  tnt_global_sqnorm_f32 is one launch of one workgroup that writes gsq[0] = G; it
 * takes no guard word (G is a pure function of the step's gradients) and must run behind the norm launch(es) and in
 * front of the first update launch of the step.
 * With a threshold c > 0 every gradient element of every variable is scaled by
 *     cs = c / fmaxf(sqrtf(G), c)                         G <= c^2 gives cs == 1.0f exactly
 * which is tf.clip_by_global_norm up to rounding.  L2, the Adam / SGD arithmetic, decoupled decay, the guard rule, the
 * metrics ring and the side workgroup's filings are those of the plain entries.  Each *_gclip_f32 entry is its plain
 * counterpart's kernel with the switch on at compile time and takes the counterpart's arguments, in which `clipnorm`
 * is c and sq / sq_override / partial[k0:k1] are not read for clipping, plus `gsq` (read on the device when the launch
 * runs: a replayed plan or hipGraph clips by the live word) and an optional decay:
 *     tnt_adam_gclip_f32               (tnt_adam_ring_f32)   gsq, lr, seg_wd   seg_wd NULL: no decay; with it lr must be given
 *     tnt_adam_fin_gclip_f32           (tnt_adam_fin_f32)    gsq, seg_wd       lr is fin->lr
 *     tnt_sgd_gclip_f32                (tnt_sgd_f32)         gsq, seg_wd       with seg_wd, lr_dev must be given
 *     tnt_dense_dw_adam_gclip_f32, tnt_dense_dw_adam_fin_gclip_f32             gsq, lr, wd   lr NULL: no decay
 * TNT_BADARG, and no launch, for a null gsq and for a threshold that is not a finite number > 0. */
int32_t tnt_global_sqnorm_f32(const float* partial, const int32_t* seg_first, const float* sq, const float* sq_override,
                              const float* extra_part, int32_t n_extra, int32_t extra_seg, int32_t nseg, float* gsq,
                              void* stream);
int32_t tnt_adam_gclip_f32(float* theta, float* m, float* v, const float* grad,
                           const int32_t* span_seg, const int64_t* span_off, const int32_t* span_len,
                           const float* seg_l2, const float* sq, const float* sq_override,
                           int32_t nspan, float lr_t, const float* lr_t_dev, float beta1, float beta2,
                           float eps, float clipnorm, const uint32_t* guard, const float* met, int32_t nmet, float* ring,
                           int32_t ring_rows, uint32_t* ring_t, const float* gsq, const float* lr, const float* seg_wd,
                           void* stream);
int32_t tnt_adam_fin_gclip_f32(float* theta, float* m, float* v, const float* grad, const int32_t* span_seg,
                               const int64_t* span_off, const int32_t* span_len, const float* sq_override, int32_t nspan,
                               float eps, float clipnorm, const tnt_finalize_desc* fin, const float* met, int32_t nmet,
                               float* ring, int32_t ring_rows, uint32_t* ring_t, const float* gsq, const float* seg_wd,
                               void* stream);
int32_t tnt_sgd_gclip_f32(float* theta, float* mom, const float* grad, const int32_t* span_seg,
                          const int64_t* span_off, const int32_t* span_len, const float* seg_l2,
                          const float* sq, const float* sq_override, int32_t nspan, float lr, const float* lr_dev,
                          float momentum, float clipnorm, const uint32_t* guard, const float* gsq, const float* seg_wd,
                          void* stream);
int32_t tnt_dense_dw_adam_gclip_f32(const float* x, const float* dpre, float* theta, float* m, float* v, float l2,
                                    const float* sq, const float* sq_override, const float* lr_t_dev, float beta1,
                                    float beta2, float eps, float clipnorm, const uint32_t* guard, int32_t N, int32_t E,
                                    int32_t Bk, int32_t ldx, const float* gsq, const float* lr, float wd, void* stream);
int32_t tnt_dense_dw_adam_fin_gclip_f32(const float* x, const float* dpre, float* theta, float* m, float* v, float l2,
                                        const float* partial, int32_t k0, int32_t k1, const float* sq_override,
                                        const float* lr_t_dev, float beta1, float beta2, float eps, float clipnorm,
                                        const uint32_t* guard, int32_t N, int32_t E, int32_t Bk, int32_t ldx,
                                        const float* gsq, const float* lr, float wd, void* stream);
/* ---- per-variable learning-rate multipliers and frozen variables (fine-tuning: keras `layer.trainable = False`, and
 * discriminative learning rates) inside the update launches.  seg_lrm holds one float per variable, indexed like seg_l2:
 * mul_s >= 0, finite.  With the current rates lr and lr_t of the plain entries one update of variable s does
 *     g, the clip scale, m, v as in the plain entry                (mul_s enters neither a norm nor the moments)
 *     theta' = (theta - ((mul_s * lr) * wd_s) * theta) - (mul_s * lr_t) * m / (sqrt(v) + eps)           Adam
 *     theta' = (theta - ((mul_s * lr) * wd_s) * theta) + (mu * mom - (mul_s * lr) * g)                  SGD
 * mul_s * lr and mul_s * lr_t are float32 products formed once per workgroup, so mul_s == 1 leaves the update bit for bit
 * what the entry without the table computes.  mul_s == 0 is a FROZEN variable: the workgroups of its spans issue no load
 * and no store of theta, m, v (mom) or grad -- the three stay bit-unchanged, and grad may hold anything, non-finite values
 * included.  The branch is uniform per workgroup.  Frozen variables are excluded by selection, never by a product with 0:
 *     tnt_span_sqnorm_lrmul_f32 / tnt_seg_sqnorm_lrmul_f32   (tnt_span_sqnorm_lr_f32 / tnt_span_sqnorm_f32, tnt_seg_sqnorm_f32)
 *         do not read a frozen variable's gradient: its slot partial[2 k] (and sq[s]) is 0; sum theta^2 and with it the L2
 *         metric are formed as for any variable.  adam_t / lr / lr_t all NULL: no lr job (tnt_span_sqnorm_f32's launch)
 *     tnt_global_sqnorm_lrmul_f32   (tnt_global_sqnorm_f32)
 *         G is the sum over the variables with mul_s != 0 in the same fixed order (a frozen variable's term is the + 0 of a
 *         slot behind the last variable; nothing of it is loaded).  A multiplier other than 0 does not change G
 *     tnt_adam_fin_lrmul_f32   (tnt_adam_fin_f32)      seg_lrm, gsq, seg_wd       a frozen span's workgroup still arrives: the
 *         finalize work, the counters' tick and the metrics ring are those of the plain entry, once per launch
 *     tnt_adam_lrmul_f32       (tnt_adam_ring_f32)     seg_lrm, gsq, lr, seg_wd
 *     tnt_sgd_lrmul_f32        (tnt_sgd_f32)           seg_lrm, gsq, seg_wd       with seg_wd, lr_dev must be given
 *     tnt_dense_dw_adam_lrmul_f32, tnt_dense_dw_adam_fin_lrmul_f32   (tnt_dense_dw_adam_f32 / _fin_f32)   lrm, gsq, lr, wd
 *         the encoder's fused update takes its one variable's multiplier as the scalar lrm, as it takes wd; lr NULL: no
 *         decay.  A negative or non-finite lrm is TNT_BADARG; lrm == 0 checks the arguments and launches nothing
 * gsq (nullable) switches global-norm clipping on as in the *_gclip_f32 entries, seg_wd (nullable) the decoupled decay as
 * in the adamw / sgdw entries.  adam_t and the bias correction stay global: a variable unfrozen later resumes with its
 * old moments at the global step count.  The table is read on the device when the launch runs, so a replayed launch plan
 * or hipGraph follows an in-place rewrite.  The guard rule is the plain entries'.  TNT_BADARG, and no launch, for a null
 * seg_lrm; the entries do not read the table on the host: a negative or non-finite entry is the caller's to refuse. */
int32_t tnt_span_sqnorm_lrmul_f32(const float* theta, const float* grad, const int32_t* span_seg, const int64_t* span_off,
                                  const int32_t* span_len, const float* seg_l2, float* partial, int32_t nspan,
                                  const int64_t* adam_t, const float* lr, float* lr_t, float beta1, float beta2,
                                  const float* sq_override, const float* seg_lrm, void* stream);
int32_t tnt_seg_sqnorm_lrmul_f32(const float* theta, const float* grad, const int32_t* span_seg, const int64_t* span_off,
                                 const int32_t* span_len, const int32_t* seg_first, const float* seg_l2, float* partial,
                                 float* sq, float* wsq, float* l2_out, int32_t nspan, int32_t nseg, const float* seg_lrm,
                                 void* stream);
int32_t tnt_global_sqnorm_lrmul_f32(const float* partial, const int32_t* seg_first, const float* sq, const float* sq_override,
                                    const float* extra_part, int32_t n_extra, int32_t extra_seg, int32_t nseg, float* gsq,
                                    const float* seg_lrm, void* stream);
int32_t tnt_adam_lrmul_f32(float* theta, float* m, float* v, const float* grad,
                           const int32_t* span_seg, const int64_t* span_off, const int32_t* span_len,
                           const float* seg_l2, const float* sq, const float* sq_override,
                           int32_t nspan, float lr_t, const float* lr_t_dev, float beta1, float beta2,
                           float eps, float clipnorm, const uint32_t* guard, const float* met, int32_t nmet, float* ring,
                           int32_t ring_rows, uint32_t* ring_t, const float* seg_lrm, const float* gsq, const float* lr,
                           const float* seg_wd, void* stream);
int32_t tnt_adam_fin_lrmul_f32(float* theta, float* m, float* v, const float* grad, const int32_t* span_seg,
                               const int64_t* span_off, const int32_t* span_len, const float* sq_override, int32_t nspan,
                               float eps, float clipnorm, const tnt_finalize_desc* fin, const float* met, int32_t nmet,
                               float* ring, int32_t ring_rows, uint32_t* ring_t, const float* seg_lrm, const float* gsq,
                               const float* seg_wd, void* stream);
int32_t tnt_sgd_lrmul_f32(float* theta, float* mom, const float* grad, const int32_t* span_seg,
                          const int64_t* span_off, const int32_t* span_len, const float* seg_l2,
                          const float* sq, const float* sq_override, int32_t nspan, float lr, const float* lr_dev,
                          float momentum, float clipnorm, const uint32_t* guard, const float* seg_lrm, const float* gsq,
                          const float* seg_wd, void* stream);
int32_t tnt_dense_dw_adam_lrmul_f32(const float* x, const float* dpre, float* theta, float* m, float* v, float l2,
                                    const float* sq, const float* sq_override, const float* lr_t_dev, float beta1,
                                    float beta2, float eps, float clipnorm, const uint32_t* guard, int32_t N, int32_t E,
                                    int32_t Bk, int32_t ldx, float lrm, const float* gsq, const float* lr, float wd,
                                    void* stream);
int32_t tnt_dense_dw_adam_fin_lrmul_f32(const float* x, const float* dpre, float* theta, float* m, float* v, float l2,
                                        const float* partial, int32_t k0, int32_t k1, const float* sq_override,
                                        const float* lr_t_dev, float beta1, float beta2, float eps, float clipnorm,
                                        const uint32_t* guard, int32_t N, int32_t E, int32_t Bk, int32_t ldx, float lrm,
                                        const float* gsq, const float* lr, float wd, void* stream);
/* ---- adaptive gradient clipping, unit-wise (AttemptFour/Model/agc.py:20-38; call site lc_NIC.py:388) ----
 * Applied in place to the flat gradient arena before the norms / clip-by-norm / Adam: per variable v (table entry:
 * arena offset var_off, row stride var_ld, L2 lambda var_lam) and per unit = output column of a keras (in, out) kernel
 * (vectors: one unit):  g <- g * max(||theta_u||, eps) * clip_factor / max(||g_u||, 1e-6)  where ||g_u|| is not below
 * that bound; g = arena gradient + 2 lambda theta (what tape.gradient returns), written back minus the L2 term.
 * item [nitem][6] = (var, c0, ncols <= 64, r0, r1, column block id), cb_first [ncb+1] = first item of each column
 * block (items of a block are consecutive); partial: nitem*128 floats.  Embedding (IndexedSlices, agc.py:25-30):
 * gsq_cols[E] = column sums of squares of the un-deduplicated row gradients (tnt_colsq_f32) replaces the dense
 * gradient's for variable gsq_var, whose column blocks are gsq_cb0 .. gsq_cb0+gsq_ncb-1; sq_out[0] receives the squared
 * norm of the clipped rows (for clip-by-norm's IndexedSlices norm), sq_part: gsq_ncb floats of scratch. */
int32_t tnt_agc_f32(const float* theta, float* grad, const int64_t* var_off, const int32_t* var_ld,
                    const float* var_lam, const int32_t* item, const int32_t* cb_first, int32_t nitem,
                    float* partial, const float* gsq_cols, int32_t gsq_var, int32_t gsq_cb0, int32_t gsq_ncb,
                    float* sq_part, float* sq_out, float clip_factor, float eps, void* stream);
/* out[c] = sum_r x[r][c]^2 */
int32_t tnt_colsq_f32(const float* x, float* out, int32_t rows, int32_t cols, int32_t ld, void* stream);
/* Sharpness-aware minimisation helper (CaptionGenerator.train_step_SAM, ThinkAndTell/model.py:166-233;
 * lc_NIC.train_step_sam, lc_NIC.py:713-838).  mode 0: e_w = (g + 2 lambda theta) * rho/(||g||+1e-12)
 * with ||g||^2 = sum_s sq[s] (from tnt_seg_sqnorm_f32; sq_override[s] >= 0 replaces sq[s]: tf.linalg.global_norm takes an
 * IndexedSlices gradient by its un-deduplicated values, nullable); theta += e_w; e_w stored.  mode 1: theta -= e_w, and
 * grad += 2 lambda e_w: the gradient the tape took at theta + e_w carries the L2 term of the PERTURBED weights, while the
 * optimizer kernels add 2 lambda theta at the restored ones. */
int32_t tnt_sam_f32(float* theta, float* grad, float* ew, const int32_t* span_seg,
                    const int64_t* span_off, const int32_t* span_len, const float* seg_l2,
                    const float* sq, const float* sq_override, int32_t nseg, int32_t nspan, float rho, int32_t mode, void* stream);
/* device-resident step state, advanced inside the (captured) step:
 * adam_t += 1; lr_t = lr[0]*sqrt(1-b2^t)/(1-b1^t); drop_step += 1.  Pointers nullable.
 * guard (nullable): a device error word (tnt_lstm_seq_fwd_f32); when it is non-zero nothing is advanced, and
 * tnt_adam_f32 / tnt_sgd_f32 given the same word skip their update: a step whose forward pass was invalid leaves
 * weights, moments, t and the dropout stream exactly as they were, so the caller can redo it. */
int32_t tnt_step_tick(int64_t* adam_t, uint32_t* drop_step, const float* lr, float* lr_t,
                      float beta1, float beta2, const uint32_t* guard, void* stream);
/* Weight averaging over the parameter arena (average.hip), one launch behind the optimizer update: an exponential moving
 * average (kind 0; tfa.optimizers.MovingAverage) or an equal-weight running mean (kind 1; tfa.optimizers.SWA) of theta in
 * avg; restated by tests/average_oracle.py.  This library's definition.  Every decision is taken on the device when the
 * launch runs, from *step (int64: the updates applied so far, the model's adam_t after its tick) and *guard, so a
 * recorded plan or a hipGraph replays with the live values; the scalars are uniform over the launch:
 *  - guard (nullable) non-zero: nothing is read or written.
 *  - t = *step, s = max(start_step, 1).  t <= s: the launch copies, avg[i] = theta[i].  The average is seeded by the
 *    parameters after update s and never depends on what avg held before.
 *  - otherwise r = t - s; r % every != 0: nothing happens; else k = r / every (>= 1) samples follow the seed and
 *      kind 0: d = momentum; with dynamic != 0, d = min(momentum, (1 + k) / (10 + k))   (tfa's dynamic_decay)
 *      kind 1: d = k / (k + 1)                                   (the mean of the seed and the k later samples)
 *    in float64; c = (float)(1.0 - d); avg[i] = fmaf(c, theta[i] - avg[i], avg[i]) in float32: two roundings per element.
 * theta is never written.  momentum is a HOST pointer to one float64, read during the call (the scalars this ABI passes
 * by value are 32/64-bit integers and float; a float64 travels by address, as tnt_scheduled_feedback_f32's sched does --
 * here from host memory, so that the entry can check it).  TNT_BADARG, and no launch, for n < 0, null theta / avg / step
 * / momentum, theta or avg not 16-byte aligned, theta and avg overlapping, kind other than 0 / 1, momentum outside
 * [0, 1) or NaN, start_step < 0, every < 1.  n == 0 is a no-op.  Float4 main path over a grid-stride range, n % 4 tail;
 * avg moves non-temporally under the TNT_STREAM_NT policy of the optimizer kernels; no atomics, LDS or scratch; every
 * address is written by one thread. */
int32_t tnt_weight_average_f32(const float* theta, float* avg, int64_t n, const int64_t* step, int32_t kind,
                               const double* momentum, int32_t dynamic, int64_t start_step, int32_t every,
                               const uint32_t* guard, void* stream);
/* a <-> b over n floats, every element moved by one thread (ModelBase.swap_weights: captured graphs and plans hold the
 * buffers' addresses, so the contents move).  TNT_BADARG, and no launch, for n < 0, a null or not 16-byte aligned
 * pointer, overlapping buffers.  n == 0 is a no-op. */
int32_t tnt_swap_f32(float* a, float* b, int64_t n, void* stream);
/* Gradient accumulation over the flat gradient arena (accumulate.hip): the device-side sum over the k micro-steps of an
 * accumulation window (gradient_accumulation_steps=k), in the place data parallel's all-reduce over ranks has; restated by
 * tests/accum_oracle.py.  This library's definition.  acc: the accumulator, n floats; grad: the gradient arena the
 * micro-step's backward has just written; sq_acc / sq_slot: one float each, the accumulated and the micro-step's
 * un-deduplicated Embedding squared norm (the model's sq_override slot); drop_step: the dropout stream's step counter.
 * The launch is the last one of a micro-step (phases 0, 1) or sits between the backward and the norm launch (phase 2):
 *   phase 0 OPEN   acc[i] = grad[i] (acc is not read);   sq_acc[0] = sq_slot[0];              drop_step[0] += 1
 *   phase 1 ADD    acc[i] = acc[i] + grad[i];            sq_acc[0] = sq_acc[0] + sq_slot[0];  drop_step[0] += 1
 *   phase 2 CLOSE  grad[i] = acc[i] + grad[i] (acc is not written);  sq_slot[0] = sq_acc[0] + sq_slot[0];  drop_step is
 *                  left alone: the tick of the update behind it advances it
 * for i in [0, n); the scalars are the work of one thread.  Plain float32 adds in exactly that operand order, every address
 * written by one thread, no atomic and no cross-thread reduction: the result is bit-identical to numpy float32 doing the
 * same adds, and a replay is bit-reproducible.  In OPEN / ADD grad is never written.
 *  - guard (nullable) non-zero: nothing is read, written or advanced (the rule of tnt_step_tick and the update kernels: a
 *    micro-step whose forward pass was invalid leaves the window as it was).
 *  - sq_acc / sq_slot are null together (no scalar sum); drop_step is nullable.  With n == 0 the scalar work still happens.
 * TNT_BADARG, and no launch, for n < 0, null acc / grad, acc or grad not 16-byte aligned, acc and grad sharing an element,
 * phase outside 0..2, exactly one of sq_acc / sq_slot null, sq_acc == sq_slot.  Float4 main path over a grid-stride range,
 * n % 4 tail; acc moves non-temporally under the TNT_STREAM_NT policy of the optimizer kernels, grad with plain accesses
 * (the backward has just written it, and in CLOSE the norm launch reads it next); no LDS or scratch. */
int32_t tnt_grad_accumulate_f32(float* acc, float* grad, int64_t n, int32_t phase, float* sq_acc, float* sq_slot,
                                uint32_t* drop_step, const uint32_t* guard, void* stream);
/* Learning-rate schedule evaluated on the device (schedule.hip): lr[0] = (float) schedule(*step), one thread, in front of
 * the first launch of a training step that reads lr; restated by tests/lr_schedule_oracle.py.  *step (int64: the updates
 * applied so far, the model's adam_t; the first update sees 0, a negative value counts as 0) and params[0..16) (float64)
 * are read on the device when the launch runs, so a recorded plan or a hipGraph replays with the live counter -- Keras's
 * lr = schedule(optimizer.iterations) with no device-to-host sync.  There is no guard argument: a step whose guard word
 * tripped does not advance adam_t, so the next step computes the same value again.
 * Layout.  params[0] = kind id, params[1] = w, the warm-up steps (0: none), params[2] = the warm-up's start value,
 * params[3..16) = the kind's fields f[0..13); unused fields are 0.  Kind 6 alone has no warm-up fields.
 *   0 constant               f = lr0
 *   1 ExponentialDecay       f = lr0, D, rate, staircase     lr0 * pow(rate, p)
 *   2 InverseTimeDecay       f = lr0, D, rate, staircase     lr0 / (1 + rate * p)
 *                            p = s / D in float64, with staircase != 0 the integer quotient s / D
 *   3 CosineDecay            f = lr0, D, alpha               c = min(s, D) / D;  lr0 * ((1 - alpha) * 0.5 * (1 + cos(pi * c)) + alpha)
 *   4 CosineDecayRestarts    f = lr0, first, t_mul, m_mul, alpha
 *                            P = first, r = s, m = 1; while r >= P: r -= P, P *= t_mul, m *= m_mul   (float64: + * and a
 *                            comparison only, so host and device leave the loop in the same trip); t_mul == 1 takes the
 *                            closed form r = s % first, m = pow(m_mul, s / first) in integers;
 *                            lr0 * ((1 - alpha) * m * 0.5 * (1 + cos(pi * r / P)) + alpha)
 *   5 PolynomialDecay        f = lr0, D, end, power, cycle   cycle != 0: D' = D * max(1, ceil(s / D)) in integers, s' = s;
 *                            else D' = D, s' = min(s, D);  (lr0 - end) * pow(1 - s' / D', power) + end
 *   6 PiecewiseConstantDecay params[1..8) = 7 boundaries, params[8..16) = 8 values: values[i] of the first i with
 *                            s <= boundaries[i], else values[7]; unused boundaries hold +inf, unused values the last value
 *   7 PiecewiseConstantDecay under a warm-up: f[0..6) = 6 boundaries, f[6..13) = 7 values, the same rule
 * Warm-up (w >= 1; kinds 0 - 5 and 7): s < w gives start + (a0 - start) * s / w with a0 = the kind at 0 updates, from w on
 * the kind at s - w updates; continuous at w.  Every expression is evaluated in float64 in the written order, products
 * and sums rounded separately (no fused multiply-add), left to right, and the result is rounded once to float32: the
 * kinds without pow / cos give the bits of the same expression on the host.  D, first, w and the boundaries are
 * integers >= 1 stored as float64; the caller validates the hyper-parameters (masters_thesis_amd.schedules).  An unknown
 * kind, a D or first below 1, a w that is no integer >= 0 and a restart loop that has not ended after 4096 trips (the
 * descriptor admits t_mul = 1 or >= 1.05: under 900) store NaN.  TNT_BADARG, and no launch, for a null step, params or
 * lr.  No atomics, LDS or scratch. */
int32_t tnt_lr_schedule_f32(const int64_t* step, const double* params, float* lr, void* stream);

/* ---- region-wise encoder: layers.LocallyDense.call (layers.py:43-48) ------------
 * CSR groups: idx[goff[r] .. goff[r+1]) are the voxel columns of group r; W is the
 * concatenation of the per-group kernels, [goff[R]][D]; bias [R][D].
 * Any B (processed in row blocks of 64, in order), D % 16 == 0, D <= 64.
 * fwd: pre/y[b][r][:] = LeakyReLU(x[b][idx_r] @ W_r + b_r)    (y,pre: [B][R][D])
 * bwd: dW_r = x[:,idx_r]^T @ dpre[:,r,:]; db_r = sum_b dpre[b][r][:]. */
/* Input gradient of a stack of per-region Dense layers -- the deeper stages of deep_layers.LocallyDense
 * (AttemptFour/Model/deep_layers.py:53-59), whose forward and weight gradients are tnt_locally_dense_*_f32 on the
 * identity groups {r*D .. (r+1)*D-1}:  dx[b][r][k] = sum_n dpre[b][r][n] * W[r][k][n];  dpre [B][R][Dout],
 * W [R][Din][Dout], dx [B][R][Din]; Din, Dout <= 64. */
int32_t tnt_block_dense_dx_f32(const float* dpre, const float* W, float* dx, int32_t B, int32_t R,
                               int32_t Din, int32_t Dout, void* stream);
int32_t tnt_locally_dense_fwd_f32(const float* x, int32_t ldx, const int32_t* idx,
                                  const int32_t* goff, const float* W, const float* bias,
                                  float* pre, float* y, int32_t B, int32_t R, int32_t D,
                                  float slope, void* stream);
int32_t tnt_locally_dense_bwd_f32(const float* x, int32_t ldx, const int32_t* idx,
                                  const int32_t* goff, const float* dpre, float* dW, float* db,
                                  int32_t B, int32_t R, int32_t D, void* stream);

/* ---- additive attention step: attention.Attention.call (attention.py:25-44) -----
 * P = LeakyReLU(F @ W1 + b1) is loop-invariant and computed once with tnt_gemm_f32.
 * fwd: q = LeakyReLU(h @ W2 + b2); s = tanh(P + q); dropout(s); e = s.v + bv;
 *      alpha = softmax_R(e); ctx = sum_R alpha*F; ctx_d = LSTM-input dropout of ctx.
 *      Saves qpre[B][A], alpha[B][R]. s_out (nullable) [B][R][A] post-dropout.
 *      keep4 (nullable, fwd and bwd): this step's [B*R*A/4] bytes of tnt_dropout_mask4_u8 for (seed, site_attn, step);
 *      when given (A % 4 == 0) the kernels read the bits instead of running Philox -- bit-identical results. */
int32_t tnt_attention_step_fwd_f32(const float* h, const float* F, const float* P,
                                   const float* W2, const float* b2, const float* v,
                                   const float* bv, float* qpre, float* alpha, float* ctx,
                                   float* ctx_d, float* s_out, int32_t B, int32_t R, int32_t D,
                                   int32_t A, int32_t U, float slope, float rate_attn,
                                   float rate_in, int32_t in_lwidth, uint64_t seed,
                                   uint32_t site_attn, uint32_t site_in, uint32_t step,
                                   const uint32_t* step_dev, const uint8_t* keep4, void* stream);
/* bwd: given dctx_d (grad wrt the dropped ctx), accumulates dP[B][R][A] += , dF[B][R][D] +=,
 * dvb[B][A+1] += (per-sample partials of dV and dbV), writes dqpre[B][A] and
 * dh[B][U] = dqpre @ W2^T.  If dz != NULL the context gradient is computed in-kernel as
 * dctx_d[b][d] = sum_n dz[b][n] * Wc[d][n] (dz: this step's LSTM dz [B][4U]; Wc: the context
 * rows of the LSTM kernel [D][4U]) and the dctx_d argument is ignored.  If dctx_part is non-null ([nparts][B][D], written
 * by tnt_lstm_step_bwd_f32; nparts*D <= 1024) the context gradient is the sum of the parts and dctx_d / dz are ignored. */
/* alpha_mse_coef: dalpha[b][r] += alpha_mse_coef * (alpha[b][r] - 1) before the softmax backward -- the gradient of
 * c * sum (1 - alpha)^2 with alpha_mse_coef = 2c (lc_NIC.train_step_sam's attention term, lc_NIC.py:751-752); 0 = none.
 * fresh != 0: dP / dF / dvb are overwritten with this step's terms instead of added to (the first executed step of a
 * chain, so the caller needs no zero fill of the three accumulators). */
int32_t tnt_attention_step_bwd_f32(const float* dctx_d, const float* F, const float* P,
                                   const float* W2, const float* v, const float* qpre,
                                   const float* alpha, float* dP, float* dF, float* dvb,
                                   float* dqpre, float* dh, int32_t B, int32_t R, int32_t D,
                                   int32_t A, int32_t U, float slope, float rate_attn,
                                   float rate_in, int32_t in_lwidth, uint64_t seed,
                                   uint32_t site_attn, uint32_t site_in, uint32_t step,
                                   const uint32_t* step_dev, const float* dz, const float* Wc,
                                   const float* dctx_part, int32_t nparts, const uint8_t* keep4,
                                   float alpha_mse_coef, int32_t fresh, void* stream);
/* the same launch with an external gradient of the attention weights as a rider: ext != NULL adds ext[b * ext_bs + r]
 * (ext_bs >= 0, in floats) to dalpha[b][r] next to the alpha_mse term, before the softmax backward.  The caller passes
 * the slab of this step.  ext == NULL is tnt_attention_step_bwd_f32, bit for bit (that entry forwards here). */
int32_t tnt_attention_step_bwd_ext_f32(const float* dctx_d, const float* F, const float* P,
                                       const float* W2, const float* v, const float* qpre,
                                       const float* alpha, float* dP, float* dF, float* dvb,
                                       float* dqpre, float* dh, int32_t B, int32_t R, int32_t D,
                                       int32_t A, int32_t U, float slope, float rate_attn,
                                       float rate_in, int32_t in_lwidth, uint64_t seed,
                                       uint32_t site_attn, uint32_t site_in, uint32_t step,
                                       const uint32_t* step_dev, const float* dz, const float* Wc,
                                       const float* dctx_part, int32_t nparts, const uint8_t* keep4,
                                       float alpha_mse_coef, int32_t fresh, const float* ext, int32_t ext_bs,
                                       void* stream);

/* ---- the forward chain of the attention captioner as ONE persistent launch (lc_NIC.py:244-256): for i < T:
 * tnt_attention_step_fwd_f32(h = hs[i], ..., qpre[i], alpha[i], ctx[i], ctx_d[i], keep4 + i * keep_stride, sites + i) then
 * tnt_lstm_step_fwd_f32(xz[i], hs[i], cs[i], Ur, ctx_d[i], Wc, ... -> hs[i+1], cs[i+1], gates[i]) with xz_bias.
 * hs / cs [T+1][B][U] (slab 0 = initial state), xz [T][B][U][4], qpre [T][B][A], alpha [T][B][R], ctx / ctx_d [T][B][D],
 * gates [T][B][U][4].  U == 512, B <= 128, R <= 512, A % 4 == D % 4 == 0, A, D <= 64, the device census of
 * tnt_lstm_seq_supported.  work: tnt_lc_seq_fwd_work_floats(B) floats of exchange space (contents irrelevant: the partial
 * query sums the LSTM workgroups hand to the attention workgroups).  sync / guard_out: as tnt_lstm_seq_fwd_f32 (same state
 * words). */
int32_t tnt_lc_seq_fwd_work_floats(int32_t B);
int32_t tnt_lc_seq_fwd_f32(const float* F, const float* P, const float* W2, const float* b2, const float* v,
                           const float* bv, float* qpre, float* alpha, float* ctx, float* ctx_d, const uint8_t* keep4,
                           int64_t keep_stride, const float* xz, const float* Wc, const float* Ur, const float* xz_bias,
                           float* hs, float* cs, float* gates, int32_t T, int32_t B, int32_t R, int32_t D, int32_t A,
                           int32_t U, float slope, float rate_attn, float rate_in, int32_t in_lwidth, uint64_t seed,
                           uint32_t site_attn0, uint32_t site_in0, const uint32_t* step_dev, float* work,
                           uint32_t* sync, float* guard_out, void* stream);
/* the same launch with the Dropout behind the LSTM (lc_NIC.py:256) as a rider: hd [T][B][U] (nullable) receives
 * tnt_dropout_f32(hs[1:], rows_per_site = B, site = site_out0 + i for step i) as the states leave the chain. */
int32_t tnt_lc_seq_fwd_drop_f32(const float* F, const float* P, const float* W2, const float* b2, const float* v,
                                const float* bv, float* qpre, float* alpha, float* ctx, float* ctx_d,
                                const uint8_t* keep4, int64_t keep_stride, const float* xz, const float* Wc,
                                const float* Ur, const float* xz_bias, float* hs, float* cs, float* gates, int32_t T,
                                int32_t B, int32_t R, int32_t D, int32_t A, int32_t U, float slope, float rate_attn,
                                float rate_in, int32_t in_lwidth, uint64_t seed, uint32_t site_attn0,
                                uint32_t site_in0, const uint32_t* step_dev, float* hd, float rate_out,
                                uint32_t site_out0, float* work, uint32_t* sync, float* guard_out, void* stream);

/* ---- the backward chain of the attention captioner as ONE persistent launch (tape.gradient through lc_NIC.py:244-256):
 * for i = T-1 .. 0: tnt_lstm_step_bwd_f32(dz_next = dz[i+1], dh_ext = the attention's query gradient of step i+1,
 * dout_t = dout[i], gates[i], cs[i+1], cs[i] -> dz[i], context-gradient parts) then tnt_attention_step_bwd_f32(parts,
 * qpre[i], alpha[i], keep4 + i * keep_stride, sites + i -> dqpre[i], query gradient), with dP [B][R][A], dF [B][R][D] and
 * dvb [B][A+1] accumulated on chip over the T steps and WRITTEN once (no zero fill by the caller).
 * dout [T][B][U], gates / dz [T][B][U][4], cs [T+1][B][U], qpre / dqpre [T][B][A], alpha [T][B][R]; work:
 * tnt_lc_seq_bwd_work_floats(B, U) floats of exchange space (contents irrelevant).  Shape limits, sync and guard_out as
 * tnt_lc_seq_fwd_f32 (a sample's P, F, dP and dF rows live in registers: without spills for R <= 384 with A, D <= 32 and
 * for R <= 192 otherwise). */
int32_t tnt_lc_seq_bwd_work_floats(int32_t B, int32_t U);
int32_t tnt_lc_seq_bwd_f32(const float* F, const float* P, const float* W2, const float* v, const float* qpre,
                           const float* alpha, const uint8_t* keep4, int64_t keep_stride, float* dP, float* dF,
                           float* dvb, float* dqpre, const float* Ur, const float* Wc, const float* dout,
                           const float* gates, const float* cs, float* dz, float* work, int32_t T, int32_t B,
                           int32_t R, int32_t D, int32_t A, int32_t U, float slope, float rate_attn, float rate_in,
                           int32_t in_lwidth, uint64_t seed, uint32_t site_attn0, uint32_t site_in0,
                           const uint32_t* step_dev, float alpha_mse_coef, uint32_t* sync, float* guard_out,
                           void* stream);
/* the same launch with that Dropout's backward as a rider: dout is the gradient w.r.t. the DROPPED outputs and meets the
 * keep mask (rate_out, site_out0 + i for step i; the bits of tnt_lc_seq_fwd_drop_f32) as the chain reads it. */
int32_t tnt_lc_seq_bwd_drop_f32(const float* F, const float* P, const float* W2, const float* v, const float* qpre,
                                const float* alpha, const uint8_t* keep4, int64_t keep_stride, float* dP, float* dF,
                                float* dvb, float* dqpre, const float* Ur, const float* Wc, const float* dout,
                                const float* gates, const float* cs, float* dz, float* work, int32_t T, int32_t B,
                                int32_t R, int32_t D, int32_t A, int32_t U, float slope, float rate_attn,
                                float rate_in, int32_t in_lwidth, uint64_t seed, uint32_t site_attn0,
                                uint32_t site_in0, const uint32_t* step_dev, float alpha_mse_coef, float rate_out,
                                uint32_t site_out0, uint32_t* sync, float* guard_out, void* stream);
/* the _drop launch (rate_out = 0: the plain one) with an external gradient of the attention weights as a rider: step i adds
 * ext[i * ext_ts + b * ext_bs + r] to dalpha[b][r] next to the alpha_mse term (element strides >= 0; the last element read,
 * (T-1) ext_ts + (B-1) ext_bs + R - 1, must lie below 2^29).  tnt_attention_coverage_f32 writes ext with strides (0, R) for
 * axis 0 and (R, 0) for axis 1; a full [T][B][R] gradient has (B R, R).  ext == NULL: the two entries above, bit for bit
 * (they forward here). */
int32_t tnt_lc_seq_bwd_ext_f32(const float* F, const float* P, const float* W2, const float* v, const float* qpre,
                               const float* alpha, const uint8_t* keep4, int64_t keep_stride, float* dP, float* dF,
                               float* dvb, float* dqpre, const float* Ur, const float* Wc, const float* dout,
                               const float* gates, const float* cs, float* dz, float* work, int32_t T, int32_t B,
                               int32_t R, int32_t D, int32_t A, int32_t U, float slope, float rate_attn,
                               float rate_in, int32_t in_lwidth, uint64_t seed, uint32_t site_attn0,
                               uint32_t site_in0, const uint32_t* step_dev, float alpha_mse_coef, float rate_out,
                               uint32_t site_out0, const float* ext, int32_t ext_ts, int32_t ext_bs, uint32_t* sync,
                               float* guard_out, void* stream);
/* the _ext launch with the gradient of the initial cell state as one more output: dc0 [B][U] (nullable) is WRITTEN behind
 * the step loop with what the cell backward of step 0 leaves for the state in front of it,
 *   dc0[b][u] = dc_0[b][u] * f_0[b][u]     (dc_0 the cell-state gradient of step 0, f_0 its forget gate),
 * by the thread that owns the element, rows b < B only.  The gradient of the initial hidden state is not formed here: it is
 * dz[0] Ur^T + dqpre[0] W2^T, two products over outputs of this launch.  dc0 == NULL: the three entries above, bit for bit
 * (they forward here). */
int32_t tnt_lc_seq_bwd_init_f32(const float* F, const float* P, const float* W2, const float* v, const float* qpre,
                                const float* alpha, const uint8_t* keep4, int64_t keep_stride, float* dP, float* dF,
                                float* dvb, float* dqpre, const float* Ur, const float* Wc, const float* dout,
                                const float* gates, const float* cs, float* dz, float* work, int32_t T, int32_t B,
                                int32_t R, int32_t D, int32_t A, int32_t U, float slope, float rate_attn,
                                float rate_in, int32_t in_lwidth, uint64_t seed, uint32_t site_attn0,
                                uint32_t site_in0, const uint32_t* step_dev, float alpha_mse_coef, float rate_out,
                                uint32_t site_out0, const float* ext, int32_t ext_ts, int32_t ext_bs, float* dc0,
                                uint32_t* sync, float* guard_out, void* stream);

/* ---- the attention layer's hoisted first Dense (P = LeakyReLU(F W1 + b1), attention.py:32) backward, behind the chain:
 * with dP [rows][A] the score gradient accumulated over the T steps and Ppre its pre-activation:
 *   g = dP * LeakyReLU'(Ppre, slope);  db1 = column sums of g;  dW1 [D][A] = F^T g;  dF [rows][D] += g W1^T
 * (lc_NIC.py:386-387) in two launches; g is not stored.  part: tnt_attention_front_bwd_parts(rows, D, A) floats of
 * scratch.  D = A = 32 (the reference's attention width; other sizes: TNT_BADARG, use the generic entry points).
 * Deterministic (partials summed in row-chunk order). */
int32_t tnt_attention_front_bwd_parts(int32_t rows, int32_t D, int32_t A);
int32_t tnt_attention_front_bwd_f32(const float* Ppre, const float* dP, const float* F, const float* W1, float* dF,
                                    float* dW1, float* db1, float* part, int32_t rows, int32_t D, int32_t A,
                                    float slope, void* stream);
/* ... and, with drop_rate > 0, the backward of the feature Dropout that produced F (layers.py:51) applied to the finished
 * dF in the same pass: dF = keep ? (dF + g W1^T) / (1 - rate) : 0, element row*D + d of stream (drop_seed, drop_site,
 * *drop_step_dev). */
int32_t tnt_attention_front_bwd_drop_f32(const float* Ppre, const float* dP, const float* F, const float* W1, float* dF,
                                         float* dW1, float* db1, float* part, int32_t rows, int32_t D, int32_t A,
                                         float slope, float drop_rate, uint64_t drop_seed, uint32_t drop_site,
                                         const uint32_t* drop_step_dev, void* stream);

/* attention "coverage" metric (lc_NIC.py:365-367): mean over (T,R) of
 * (1 - sum_b alpha[t][b][r])^2.  alpha is [T][B][R].  work: tnt_attention_metric_parts(T, R) floats of partial sums;
 * out == NULL: only the partials are written, and the metric is their sum times 1 / (T R) (taken by
 * tnt_step_finalize_f32's x2 job inside the fused training step). */
int32_t tnt_attention_metric_parts(int32_t T, int32_t R);
int32_t tnt_attention_metric_f32(const float* alpha, float* out, float* work,
                                 int32_t T, int32_t B, int32_t R,
                                 int64_t tstride /* floats between timesteps; 0 = B*R */, void* stream);

/* ---- attention coverage penalty ("doubly stochastic attention", Xu et al. 2015, section 4.2.1).  alpha [T][B][R] are the
 * attention weights of all steps (tstride floats between steps; <= 0 = B R).
 *   axis 0 ("time", Xu et al.):  s[b][r] = sum_t alpha[t][b][r],  N = B R
 *   axis 1 ("batch", the line of lc_NIC.py:365-367, whose axis=1 of the stacked (T, B, R, 1) scores is the batch axis):
 *                                s[t][r] = sum_b alpha[t][b][r],  N = T R; its value is tnt_attention_metric_f32's
 *   coverage = (1 / N) sum (1 - s)^2            (keras MeanSquaredError of s against ones)
 * The term a training step adds to its loss is weight * coverage, so
 *   d / d alpha[t][b][r] = (2 weight / N) (s - 1),  s the sum that holds the element.
 * The launch writes ext[b R + r] (axis 0) or ext[t R + r] (axis 1) = coef * (s - 1) -- the caller passes coef = 2 weight / N
 * and hands ext to tnt_lc_seq_bwd_ext_f32 / tnt_attention_step_bwd_ext_f32 with strides (ext_ts, ext_bs) = (0, R) or (R, 0)
 * -- and out[0] = coverage, unweighted.  ext == NULL: the value only (evaluation); out == NULL: ext only (one launch).
 * Every sum is taken in ascending index order in float32 and the partial sums of (1 - s)^2 meet in a fixed order: no
 * atomics, the same bits every time.  work: rows * ceil(R / 256) floats with rows = B for axis 0 and T for axis 1. */
int32_t tnt_attention_coverage_f32(const float* alpha, int64_t tstride, int32_t T, int32_t B, int32_t R, int32_t axis,
                                   float coef, float* ext, float* out, float* work, void* stream);

/* ---- learned initial LSTM state of the attention model (Xu et al. 2015, section 3.1.2: "the initial memory state and
 * hidden state of the LSTM are predicted by an average of the annotation vectors fed through two separate MLPs"; the
 * reference's learn_init_state, lc_NIC.py:169-173, whose two layers it never builds).  F [B][R][D] are the region features
 * the attention reads, Wh / Wc [D][U] and bh / bc [U] the two layers:
 *   m[b][d] = (1/R) sum_r F[b][r][d]
 *   h0[b][u] = tanh(bh[u] + sum_d m[b][d] Wh[d][u])
 *   c0[b][u] = tanh(bc[u] + sum_d m[b][d] Wc[d][u])
 * One launch, one workgroup per sample.  fmean [B][D] (nullable: inference) receives m for the backward; h0 and c0 [B][U]
 * are written (the callers pass slab 0 of the chains' hs / cs).  Any B, R, U >= 1 and 1 <= D <= 64, no alignment
 * requirement; anything else: TNT_BADARG.  Row b's bits depend on F[b] and the weights alone -- not on B, not on the row's
 * position -- and every sum runs in a fixed order (regions in 256 / D interleaved groups, each ascending, the groups in
 * order; d ascending from the bias): no atomics, the same bits every time. */
int32_t tnt_init_state_fwd_f32(const float* F, const float* Wh, const float* bh, const float* Wc, const float* bc,
                               float* fmean, float* h0, float* c0, int32_t B, int32_t R, int32_t D, int32_t U,
                               void* stream);
/* its backward.  dh0 / dc0 [B][U] are the gradients of the two outputs, h0 / c0 the outputs themselves, fmean the forward's:
 *   gh = dh0 (1 - h0^2),  gc = dc0 (1 - c0^2)
 *   dWh [D][U] = fmean^T gh,  dbh [U] = column sums of gh,  dWc, dbc likewise from gc      -- WRITTEN, not accumulated
 *   dF[b][r][:] += (1/R) (gh Wh^T + gc Wc^T)[b][:]  for every region r                    -- ADDED to what dF holds
 * dF [B][R][D] is nullable (the parameter gradients alone: one launch instead of two); so are the four parameter gradients,
 * all of them or none (NULL: both layers frozen, the dF launch alone).  fmean is required.  Same sizes as the forward.  No
 * scratch, no atomics; the sums over b (ascending) and over u (per lane ascending, then the 64-lane butterfly) run in a
 * fixed order: the same bits every time. */
int32_t tnt_init_state_bwd_f32(const float* dh0, const float* dc0, const float* h0, const float* c0, const float* fmean,
                               const float* Wh, const float* Wc, float* dWh, float* dbh, float* dWc, float* dbc, float* dF,
                               int32_t B, int32_t R, int32_t D, int32_t U, void* stream);

/* ---- sentence-embedding target: cosine loss, inverse row norms, cosine top-k (csrc/semantic.hip).  The reference hands every
 * model the caption's sentence embedding ("GUSE") and defines cosine_loss = 1 - cosine_similarity (lc_NIC.py:488-502) with
 * keras l2_normalize, epsilon 1e-12.  All three entries are float32, take every sum in a fixed order and use no float atomics:
 * the same bits every time, and row r's outputs depend on row r's inputs alone (not on B / rows, not on the row's place).
 *
 * tnt_cosine_loss_f32.  z [B][ldz] the predictions, g [B][ldg] the targets, G <= ldz, ldg columns used, 1 <= G <= 2048:
 *   nz2 = max(sum_j z_j^2, 1e-12),  ng2 = max(sum_j g_j^2, 1e-12),  nz = sqrt(nz2),  ng = sqrt(ng2)
 *   zn = z / nz,  gn = g / ng,  cos = sum_j zn_j gn_j  (formed as ((sum_j z_j g_j) * (1 / nz)) * (1 / ng)),  loss = 1 - cos
 *   cos_row[r] = cos,  loss_row[r] = loss,  out[0] (nullable) = (sum_r loss_row[r]) / B, the rows added in ascending order
 *   dz (nullable) [B][ldz], the gradient of gscale * sum_r loss_r:
 *     sum z^2 >  1e-12:  dz_j = -gscale * (gn_j - cos * zn_j) / nz
 *     sum z^2 <= 1e-12:  dz_j = -gscale * gn_j / nz            (the normaliser is the constant 1e-6 there)
 *   A training step passes gscale = weight / B.  An all-zero target row has gn = 0: cos = 0, loss = 1, dz = 0, and it counts
 *   in the mean.  dz may be z itself (each element is read, then written, by the same lane); columns >= G of dz are not
 *   written.  The three sums of a row: lane l of one wave takes the float4 l, l + 64, ... (the four elements in order) and
 *   then the G % 4 tail, by fused multiply-add, then the 64-lane butterfly; without 16-byte alignment of z, g, dz or with ldz
 *   or ldg not a multiple of 4 the lanes take single floats l, l + 64, ... instead.  B <= 256 is one launch; above, a second
 *   one-thread launch forms out.  Null z, g, loss_row or cos_row, B < 1, G outside [1, 2048], ldz < G, ldg < G: TNT_BADARG,
 *   nothing launched. */
int32_t tnt_cosine_loss_f32(const float* z, int32_t ldz, const float* g, int32_t ldg, float* dz /* nullable */,
                            float* loss_row, float* cos_row, float* out /* nullable */, int32_t B, int32_t G, float gscale,
                            void* stream);
/* inv[r] = 1 / sqrt(max(sum_j X[r][j]^2, 1e-12)) for the rows of X [rows][ldx], G <= ldx columns used, any G >= 1; the sum as
 * in tnt_cosine_loss_f32 (one wave per row).  Null pointers, rows < 1, G < 1, ldx < G: TNT_BADARG. */
int32_t tnt_row_inv_norm_f32(const float* X, int64_t ldx, float* inv, int64_t rows, int32_t G, void* stream);
/* The k most similar bank rows of every query.  S [B][lds] holds the raw dot products S[b][m] = <q_b, bank_m>, M <= lds
 * columns used, qinv [B] and binv [M] the inverse norms (tnt_row_inv_norm_f32).  The similarity is
 *   c[b][m] = (S[b][m] * qinv[b]) * binv[m]        two float32 multiplications, in exactly this order
 * idx [B][k] (int32) and sim [B][k] receive the k largest of row b in descending order of this total order: a larger c comes
 * first; equal c (-0 equals +0) in ascending index order (the first-max rule of every argmax in this library); NaN comes
 * behind -inf, and NaNs among themselves in ascending index order.  sim holds c's own bits.  1 <= k <= 64, k <= M, any
 * M >= 1 (a row is read k times and is expected to stay in the L2: 256 KB at M = 65 536).  A null pointer, B < 1, M < 1,
 * k outside [1, min(64, M)], lds < M: TNT_BADARG, nothing launched. */
int32_t tnt_cosine_topk_f32(const float* S, int64_t lds, const float* qinv, const float* binv, int32_t* idx, float* sim,
                            int32_t B, int32_t M, int32_t k, void* stream);

/* ---- contrastive sentence-embedding loss (csrc/contrastive.hip): the CLIP-style form of nic.NIC's semantic target, with in-batch
 * negatives, a temperature, both directions and optional soft targets.  z [B][ldz] the predictions, g [B][ldg] the targets,
 * G <= ldz, ldg columns used; 1 <= B <= 1024, 1 <= G <= 2048; eps = 1e-12 as in tnt_cosine_loss_f32.
 *   iz_i = 1 / sqrt(max(sum z_i^2, eps)),  ig_j likewise,  zn = z iz,  gn = g ig
 *   valid_j = (sum g_j^2 > eps)                 an all-zero target is the reference's missing embedding
 *   Bv = number of valid rows
 *   L_ij = (zn_i . gn_j) inv_temperature         over valid i, j only; formed as (((z_i . g_j) iz_i) ig_j) inv_temperature
 *   Q_ij = [i == j]                              hard targets (soft_inv_temperature == 0)
 *   Q_i. = softmax_j(S_ij) over valid j,  S_ij = ((g_i . g_j) (ig_i ig_j)) soft_inv_temperature      soft (S_ij and S_ji: the same bits)
 *   lr_i = - sum_j Q_ij log softmax_j(L_i.)_j    scan -> caption
 *   lc_i = - sum_j Q_ij log softmax_j(L_.i)_j    caption -> scan: column i of L, softmax over rows
 *   loss_row[i] = symmetric ? 0.5 (lr_i + lc_i) : lr_i;  0 for an invalid row
 *   hit_row[i]  = valid_i and (first argmax over valid j of L_ij) == i
 *   out[0] (out nullable) = (sum_i loss_row[i]) / max(Bv, 1),  out[1] = (sum_i hit_row[i]) / max(Bv, 1), the rows added in
 *   ascending order in float32
 *   dz (nullable) [B][ldz], the gradient of weight * out[0] in z:
 *     dL_ij = weight / max(Bv, 1) * ((1 - b) (Pr_ij - Q_ij) + b (Pc_ij - Q_ji)),  b = symmetric ? 0.5 : 0,
 *             Pr the row softmax of L, Pc_ij the softmax over rows of column j
 *     dzn_i = inv_temperature sum_j dL_ij gn_j     (valid j in ascending order, one accumulator per column)
 *     dz_i  = iz_i (dzn_i - zn_i (zn_i . dzn_i));  where sum z_i^2 <= eps the normaliser is the constant 1e-6: dz_i = iz_i dzn_i
 *   There is no gradient to g.  An invalid row gets dz = 0 and takes no part in any softmax, neither as a row nor as a column.
 *   Bv = 0 and B = 1 give loss 0 and a zero gradient.  Every softmax subtracts its maximum.  dz may be z itself (an element
 *   of z is read, then that element of dz written, by the same thread, in the last launch that reads z); columns >= G of z, g
 *   and dz are neither read nor written.  No alignment is asked of any pointer.
 * work is scratch of TNT_CONTRASTIVE_WORK_FLOATS(B, soft) floats: sum z^2 [B], sum g^2 [B], the row, column and target
 * log-sum-exp [B] each, L [B][B] and, soft, S [B][B].
 * Launches, in order on the one stream (a phase that needs another's result is another launch; no workgroup waits for
 * another): the logits in 16 x 16 tiles with the squared norms beside them; one wave per row for the log-sum-exp, loss and hit;
 * (dz given) one workgroup per row for the gradient; (out given) one launch for the two means.  float32, no float atomics,
 * every sum in a fixed order that does not depend on the grid: the same bits every time.
 * A null z, g, work, loss_row or hit_row: TNT_BADARG(1); ldz < G (2), ldg < G (4), B outside [1, 1024] (10), G outside
 * [1, 2048] (11), inv_temperature not a finite number > 0 (12), soft_inv_temperature not a finite number >= 0 (13), symmetric
 * not 0 or 1 (14), weight not a finite number >= 0 (15); nothing launched. */
#define TNT_CONTRASTIVE_WORK_FLOATS(B, soft) (5 * (B) + ((soft) ? 2 : 1) * (B) * (B))
int32_t tnt_contrastive_loss_f32(const float* z, int32_t ldz, const float* g, int32_t ldg, float* dz /* nullable, may be z */,
                                 float* work, float* loss_row, int32_t* hit_row, float* out /* nullable: [0] loss, [1] top1 */,
                                 int32_t B, int32_t G, float inv_temperature, float soft_inv_temperature /* 0: hard */,
                                 int32_t symmetric, float weight, void* stream);

/* ---- symmetric positive-definite solves for ridge decoding (csrc/cholesky.hip; masters_thesis_amd/ridge.py).  The baseline of
 * every fMRI decoding paper -- ridge regression from the voxels to the sentence embedding -- in its dual form needs, for the
 * n x n Gram matrix K of the scans, (K + alpha I) A = Y per regularisation strength.  Everything is float32 in memory; the
 * 64 x 64 triangular work is done in float64 in LDS and rounded once.  No workgroup waits for another inside a launch (launch
 * boundaries are the only synchronisation: no spin, no flag), no float atomics, every sum in a fixed order: the same input
 * gives the same bits.  The products run on this library's own family, called inside the library: tnt_gemm3_f32 at the tile
 * tnt_gemm3_plan picks with allow_split = 0 (no exchange buffer, no sync word), or tnt_gemm_f32 (splitk 1) where gemm3's
 * 32-bit operand offsets do not reach (n * ld >= 2^29 floats); the choice depends on the sizes alone.
 *
 * tnt_cholesky_f32: the lower factor of K + shift I,  L L^T = K + shift I.
 *   K [n][ldk] symmetric; only its lower triangle (diagonal included) is read and it is never written, so one Gram matrix
 *   serves every shift.  L [n][ldl] is another buffer; only its lower triangle (diagonal included) is written; its strictly
 *   upper triangle and its pad columns [n, ldl) are neither read nor written by the kernels of this file (a product may fetch
 *   such floats beside an M-contiguous operand; they only reach rows of its result that are not stored).
 *   Blocked left-looking at NB = 64.  For block column j (j0 = 64 j, nb = min(64, n - j0)), in stream order:
 *     (j > 0) one product  P = L[j0:, :j0] L[j0:j0+nb, :j0]^T  into work, [n - j0][64].  Both operands are K-contiguous with
 *       K = j0, a multiple of 64, so no stage of gemm3 reaches past K: its "finite behind K" contract holds by construction.
 *     one panel launch of ceil((n - j0) / 64) workgroups.  Each factors D = K[j0:j0+nb, j0:j0+nb] + shift I - P[:nb] itself in
 *       float64 (right-looking inside the block, a_ij -= a_ik a_jk / a_kk, L_ik = a_ik / sqrt(a_kk)), rounds it to float32
 *       once, and then workgroup 0 stores L11 while workgroup b >= 1 solves rows [j0 + 64 b, j0 + 64 b + 64) of
 *       L21 = (K21 - P21) L11^-T against the rounded L11 in float64 and stores them rounded once.
 *   work: 64 * n floats (n - 64 rows suffice).  status: one int32 in device memory, set to 0 by the call (a memset node on
 *   the stream).  A pivot a_kk that is not finite, is <= 0, or whose square root is not a positive finite float32 sets
 *   status = 1 + its row index; all workgroups of a panel find the same pivot, the first in row order, and one of them files
 *   it.  A panel or triangular launch that finds status != 0 returns before it touches anything else; the products of the
 *   remaining block columns still run, over whatever L holds, into work alone.  A matrix that is not positive definite, or
 *   one with a NaN, therefore cannot fault and costs idle launches; L is then unspecified.
 *   TNT_BADARG, nothing launched: K null or not 16-byte aligned (1), ldk < n or not a multiple of 4 (2), L null, unaligned or
 *   K itself (3), ldl likewise (4), n outside [1, 32768] (5), work null or unaligned (7), status null (8).
 *
 * tnt_cholesky_solve_f32: X <- L^-T L^-1 X in place, the solution of (L L^T) A = X.  X [n][ldx], G >= 1 columns used.
 *   Forward sweep, block rows ascending:  (j > 0) P = L[j0:j0+nb, :j0] X[:j0] into work [64][ldx], then one launch of
 *   ceil(G / 64) workgroups: X_j <- L_jj^-1 (X_j - P).  Backward sweep, descending: (rows below) P = L[j0+64:, j0:j0+64]^T
 *   X[j0+64:], then X_j <- L_jj^-T (X_j - P).  The triangular launches hold 64 columns of X_j in float64 in LDS and round once.
 *   Only the lower triangle of L is read.  The forward product's A has K = j0, a multiple of 64; the backward product has no
 *   K-contiguous operand.  If *status != 0 on entry every triangular launch returns untouched and X keeps its bits.
 *   work: 64 * ldx floats.  TNT_BADARG: L null / unaligned (1), ldl < n or not a multiple of 4 (2), n outside [1, 32768] (3),
 *   X null / unaligned (4), ldx < G or not a multiple of 4 (5), G < 1 (6), work null / unaligned (7), status null (8).
 *
 * tnt_gram_center_f32: K <- H K H in place, H = I - 11^T / n, for a symmetric K [n][ldk] (both triangles held), so that the
 *   n x N scans are never copied or centred themselves.  mean: n + 1 floats, kept for the caller (the centred cross-Gram of
 *   new rows needs the training means): mean[i] = (sum_j K_ij) / n, mean[n] = (sum_i mean[i]) / n.  Two launches: one wave per
 *   row for the means (lane l adds the float4 l, l + 64, ... in float64, then the butterfly); then 16 rows per workgroup,
 *   every workgroup forming the grand mean itself from mean[0..n) in float64 in one fixed order (thread t adds t, t + 256, ...,
 *   then a binary tree), and K_ij <- (float)((double)K_ij - mean[i] - mean[j] + grand).  tnt_colsum_f32 is not used for the
 *   first half: it adds in float32 over row chunks through a work buffer, and the means here are taken in float64.
 *   TNT_BADARG: K null / unaligned (1), ldk < n or not a multiple of 4 (2), n outside [1, 32768] (3), mean null (4). */
int32_t tnt_cholesky_f32(const float* K, int32_t ldk, float* L, int32_t ldl, int32_t n, float shift, float* work,
                         int32_t* status, void* stream);
int32_t tnt_cholesky_solve_f32(const float* L, int32_t ldl, int32_t n, float* X, int32_t ldx, int32_t G, float* work,
                               const int32_t* status, void* stream);
int32_t tnt_gram_center_f32(float* K, int32_t ldk, int32_t n, float* mean, void* stream);

/* ---- symmetric eigensolver of order <= 128 for PCA of the scans (csrc/eigen.hip; masters_thesis_amd/pca.py).  Block subspace
 * iteration on the n x n Gram matrix of the scans needs two small dense decompositions per iteration: the eigenvectors of the
 * m x m Ritz matrix and the matrix that orthonormalises a block of m columns from their Gram matrix.  Both are ONE launch of ONE
 * workgroup (16 waves) of the same kernel, with the matrix and the eigenvectors held in LDS in float32 (two 128 x 129 float
 * arrays, 132 KB of the CU's 160 KB, as dynamic LDS).  No atomics, every sum and every rotation in a fixed order: the same
 * input gives the same bits.
 *
 * tnt_syev_jacobi_f32: all eigenvalues and eigenvectors of the symmetric float32 matrix A [m][lda], 1 <= m <= 128.
 *   Only A's lower triangle (diagonal included) is read; it is mirrored on load; A is never written.
 *   Cyclic Jacobi in the round-robin ordering of the circle method over n2 = m rounded up to even, n1 = n2 - 1: round r
 *   (0 <= r < n1) holds the pairs {r, n1} (slot 0) and {(r + k) mod n1, (r - k) mod n1} for slots k = 1 .. n2 / 2 - 1, each
 *   ordered p < q.  For odd m index n1 = m is the bye and slot 0 is left out: a round has floor(m / 2) disjoint pairs for
 *   every m, and a sweep has m - 1 rounds for even m and m rounds for odd m (m (m - 1) / 2 pairs either way).
 *   Pair (p, q) of a round is rotated iff  |a_qp| > 2^-24 sqrt(|a_pp a_qq|)  and  |a_qp| > 2^-24 ||A||_F / sqrt(m),  both
 *   evaluated in float64 on the float32 entries the round starts with; ||A||_F is taken once at load in float64 (each row
 *   left to right, then the rows top to bottom).  For a rotated pair, in float64:  th = (a_qq - a_pp) / (2 a_qp),
 *   t = sign(th) / (|th| + sqrt(1 + th^2)) (sign(0) = +1), c = 1 / sqrt(1 + t^2), s = t c, rounded once to float32, and the
 *   new diagonal pair a_pp - t a_qp, a_qq + t a_qp, rounded once.  Then A <- J^T A J and V <- V J, J = [c s; -s c] on (p, q), in
 *   float32:  x' = fma(c, x, -(s y)),  y' = fma(s, x, c y);  the 2 x 2 block itself is set to the new diagonal pair and two
 *   exact zeros.  Both triangles of A are kept; decisions read the lower one.
 *   The kernel stops after the first sweep in which no pair rotated (info[0] = 0) or after max_sweeps sweeps (info[0] = 1; w
 *   and V are written and are what the last sweep left).
 *   w [m]: the diagonal in descending order, ties in ascending order of the column they came from.  V [m][ldv]: column i is
 *   the eigenvector of w[i] as the float32 rotations left it (unit to rounding), negated where needed so that its entry of
 *   largest magnitude -- the first one on ties -- is positive.  Columns [m, ldv) of V are not written.
 *   info: three int32 words in device memory.  info[0]: 0 converged; 1 not converged within max_sweeps; 2 a non-finite entry in
 *   the lower triangle, w and V untouched.  info[1]: sweeps run (the last, rotation-free one included).  info[2]: m.
 *   TNT_BADARG, nothing launched: A null or not 16-byte aligned (1), lda < m or not a multiple of 4 (2), m outside [1, 128] (3),
 *   w null or not 4-byte aligned (4), V null or not 16-byte aligned (5), ldv < m or not a multiple of 4 (6), max_sweeps outside
 *   [1, 64] (7), info null or not 4-byte aligned (8), V == A (9); the dynamic LDS refused by the device (90).
 *
 * tnt_gram_whiten_f32: M [m][ldm] with (Z M)^T (Z M) = I from the Gram matrix S = Z^T Z [m][lds] of a block of m columns
 *   (lower triangle read).  d_j = S_jj; r_j = 1 / sqrt(d_j) in float64 where d_j is finite and > 0, else 0 (a zero column is
 *   dropped); C = diag(r) S diag(r) formed in float64 and rounded once; (w, W) = the eigen-decomposition of C exactly as above
 *   (max_sweeps 64, the sort and the sign rule included);  M = diag(r) W diag(1 / sqrt(max(w_i, tau w_0))), a column whose
 *   max(w_i, tau w_0) is not > 0 set to zero, formed in float64 and rounded once.  w [m]: the eigenvalues of C.  info[0] and
 *   info[1] as above; info[2]: the number of w_i > tau w_0, the numerical rank (0 with info[0] = 2).  Where the rank is full Z M
 *   has orthonormal columns; where it is not, its columns have norm <= 1 and span the same space, and nothing is NaN.  The
 *   scaling to unit diagonal makes C well conditioned for nearly orthogonal columns however they are graded.
 *   TNT_BADARG: S null / unaligned (1), lds < m or not a multiple of 4 (2), m outside [1, 128] (3), M null / unaligned (4),
 *   ldm < m or not a multiple of 4 (5), tau not in (0, 1) (6), w null / not 4-byte aligned (7), info likewise (8), M == S (9);
 *   (90) as above. */
int32_t tnt_syev_jacobi_f32(const float* A, int32_t lda, int32_t m, float* w, float* V, int32_t ldv, int32_t max_sweeps,
                            int32_t* info, void* stream);
int32_t tnt_gram_whiten_f32(const float* S, int32_t lds, int32_t m, float* M, int32_t ldm, float tau, float* w, int32_t* info,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNT_HIP_H */
