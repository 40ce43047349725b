/* klab_mm.h -- C ABI of the MI355X-native Swin-V2 -> T5 caption-training hot path.
 *
 * The reference (Da-Tsuchi/KLab_MultiModalModel) has no FFI of its own: its hot path is the
 * Python call `MyModel.forward` + autograd backward (ref/models/model.py:19-26, ref/train.py:58-62),
 * whose arithmetic runs inside `transformers` (HF/swinv2, HF/t5; see SURVEY.md for the prefixes).
 * This header is the boundary a maintainer would bind instead (last row): plain
 * pointers and sizes, no torch types.  Conventions for EVERY entry point:
 *   - all buffers are caller-owned device allocations; nothing is allocated, freed or retained
 *     (the engine object is the one exception: it owns only host-side plans);
 *   - every call is stream-ordered on the `hipStream_t` passed as `void* stream`, never
 *     synchronises and never throws; it returns 0, a positive `hipError_t`, or a negative KLAB_ERR_*;
 *   - `dtype` is the storage type of GEMM operands / activations: KLAB_F32 (parity mode, exact f32
 *     MFMA) or KLAB_BF16 (bf16 operands, fp32 accumulation, fp32 residual stream and statistics);
 *   - dropout masks are a pure function of (*seed_dev, tag, element index) so that backward
 *     regenerates them; `seed_dev` points to ONE uint32 in device memory (graph-replay friendly).
 */
#ifndef KLAB_MM_H
#define KLAB_MM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KLAB_OK 0
#define KLAB_ERR_UNSUPPORTED (-2)
#define KLAB_ERR_BADARG (-3)

#define KLAB_F32 0
#define KLAB_BF16 1
#define KLAB_FP8 2 /* engine mode only (klab_model_cfg.dtype): bf16 storage and backward, forward Linear GEMMs on fp8 MFMA */

#define KLAB_ACT_NONE 0
#define KLAB_ACT_RELU 1 /* T5 DenseReluDense, HF/t5:83-94 */
#define KLAB_ACT_GELU 2 /* erf GELU, Swin-V2 MLP, HF/swinv2:539-548 */

#define KLAB_AUX_NONE 0
#define KLAB_AUX_NONZERO 1 /* x = aux!=0 ? x*aux_scale : 0   (backward of relu+dropout) */
#define KLAB_AUX_DGELU 2   /* x *= gelu'(aux)                (backward of erf GELU)    */

int klab_version(void);

/* ---- dense contraction (replaces every nn.Linear / Conv2d-as-GEMM of HF/t5 and HF/swinv2 and
 *      their autograd dgrad/wgrad; SURVEY §2.4 K1,K5,K6,K11-K14) -------------------------------
 * C[M,N] = epilogue(alpha * sum_k A(m,k) * B(n,k)).
 * a_kmajor=1: A(m,k) = A[m*lda + k]   (x[M,K] of a Linear forward)
 * a_kmajor=0: A(m,k) = A[k*lda + m]   (contraction over the slow dimension: wgrad)
 * same for B (b_kmajor=1 is a torch Linear weight W[N,K]).                                      */
typedef struct klab_gemm_args {
  int M, N, K;
  int dtype;   /* operand dtype */
  const void* A; long lda; int a_kmajor;
  const void* B; long ldb; int b_kmajor;
  void* C; long ldc; int c_dtype; /* KLAB_F32 or == dtype */
  int accumulate;                 /* C += result */
  float alpha; const float* alpha_dev; /* effective alpha = alpha * (*alpha_dev if non-null) */
  const float* bias;              /* [N] f32 or NULL */
  int act;
  const void* aux; long ldaux; int aux_mode; float aux_scale; /* aux: [M,N] in `dtype` */
  const void* residual; long ldr; int r_dtype;                /* added last */
  float drop_p; const uint32_t* seed_dev; uint32_t drop_tag;  /* dropout before the residual */
  int name_tag; /* 1: launch under the symbol klab_lmhead_gemm (128x128 NT tile) so profiles can single it out;
                   2: take the 256x256 eight-wave kernel (mm8p) whenever the shape is legal for it, 3: never (A/B, tests) */
  int atomic_ok; /* with accumulate=1 and a plain f32 product: the kernel may split K and add partial sums with
                    float atomics (summation order, hence the last bits, then vary run to run) */
} klab_gemm_args;
int klab_gemm(const klab_gemm_args* args, void* stream);
/* measurement only: HIP events around every klab_gemm launch (on the stream it is launched on) while enabled; read returns the launch
 * count, the summed duration and the summed algorithmic FLOPs (2 M N K) since it was enabled.  Call read after a synchronize.          */
int klab_gemm_probe_enable(int on);
int klab_gemm_probe_read(int* launches, float* total_ms, double* flops_total);
/* fp8 forward GEMM (BASELINE configs[4]): C = epilogue(alpha * sa[m] * sb[n * b_scale_stride] * sum_k A8(m,k) B8(n,k)).
 * A, B: OCP e4m3 bytes, both K-major (lda / ldb in bytes = elements); a_row_scale [M] and b_row_scale are the per-row
 * dequantisation scales klab_quant_fp8_rows / klab_quant_fp8_arena produce (amax / 448).  Every other field of klab_gemm_args
 * as for klab_gemm with dtype = KLAB_BF16 (bias, act, dropout, residual, bf16 / f32 output); accumulate is not supported.
 * K % 16 == 0, 16-byte aligned operands.                                                                             */
int klab_gemm_fp8(const klab_gemm_args* a, const float* a_row_scale, const float* b_row_scale, long b_scale_stride, void* stream);
/* x [M, K] bf16 rows -> x8 [M, K] e4m3 + row_scale[m] = amax(row) / 448 (1 for an all-zero row); K <= 4096, K % 8 == 0 */
int klab_quant_fp8_rows(const void* x, long ldx, int M, int K, void* x8, long ld8, float* row_scale, void* stream);
/* all GEMM weights of a bf16 arena in one launch: desc_dev[i] = {long arena_off, rows, K, first_row}; row r of tensor i is
 * quantised to arena_fp8 + off + r*K with its scale at scales[(off + r*K) / 8]                                         */
int klab_quant_fp8_arena(const void* desc_dev, int ndesc, long total_rows, const void* arena_bf16, void* arena_fp8, float* scales,
                         void* stream);
/* n independent GEMMs.  Weight-gradient members (bf16, both operands m-major, f32 C with atomic_ok, no epilogue extras) are
 * batched into single launches of up to 8; every other member is run through klab_gemm.  Per member: accumulate = 1 adds to C
 * (split along K, float atomics); accumulate = 0 stores the product (never split, plain stores, C is not read). */
int klab_gemm_grouped(const klab_gemm_args* list, int n, void* stream);
/* the same with the choice of tile: large_tiles = 0 is klab_gemm_grouped; large_tiles = 1 runs the WHOLE list (at most 32 members) in one
 * launch on 256 x 256 tiles without split-K or atomics when every member has that form (as above, and N >= 128, K % 64 == 0, K >= 1024,
 * ldc % 4 == 0); a list with any other member, or with more than 32, is run whole as large_tiles = 0 would. */
int klab_gemm_grouped_tiles(const klab_gemm_args* list, int n, int large_tiles, void* stream);

/* ---- T5 RMS-norm (T5LayerNorm, HF/t5:59-72) ------------------------------------------------
 * y = drop(x * rsqrt(mean(x^2)+eps) * w); x is the f32 residual stream [rows,d]; y (dtype y_dtype)
 * and/or y_f32 are written at row (row/grp)*grp_stride + row%grp + off when grp>0 (this is how the
 * frozen language encoder writes its output straight into the concatenated encoder input,
 * ref/models/model.py:23).  rstd[rows] is saved for backward (may be NULL).                     */
int klab_rmsnorm_fwd(const float* x, const float* w, void* y, int y_dtype, float* y_f32, float* rstd, int rows, int d,
                     float eps, int grp, int grp_stride, int off, float drop_p, const uint32_t* seed_dev,
                     uint32_t tag, void* stream);
/* backward: dx = dres + rmsnorm'(dy * dropmask_y); dw += ...; dxt = dtype(dx * dropmask_prev)
 * (dxt is the gradient of the previous sub-layer's GEMM output: residual add + dropout of
 * HF/t5:400,141).  dy is indexed through the same row remap as y.                              */
/* fp8 mode: the norm's bf16 output AND the same rows in OCP e4m3 (y8 [rows, d]) with one dequantisation scale per row --
 * klab_quant_fp8_rows folded into the kernel that owns the row; bit-identical to norm followed by that pass.  d <= 1024.        */
int klab_rmsnorm_fwd_q8(const float* x, const float* w, void* y_bf16, float* rstd, void* y8, float* yscale, int rows, int d, float eps,
                        float drop_p, const uint32_t* seed_dev, uint32_t tag, void* stream);
int klab_layernorm_fwd_q8(const void* y_bf16, const float* gamma, const float* beta, const float* shortcut, float* out, void* outt_bf16,
                          float* mean, float* rstd, void* o8, float* oscale, int rows, int C, float eps, void* stream);
int klab_gelu_fwd_q8(const void* x_bf16, void* y_bf16, void* y8, float* yscale, int rows, int F, void* stream); /* F <= 4096, F % 8 == 0 */
int klab_rmsnorm_bwd(const float* dy, const float* x, const float* w, const float* rstd, const float* dres, float* dx,
                     void* dxt, int dxt_dtype, float* dw, int rows, int d, int grp, int grp_stride, int off,
                     float p_y, uint32_t tag_y, float p_prev, uint32_t tag_prev, const uint32_t* seed_dev,
                     void* stream);
/* Deferred weight gradient: same as klab_rmsnorm_bwd, but dw is left as per-workgroup partial sums
 * dw_part[klab_rmsnorm_part_rows(rows), d]; several calls' partials (call c at part + c*call_stride) are then folded into
 * their dw vectors by ONE klab_colpart_reduce (fixed summation order: bit-reproducible, and no same-address atomics). */
int klab_rmsnorm_part_rows(int rows);
int klab_rmsnorm_bwd_part(const float* dy, const float* x, const float* w, const float* rstd, const float* dres, float* dx, void* dxt,
                          int dxt_dtype, float* dw_part, int rows, int d, int grp, int grp_stride, int off, float p_y, uint32_t tag_y,
                          float p_prev, uint32_t tag_prev, const uint32_t* seed_dev, void* stream);
int klab_colpart_reduce(const float* part, long call_stride, int nparts, int d, float* const* dst_dev, int ncalls, void* stream);

/* ---- Swin-V2 LayerNorm, res-post-norm form (HF/swinv2:697-702; also :242, :354, :953) --------
 * out = drop(shortcut + LN(y)*gamma + beta)  (f32, remapped rows) and/or outt (dtype copy).     */
int klab_layernorm_fwd(const void* y, int y_dtype, const float* gamma, const float* beta, const float* shortcut,
                       float* out, void* outt, int outt_dtype, float* mean, float* rstd, int rows, int C, float eps,
                       int grp, int grp_stride, int off, float drop_p, const uint32_t* seed_dev, uint32_t tag,
                       void* stream);
int klab_layernorm_bwd(const float* dout, const void* y, int y_dtype, const float* gamma, const float* mean,
                       const float* rstd, void* dy, float* dgamma, float* dbeta, int rows, int C, int grp,
                       int grp_stride, int off, float drop_p, const uint32_t* seed_dev, uint32_t tag, void* stream);
/* the same, and dprev_bias[c] += sum_rows dy[:, c] -- the bias gradient of the Linear whose output the norm consumed (its input
 * gradient is dy) -- in the same pass (C <= 1024: one fused kernel for dy, dgamma, dbeta and dprev_bias)                      */
int klab_layernorm_bwd_bias(const float* dout, const void* y, int y_dtype, const float* gamma, const float* mean,
                            const float* rstd, void* dy, float* dgamma, float* dbeta, float* dprev_bias, int rows, int C, int grp,
                            int grp_stride, int off, float drop_p, const uint32_t* seed_dev, uint32_t tag, void* stream);

/* ---- T5 attention core (HF/t5:144-173 as called from :281-369) ------------------------------
 * S = Q K^T (unscaled, HF/t5:196-197) + bias[h,Lq,Lk] (+ causal); P = softmax(S); ctx = drop(P) V.
 * q/k/v/ctx/dq/dk/dv are [B*L, ld] matrices in `dtype`, head h at column h*dk (no transposes).
 * lse[B,H,Lq] (f32) is written by fwd and read by bwd; dbias[h,Lq,Lk] (f32) is ACCUMULATED by
 * bwd (position-bias gradient, shared by all layers: HF/t5:739-742) and may be NULL.            */
typedef struct klab_attn_args {
  int dtype;
  const void* q; long ldq;
  const void* k; long ldk;
  const void* v; long ldv;
  const float* bias; int causal;
  void* ctx; long ldo;
  float* lse;
  int B, H, Lq, Lk, dk;
  float drop_p; const uint32_t* seed_dev; uint32_t drop_tag;
  /* backward only */
  const void* dctx; long lddo;
  void* dq; long lddq;
  void* dk_out; long lddk;
  void* dv; long lddv;
  float* dbias;
  void* ds_ws; /* optional scratch [B,H,Lq,roundup(Lk,32)] in `dtype`: with it the position-bias gradient is a
                  deterministic batch reduction of stored dS instead of 64-way contended float atomics */
  int ds_defer; /* 1: only store dS; the caller reduces several layers' scratch at once with klab_dbias_reduce */
  /* backward, bf16 MFMA path only (used for the Swin-V2 window attention on window-ordered copies): */
  const float* score_scale; /* [H] device: S = score_scale[h] * Q K^T + bias (fp32), NULL = 1 */
  int bias_mod;             /* > 0: bias is [bias_mod, H, Lq, Lk] and batch element b uses slab b % bias_mod */
} klab_attn_args;
int klab_t5_attn_fwd(const klab_attn_args* a, void* stream);
int klab_t5_attn_bwd(const klab_attn_args* a, void* stream);
/* Front half of a T5 attention sub-layer in ONE launch (forward): T5LayerNorm (HF/t5:59-72) -> q|k|v projection (self, HF/t5:206-209)
 * or q projection (cross) -> attention core (HF/t5:144-173), one workgroup per (sample, head).  Replaces klab_rmsnorm_fwd + the
 * projection klab_gemm + klab_t5_attn_fwd of the serial chain; everything the backward pass reads is still written: xn (the
 * normalised rows, bf16) and rstd, the projected q|k|v (self: [B*Lq, 3*inner] column blocks q | k | v; cross: q [B*Lq, inner]),
 * attn.lse and attn.ctx.  attn.q / .k / .v are ignored for self attention; cross attention reads attn.k / attn.v (the projected
 * encoder output).  Envelope: bf16, d_model = 512, head dim 64, Lq <= 64, Lk <= 64 (self: Lk == Lq); otherwise
 * KLAB_ERR_UNSUPPORTED and the caller issues the three launches.                                                              */
typedef struct klab_attn_fused_args {
  const float* x; const float* gamma; float eps; int d_model;
  const void* w;            /* bf16 projection rows: self q|k|v [3*inner, d_model]; cross q [inner, d_model] */
  void* xn; float* rstd;    /* [B*Lq, d_model] bf16, [B*Lq] */
  void* proj; long ldproj;
  int cross;
  klab_attn_args attn;
} klab_attn_fused_args;
int klab_t5_attn_fused_fwd(const klab_attn_fused_args* a, void* stream);
/* Back half of a T5 attention sub-layer in ONE launch (backward): the o / co projection dgrad dctx_h = dy W[:, h*dk : h*dk+dk]
 * (K = d_model; bf16-rounded as the klab_gemm output, kept on chip, never written) -> delta = rowsum(dctx_h * ctx) -> the attention
 * backward (dq | dk | dv, and dS to attn.ds_ws / attn.dbias exactly as klab_t5_attn_bwd), one workgroup per (sample, head).
 * Replaces the projection klab_gemm + klab_t5_attn_bwd; attn.dctx / attn.lddo are ignored.  Envelope: bf16, d_model = 512,
 * head dim 64, H * dk = 512, 1 <= Lq, Lk <= 64, no score_scale / bias_mod; otherwise KLAB_ERR_UNSUPPORTED and the caller issues
 * the two launches.                                                                                                            */
typedef struct klab_attn_bwd_fused_args {
  const void* dy; long lddy; /* [B*Lq, d_model] bf16: gradient of the projection's output */
  const void* w;             /* [d_model, H*dk] bf16: the o / co projection weight (nn.Linear layout) */
  int d_model;
  klab_attn_args attn;
} klab_attn_bwd_fused_args;
int klab_t5_attn_bwd_fused(const klab_attn_bwd_fused_args* a, void* stream);
/* dbias[H,Lq,Lk] += sum over nbatch slabs of ds_ws [nbatch, H, Lq, roundup(Lk,32)] (bf16).  nbatch <= 64: one pass over the
 * slabs in a fixed order (bit-reproducible).  nbatch > 64: the slabs are cut into min(nbatch / 16, 32) chunks of consecutive slabs, each
 * chunk is summed in order and the chunks' sums are added to dbias with float atomics (the last bits then vary run to run).  The pad
 * columns Lk .. roundup(Lk,32)-1 of a slab are never read. */
int klab_dbias_reduce(const void* ds_ws, int dtype, float* dbias, int nbatch, int H, int Lq, int Lk, void* stream);

/* ---- Swin-V2 shifted-window cosine attention (HF/swinv2:389-455 + roll/partition/mask/reverse of
 * :652-705, :146-166, :620-643) -- one call per block.  qkv [B*R*R, 3C], ctx [B*R*R, C] (`dtype`),
 * bias [H, w*w, w*w] f32 (= 16*sigmoid(CPB), klab_swin_cpb_bias), logit_scale [H] f32 (raw param),
 * lse [B*nW*H*w*w] f32 (fwd out, optional; bwd in).  bwd writes dqkv and accumulates dbias /
 * dlogit_scale.  R % w must be 0 (the padded-window path is out of scope).
 * bwd_ws / bwd_ws_bytes (optional): scratch of at least klab_swin_attn_bwd_ws_bytes(...) bytes; with it (bf16, head dim 32,
 * w*w <= 64) the backward runs on the matrix cores -- window-ordered unit q|k|v copies, the T5 attention backward kernel with a
 * per-head score scale and the per-window bias+mask table, then the L2-normalisation Jacobian on the way back to token
 * order.  Without it (or outside that envelope) the vector-ALU kernel runs.                       */
typedef struct klab_swin_attn_args {
  int dtype;
  const void* qkv; void* ctx; const float* bias; const float* logit_scale; float* lse;
  int B, R, w, shift, H, C;
  const void* dctx; void* dqkv; float* dbias; float* dlogit_scale;
  void* bwd_ws; size_t bwd_ws_bytes;
  /* Windows of more than 64 tokens (384 px / window 24: n = 576), or any window when bias == NULL: the position bias is
   * looked up per score in bias_table [(2w-1)^2, H] = 16*sigmoid(CPB MLP) (klab_swin_cpb_table) instead of a dense
   * [H, n, n] tensor (21 MB per block at n = 576, H = 16); backward accumulates d(bias_table) into dbias_table
   * [(2w-1)^2, H] (zeroed by the caller).  These shapes run tiled kernels (keys streamed in blocks of 64, LDS use
   * independent of n); lse / dlogit_scale / dqkv as above.                                                         */
  const float* bias_table; float* dbias_table;
  /* Window padding (R % w != 0, HF/swinv2:645-650, 688-690): the token grid is padded to ceil(R/w)*w with zero input rows that
   * still act as keys -- k = 0, v = v_bias [C] (the value Linear's bias, NULL = 0) -- and are cropped from the output; their
   * d v is added to dv_bias [C] (optional).  Padded shapes always run the tiled / streaming kernels; lse then has
   * B * ceil(R/w)^2 * H * w*w entries.                                                                              */
  const float* v_bias; float* dv_bias;
} klab_swin_attn_args;
int klab_swin_attn_fwd(const klab_swin_attn_args* a, void* stream);
/* scratch bytes the matrix-core backward needs for this shape (0: shape outside its envelope) */
size_t klab_swin_attn_bwd_ws_bytes(int dtype, int B, int R, int w, int H, int C);
/* Frozen tower (forward only): the q|k|v projection fused into the window attention, HF/swinv2:389-455 in one kernel.
 * x [B*R*R, C] (the block's LN'd input), wqkv [3C, C] rows q|k|v, bqkv [3C] f32 (k part zero) or NULL, ctx [B*R*R, C].
 * bf16, head dim 32, C in {64, 128, 256}, w*w <= 64; otherwise KLAB_ERR_UNSUPPORTED (caller: klab_gemm + klab_swin_attn_fwd). */
int klab_swin_qkv_attn_fused(const void* x, const void* wqkv, const float* bqkv, void* ctx, const float* bias, const float* logit_scale,
                             int dtype, int B, int R, int w, int shift, int H, int C, void* stream);
/* The same kernel on a pre-arranged bias image (built once per weight version from the dense bias [H, n, n] of klab_swin_cpb_bias):
 * image [classes, H, 4, 64, 16] f32 -- query tile qt, lane, then (t, r) t-major, the order in which the score MFMA's lane holds
 * query qt*16 + (lane & 15) x key t*16 + (lane >> 4)*4 + r.  Value: bias[h][min(q, n-1)][min(key, n-1)], -200 added where the shift
 * regions of q and key differ, -inf where key >= n.  classes = 4 with shift > 0 (2 * (window in the last window row) + (window in
 * the last window column)), else 1.  klab_swin_qkv_attn_fused_img takes the image in place of bias; ctx is bit-identical.      */
size_t klab_swin_bias_image_bytes(int w, int shift, int H);
int klab_swin_bias_image(const float* bias, float* image, int R, int w, int shift, int H, void* stream);
int klab_swin_qkv_attn_fused_img(const void* x, const void* wqkv, const float* bqkv, void* ctx, const float* image, const float* logit_scale,
                                 int dtype, int B, int R, int w, int shift, int H, int C, void* stream);
int klab_swin_attn_bwd(const klab_swin_attn_args* a, void* stream);
/* continuous position bias (HF/swinv2:376-378,418-428): coords [(2w-1)^2,2], index [n*n] are the
 * input-independent buffers of HF/swinv2:457-492; table [(2w-1)^2,H] and hidden [(2w-1)^2,512]
 * (optional, for backward) are scratch/outputs.                                                 */
int klab_swin_cpb_bias(const float* coords, const int* index, const float* w0, const float* b0, const float* w2,
                       float* table, float* hidden, float* bias, int ntab, int n, int heads, int nhidden, void* stream);
/* table form for large windows: table [(2w-1)^2, H] (raw MLP output), hidden (optional), bias_table = 16*sigmoid(table);
 * backward: d(bias_table) -> MLP weight gradients (accumulated: dw0 [512,2], db0 [512], dw2 [H,512]); dtable is scratch
 * [(2w-1)^2, H]; any table size, H <= 64.                                                                         */
int klab_swin_cpb_table(const float* coords, const float* w0, const float* b0, const float* w2, float* table, float* hidden,
                        float* bias_table, int ntab, int heads, int nhidden, void* stream);
int klab_swin_cpb_table_bwd(const float* dbias_table, const float* bias_table, const float* coords, const float* hidden, const float* w2,
                            float* dtable, float* dw0, float* db0, float* dw2, int ntab, int heads, int nhidden, void* stream);

/* ---- input pipeline ---------------------------------------------------------
 * Replaces, for a batch of decoded RGB images, `Image.resize((256,256))` + `ToTensor()` (ref/modules/loader.py:15-16; Pillow
 * ImagingResample, default BICUBIC) and `image_processor(images, return_tensors="pt")` (ref/train.py:55; ViTImageProcessor,
 * HF/vitproc:20-27: Pillow BILINEAR to 224x224, rescale, normalise).  Every intermediate uint8 image is bit-identical to
 * Pillow's (22-bit fixed-point weights from the same double-precision evaluation).
 *   src: device bytes holding the images as HWC uint8 RGB; desc_dev[i] = {byte offset into src, height, width} (device).
 *   filter_a / filter_b: PIL resampling ids of the two resizes (2 = BILINEAR, 3 = BICUBIC); filter_a = 0: src already is
 *   the loader's [n, mid, mid, 3] uint8 batch (desc_dev / ws unused) and only the processor's part runs.
 *   pixel_values [n, 3, out, out] f32 = (u8 * rescale - mean[c]) / std[c]; the reference's effective rescale is 1/255/255
 *   (its processor divides the ToTensor output by 255 a second time).  mean3 / std3 are host pointers to 3 floats.
 *   KLAB_ERR_UNSUPPORTED: other filters, or a size ratio whose weight table exceeds the LDS budget.                        */
typedef struct klab_image_desc { long long offset; int height, width; } klab_image_desc;
size_t klab_image_preprocess_ws_bytes(int n_images, int max_h, int mid);
int klab_image_preprocess(const unsigned char* src, const klab_image_desc* desc_dev, int n_images, int max_h, int max_w, int mid,
                          int out_size, int filter_a, int filter_b, double rescale, const float* mean3, const float* std3,
                          float* pixel_values, void* ws, size_t ws_bytes, void* stream);
/* The same pipeline on a sub-rectangle of every image, mirrored left-right where asked: train-time random-resized-crop + flip.
 * Image i gives exactly `im.crop((left, top, left + w, top + h)).resize((mid, mid), filter_a)`, then
 * `.transpose(FLIP_LEFT_RIGHT)` when bit 0 of `flags` is set, then the processor's part as above.  Crop, THEN resize: the filter
 * taps are clamped at the crop's edges (Pillow's `resize(box=...)` reads outside the box and gives other bytes).  No pixel is
 * copied for the crop and the launches are the three of `klab_image_preprocess`:
 *   offset: byte offset in `src` of the crop's first pixel = image offset + (top * pitch + left) * 3;  height, width: the crop's;
 *   pitch: pixels from one source row to the next (the image's width).  The caller keeps the crop inside its image.
 *   max_crop_h / max_crop_w: the largest crop of the batch; they size the workspace (`klab_image_preprocess_ws_bytes(n,
 *   max_crop_h, mid)`), the grid and the weight tables, so an image too wide for the un-cropped call is taken with a crop that
 *   fits.  filter_a must be 2 or 3.                                                                                           */
#define KLAB_IMAGE_FLIP_LR 1
typedef struct klab_image_crop_desc { long long offset; int height, width, pitch, flags; } klab_image_crop_desc;
int klab_image_preprocess_crop(const unsigned char* src, const klab_image_crop_desc* desc_dev, int n_images, int max_crop_h,
                               int max_crop_w, int mid, int out_size, int filter_a, int filter_b, double rescale, const float* mean3,
                               const float* std3, float* pixel_values, void* ws, size_t ws_bytes, void* stream);

/* ---- JPEG decoding (row f-1: `Image.open(path).convert('RGB')`, ref/modules/loader.py:15) -------------------------------
 * Hybrid decoder for baseline / extended-sequential / progressive 8-bit Huffman JPEG (SOF0 / SOF1 / SOF2; grey, or three
 * components with 4:4:4, 4:2:2 or 4:2:0 sampling; restart intervals; sequential files: one interleaved scan).  The serial part -- marker parsing and Huffman
 * decoding -- runs on the host (`klab_jpeg_entropy_decode*`, threaded over the images of a batch) and yields quantised DCT
 * coefficients; dequantisation, the inverse DCT, chroma upsampling and the colour transform run on the GPU
 * (`klab_jpeg_decode_device`) and write HWC uint8 RGB at the offsets `klab_image_preprocess` reads.  Output is bit-identical to
 * Pillow's decode (libjpeg-turbo defaults: integer "islow" IDCT, triangle-filter upsampling, 16-bit colour tables).
 * Arithmetic-coded / lossless / 12-bit / CMYK / multi-scan sequential files: KLAB_ERR_UNSUPPORTED (`supported` = 0 in klab_jpeg_info).
 *   coefs:  int16, 64 per block in natural (row-major) order; per image the blocks of component 0, then 1, then 2, each as
 *           [bh][bw] over the MCU-padded block grid; qt: uint16 [3][64] per image (natural order, one table per component).   */
#define KLAB_JPEG_GRAY 0
#define KLAB_JPEG_YCC 1
#define KLAB_JPEG_RGB 2
typedef struct klab_jpeg_info {
  int width, height, ncomp, precision, progressive, supported, colour;
  int hmax, vmax, mcus_x, mcus_y;
  int hs[3], vs[3], bw[3], bh[3], tq[3];
  long long coef_blocks; /* sum of bw*bh over the components */
} klab_jpeg_info;
typedef struct klab_jpeg_item { klab_jpeg_info info; long long coef_block0; long long rgb_off; } klab_jpeg_item;
int klab_jpeg_read_info(const unsigned char* data, size_t n, klab_jpeg_info* info);                       /* host, header only */
int klab_jpeg_entropy_decode(const unsigned char* data, size_t n, short* coefs, unsigned short* qt, klab_jpeg_info* info); /* host */
/* host, n_threads workers; coefs[i] -> room for infos[i].coef_blocks*64 shorts; qt: [n][3][64]; rcs[i]: per-image status      */
int klab_jpeg_entropy_decode_batch(const unsigned char* const* data, const size_t* sizes, int n, short* const* coefs,
                                   unsigned short* qt, klab_jpeg_info* infos, int* rcs, int n_threads);
/* device: items (host copy, validated and used to size the grids) / items_dev (the same bytes on the device): per image the
 * header info, the first coefficient block in coefs_dev and the byte offset of its RGB image in rgb_dev                        */
size_t klab_jpeg_decode_ws_bytes(const klab_jpeg_item* items, int n);
int klab_jpeg_decode_device(const short* coefs_dev, const unsigned short* qt_dev, const klab_jpeg_item* items,
                            const klab_jpeg_item* items_dev, int n, unsigned char* rgb_dev, void* ws, size_t ws_bytes, void* stream);

/* ---- glue --------------------------------------------------------------------------------- */
/* multi-tensor f32 -> dtype cast into one arena; desc_dev: device array of
 * {const float* src; long dst_off; long n4_prefix} (prefix sums of element counts / 4)           */
int klab_cast_pack(const void* desc_dev, int ndesc, long total4, void* dst, int dtype, void* stream);
/* embedding gather with optional T5 _shift_right (HF/t5:618-637) and input dropout (HF/t5:725)  */
int klab_embed_fwd(const long long* ids, int shift_right, int L, int start_id, int pad_id, const float* table, int vocab,
                   float* out, int rows, int d, float drop_p, const uint32_t* seed_dev, uint32_t tag, int* err_flag,
                   void* stream);
int klab_embed_bwd(const long long* ids, int shift_right, int L, int start_id, int pad_id, const float* dh, float* dtable,
                   int vocab, int rows, int d, float drop_p, const uint32_t* seed_dev, uint32_t tag, void* stream);
/* relative position bias gather / scatter (HF/t5:264-279); bucket[Lq*Lk] int32 from the host     */
int klab_relbias_fwd(const float* table, const int* bucket, float* bias, int heads, int Lq, int Lk, void* stream);
int klab_relbias_bwd(const float* dbias, const int* bucket, float* dtable, int heads, int Lq, int Lk, int nbuckets,
                     void* stream);
/* cross-entropy over logits [rows, V] (HF/t5:1050-1054); with write_grad (bit 0) the logits are replaced in
 * place by d loss / d logits = (softmax - onehot) / n_valid.  loss_row [rows], inv_n [1], loss [1].
 * write_grad bit 1: inv_n was already produced by klab_ce_count for the same labels (saves the counting launch). */
int klab_ce_count(const long long* labels, int rows, float* inv_n, void* stream);
int klab_ce_fwd(void* logits, long ld, int dtype, const long long* labels, int rows, int V, float* inv_n, float* loss_row,
                float* loss, int write_grad, void* stream);
/* the same with options (csrc/ce.hip): label smoothing eps in [0, 1), z-loss z >= 0 and per-row weights (f32 [rows], finite,
 * >= 0, NULL = all ones):
 *   l_i = lse - (1 - eps) x_y - (eps / V) sum_j x_j + z lse^2 (0 where the label is -100), loss = sum_i w_i l_i / W with
 *   W = sum of w_i over the rows with a label (loss 0 when W == 0), d l / d x_j = (w_i / W) [p_j (1 + 2 z lse) - (1 - eps) [j == y] - eps / V].
 * loss_row receives the UNWEIGHTED l_i; a row with w_i == 0 or without a label gets a gradient of exact zeros.
 * klab_ce_wsum writes inv_w[0] = 1 / W (0 when W == 0) in a fixed order; write_grad as klab_ce_fwd (bit 1: inv_w is already filled).
 * With eps = 0, z = 0 and weights NULL or all ones every output equals klab_ce_fwd's bit for bit. */
int klab_ce_wsum(const long long* labels, const float* weights, int rows, float* inv_w, void* stream);
int klab_ce_fwd_opts(void* logits, long ld, int dtype, const long long* labels, const float* weights, int rows, int V, float eps, float z,
                     float* inv_w, float* loss_row, float* loss, int write_grad, void* stream);
/* the same mixed with knowledge distillation (csrc/ce.hip): teacher logits t [rows, V] (bf16 or f32 whatever the student's
 * dtype, row stride ldt >= V, FINITE -- a precondition, not checked on the device), temperature T > 0, alpha in [0, 1]:
 *   kl_i = KL(softmax(t / T) || softmax(x / T)),  l_i = (1 - alpha) ce_i + alpha T^2 kl_i with ce_i the l_i above (0 where the label is -100),
 *   d l / d x_j = (w_i / W) [(1 - alpha) (the bracket above) + alpha T (softmax(x / T)_j - softmax(t / T)_j)].
 * loss_row receives the unweighted l_i, kl_row the unweighted kl_i (without alpha T^2; 0 where the label is -100).  The teacher is only
 * read; a teacher range that overlaps the logits range, alpha outside [0, 1] or T not finite and > 0 return KLAB_ERR_BADARG, a width or
 * stride off either dtype's 16-byte vector KLAB_ERR_UNSUPPORTED, before anything is launched.  inv_w, write_grad and the launch count are
 * klab_ce_fwd_opts'; no float atomics, the same bits on every run.  With alpha == 0 logits, inv_w, loss_row and loss equal
 * klab_ce_fwd_opts' bit for bit. */
int klab_ce_fwd_distill(void* logits, long ld, int dtype, const void* teacher, long ldt, int t_dtype, const long long* labels,
                        const float* weights, int rows, int V, float eps, float z, float alpha, float temperature, float* inv_w,
                        float* loss_row, float* kl_row, float* loss, int write_grad, void* stream);
int klab_im2col_patch(const float* pixels, void* out, int dtype, int B, int Cin, int Himg, int P, void* stream);
/* same, rows of `ldo` >= Cin*P*P elements with the tail columns zero-filled (lets the patch-embedding GEMM run with K
 * padded to a multiple of 32); P == 4 takes a one-thread-per-patch vector path */
int klab_im2col_patch_ld(const float* pixels, void* out, int dtype, int B, int Cin, int Himg, int P, int ldo, void* stream);
int klab_merge_gather(const float* x, void* out, int dtype, int B, int R, int C, void* stream);
int klab_merge_scatter(const float* dmerged, float* dx, int B, int R, int C, void* stream);
int klab_colsum(const void* dy, long ld, int dtype, int M, int N, float* out, void* stream);
int klab_convert(const float* x, void* y, int dtype, long n, float scale, void* stream);
int klab_add_f32(float* y, const float* x, long n, void* stream);

int klab_gelu_fwd(const void* x, void* y, int dtype, long n, void* stream);
/* Gate of the T5 v1.1 feed-forward (HF T5DenseGatedActDense): ab [M, 2F] row-major with leading dimension ldab holds the two
 * pre-activations side by side, a = ab[:, :F] (wi_0 x) and b = ab[:, F:] (wi_1 x).
 *   forward : h[M,F] = dropout(gelu_new(a) * b), mask = keep(seed_dev, tag, m * F + f), scale 1/(1-p)
 *   backward: dab[:, :F] = dh * mask/(1-p) * b * gelu_new'(a),  dab[:, F:] = dh * mask/(1-p) * gelu_new(a)   (the mask is regenerated)
 * gelu_new is the tanh approximation.  Every matrix in `dtype` (f32 | bf16), arithmetic in f32.  F % 8 == 0, ld* % 8 == 0. */
int klab_geglu_fwd(const void* ab, long ldab, void* h, long ldh, int dtype, int M, int F, float drop_p, const uint32_t* seed_dev,
                   uint32_t drop_tag, void* stream);
int klab_geglu_bwd(const void* dh, long lddh, const void* ab, long ldab, void* dab, long lddab, int dtype, int M, int F, float drop_p,
                   const uint32_t* seed_dev, uint32_t drop_tag, void* stream);
/* Frozen-tower (forward-only) fusion of the MLP half of a Swin-V2 block, HF/swinv2:539-563 + 697-702:
 *   out[M,C] = shortcut + LayerNorm(fc2(GELU(fc1(x) + b1)) + b2) * gamma + beta,  outt = bf16(out) (optional)
 * x [M,C], w1 [4C,C], w2 [C,4C] in `dtype` (bf16 only), everything else f32.  C in {64, 128}; other widths return
 * KLAB_ERR_UNSUPPORTED and the caller keeps the three-kernel path (klab_gemm x2 + klab_layernorm_fwd). */
/* ... and of the attention half's tail, HF/swinv2:496-506 + 697-700: out = shortcut + LayerNorm(x Wp^T + bp) * gamma + beta */
int klab_swin_proj_ln_fused(const void* x, const float* shortcut, const void* w, const float* b, const float* gamma, const float* beta,
                            float* out, void* outt, int dtype, int M, int C, float eps, void* stream);
int klab_swin_mlp_fused(const void* x, const float* shortcut, const void* w1, const float* b1, const void* w2, const float* b2,
                        const float* gamma, const float* beta, float* out, void* outt, int dtype, int M, int C, float eps,
                        void* stream);
/* Frozen-tower fusion of the patch embedding, HF/swinv2:234-259, 281, 293-302: out = LayerNorm(Conv2d(3 -> C, k 4, s 4)(pixels)) in one
 * launch (no column matrix, no stored GEMM output).  w: bf16 [C, ldw >= 64], columns 48..63 zero (the Conv2d weight [C,3,4,4] flattened
 * and zero-padded); out [B*(image_size/4)^2, C] f32, outt the same in bf16 (optional).  bf16, patch 4, 3 channels, C in {64, 96, 128};
 * otherwise KLAB_ERR_UNSUPPORTED (caller: klab_im2col_patch_ld + klab_gemm + klab_layernorm_fwd).                                 */
int klab_swin_patch_embed_fused(const float* pixels, const void* w, int ldw, const float* bias, const float* gamma, const float* beta,
                                float* out, void* outt, int dtype, int B, int in_ch, int image_size, int patch, int C, float eps, void* stream);
/* Frozen-tower fusion for the WIDE stages, HF/swinv2:496-506 / 555-563 + 697-702: out = shortcut + LayerNorm(x W^T + b) * gamma + beta in
 * one launch, for the attention output projection (K = C) and the MLP's second Linear (K = 4C).  x [M, K], w [C, K] in `dtype` (bf16
 * only), the rest f32; out [M, C] f32, outt its bf16 copy (optional).  C == 256, K % 32 == 0, K >= 128; otherwise
 * KLAB_ERR_UNSUPPORTED (caller: klab_gemm + klab_layernorm_fwd).                                                                    */
int klab_swin_linear_ln_fused(const void* x, const float* shortcut, const void* w, const float* bias, const float* gamma,
                              const float* beta, float* out, void* outt, int dtype, int M, int K, int C, float eps, void* stream);
int klab_swin_cpb_bias_bwd(const float* dbias, const float* bias, const int* index, const float* coords, const float* hidden,
                           const float* w0, const float* w2, float* dtable, float* dw0, float* db0, float* dw2, int ntab, int n,
                           int heads, int nhidden, void* stream);
/* the same with `dtable_zeroed`: non-zero = the caller has cleared dtable[ntab * heads] (the engine clears every block's slice in one fill) */
int klab_swin_cpb_bias_bwd_pz(const float* dbias, const float* bias, const int* index, const float* coords, const float* hidden,
                              const float* w0, const float* w2, float* dtable, float* dw0, float* db0, float* dw2, int ntab, int n,
                              int heads, int nhidden, int dtable_zeroed, void* stream);

/* ==== the whole path: MyModel.forward + backward (ref/models/model.py:19-26, ref/train.py:58-62) ====
 * The engine is a host-side plan over the kernels above.  It owns no device memory: parameters are
 * the caller's fp32 tensors (named exactly like the HuggingFace state dict), activations
 * live in one caller-provided workspace, gradients are written into caller-provided flat f32 buffers
 * at the offsets published by klab_engine_param_info.  model index: 0 = Swin-V2 image_model,
 * 1 = frozen language_model (T5 encoder), 2 = transformer (T5ForConditionalGeneration).            */
typedef struct klab_swin_cfg {  /* HF/swinv2cfg:56-73 */
  int image_size, patch, in_ch, embed_dim, n_stages;
  int depths[8], heads[8];
  int window;
  int pretrained_window[8];
  int mlp_ratio, qkv_bias;
  float ln_eps;
} klab_swin_cfg;
typedef struct klab_t5_cfg {    /* HF/t5cfg:44-62,82-83 */
  int vocab, d_model, d_kv, n_heads, d_ff, n_layers, n_dec_layers, rel_buckets, rel_max_dist;
  float dropout, ln_eps;
  int start_id, pad_id, scale_decoder_outputs;
  int ffn_gated;   /* 0: wo(relu(wi x)) (T5 v1.0); 1: wo(gelu_new(wi_0 x) * (wi_1 x)) (T5 v1.1 / Flan-T5, HF T5DenseGatedActDense) */
  int tie_lm_head; /* 1: the LM head is shared.weight (v1.0); 0: lm_head.weight is a parameter of its own */
} klab_t5_cfg;
typedef struct klab_model_cfg {
  klab_swin_cfg swin;
  klab_t5_cfg lang, main;
  int dtype;      /* KLAB_F32 parity mode | KLAB_BF16 | KLAB_FP8 (bf16 + fp8 forward GEMMs with per-row scales) */
  int train_swin; /* args.image_model_train (ref/models/model.py:15) */
} klab_model_cfg;
typedef struct klab_engine klab_engine;

int klab_sizeof_t5_cfg(void);    /* sizeof(klab_t5_cfg) / sizeof(klab_model_cfg): the ctypes mirrors are checked against them */
int klab_sizeof_model_cfg(void);
int klab_sizeof_sample_args(void); /* likewise klab_sample_args, klab_logits_proc_args, klab_gen_cfg, klab_constrain_args (below) */
int klab_sizeof_logits_proc_args(void);
int klab_sizeof_gen_cfg(void);
klab_engine* klab_engine_create(const klab_model_cfg* cfg); /* NULL on an invalid config (e.g. Swin width != d_model:
                                                               the reference raises at its torch.cat, model.py:23) */
void klab_engine_destroy(klab_engine* e);
int klab_engine_num_params(const klab_engine* e, int model);
int klab_engine_param_info(const klab_engine* e, int model, int i, char* name, int name_cap, long* shape4, int* ndim,
                           long* grad_off /* element offset in the model's flat grad buffer, -1 = frozen */);
long klab_engine_grad_elems(const klab_engine* e, int model);
/* backward segment -> (model, offset, length) of the flat-grad slice that is final when it returns */
/* Gradient buckets INSIDE a backward segment (data parallelism, ref/train.py:26,62: DDP reduces buckets as they become
 * ready).  Bucket i of a segment = the GEMM-weight gradients of one T5 layer (segments 0, 1) or one Swin block (segment 2),
 * a contiguous range [off, off+len) of that segment's flat gradient buffer; i counts in the order the backward finishes
 * them (last layer first).  klab_engine_bucket_wait makes `stream` wait until bucket i of the LAST klab_engine_backward of
 * that segment is final (an engine-owned event behind the layer's weight-gradient launch); KLAB_ERR_UNSUPPORTED under graph
 * replay or before any backward.  Everything of the segment outside its buckets is final when klab_engine_backward returns
 * (on the stream passed to it).                                                                                           */
int klab_engine_num_buckets(const klab_engine* e, int segment);
int klab_engine_bucket(const klab_engine* e, int segment, int i, long* off, long* len);
int klab_engine_bucket_wait(klab_engine* e, int segment, int i, void* stream);
/* the per-bucket events are recorded only after klab_engine_set_bucket_events(e, 1) (a data-parallel reducer is attached);
 * off by default: a single-GPU step pays nothing for them                                                            */
int klab_engine_set_bucket_events(klab_engine* e, int on);
int klab_engine_segment(const klab_engine* e, int seg, int* model, long* off, long* len);
/* Captions per image, n >= 1, of the NEXT klab_engine_bind: one-shot, the bind takes it and puts 1 back, so a caller that never
 * sets it binds as before.  klab_engine_workspace_bytes sizes the binding that klab_engine_bind would make now (it reads the value
 * and leaves it); klab_engine_workspace_bytes_n is the plain query for a given n and touches nothing.  The Swin tower, both encoders and the cross K/V of that binding run B rows of images; the decoder, the
 * LM head and the loss run B*n target sequences in image-major order: tgt_ids [B,n,Lt], loss weights [B,n,Lt], loss_row /
 * logits / decoder_out rows ((b*n + j)*Lt + t).  Cross-attention of an image's n sequences is issued as ONE batch element with
 * n*Lt queries over the image's K/V (no position bias, no mask: HF/t5:404-432), so d(encoder output) needs no reduction over n.
 * The loss is the mean over all scored tokens of all sequences.  Decoding sessions (klab_engine_gen_*) need a binding with n = 1. */
int klab_engine_set_captions(klab_engine* e, int n);
size_t klab_engine_workspace_bytes(klab_engine* e, int B, int Ls, int Lt);
size_t klab_engine_workspace_bytes_n(klab_engine* e, int B, int Ls, int Lt, int n);
/* *_params: host arrays of device pointers in klab_engine_param_info order.  *_bucket: int32 device
 * arrays [L*L] of T5 relative-position buckets (HF/t5:216-262, computed by the host exactly as the
 * reference does).  swin_coords[s] / swin_index[s]: per-stage CPB tables (HF/swinv2:457-492).      */
int klab_engine_bind(klab_engine* e, int B, int Ls, int Lt, void* workspace, size_t ws_bytes, const void* const* swin_params,
                     const void* const* lang_params, const void* const* main_params, float* main_grads, float* swin_grads,
                     const int* lang_bucket, const int* enc_bucket, const int* dec_bucket, const void* const* swin_coords,
                     const void* const* swin_index, void* stream);
/* pixels [B,3,H,W] f32, src_ids [B,Ls] / tgt_ids [B,n,Lt] int64 (device).  training: T5 dropout on
 * (model.module.transformer.train(), ref/train.py:52).  `seed` (re)bases the device-side counter RNG whenever
 * it changes; every forward advances the counter itself.  The loss lands in *klab_engine_loss_ptr.      */
int klab_engine_forward(klab_engine* e, const float* pixels, const long long* src_ids, const long long* tgt_ids, int training,
                        uint32_t seed, int want_grad, void* stream);
/* hipGraph replay of the forward / backward launch sequences (first use eager, second captured, then replayed;
 * inputs are staged into engine-owned buffers so node addresses stay fixed).  Off by default.          */
int klab_engine_set_graph(klab_engine* e, int on);
/* dropout RNG state of the binding (base seed, forwards since seeding): saved / restored by a true resume so that the run
 * continues its mask stream.  get synchronises `stream`.                                                                  */
int klab_engine_get_rng(klab_engine* e, uint32_t* base, uint32_t* counter, void* stream);
int klab_engine_set_rng(klab_engine* e, uint32_t base, uint32_t counter, void* stream);
/* torch.optim.Adam's update (ref/train.py:28; no amsgrad, L2 weight decay) for ALL parameters of the
 * trainable T5 in one pass.  m / v: caller-owned f32 state laid out like the "main" flat gradient buffer.  bias_corr{1,2} =
 * 1 - beta^step.  Also refreshes the compute-dtype copies of the GEMM weights, so the next klab_engine_forward may be
 * told (training bit 2) that they are current. */
int klab_engine_adam_step(klab_engine* e, float* m, float* v, float lr, float beta1, float beta2, float eps, float weight_decay,
                          float bias_corr1, float bias_corr2, void* stream);
/* the kernel behind it: desc = device array of {float* p; long grad_off; long arena_off (<0: none); long n4_prefix} */
int klab_adam_step(const void* desc_dev, int ndesc, long total4, const float* grads, float* m, float* v, void* arena, int dtype, float lr,
                   float beta1, float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, void* stream);
/* the same update restricted to the tensors of ONE backward segment (0: decoder + tied embedding, 1: encoder): under data
 * parallelism segment 0 can be updated while segment 1's gradient all-reduce is still in flight.  Both segments = one full step. */
int klab_engine_adam_step_segment(klab_engine* e, int segment, float* m, float* v, float lr, float beta1, float beta2, float eps,
                                  float weight_decay, float bias_corr1, float bias_corr2, void* stream);
/* vec4 range [begin4, end4) of the descriptor table's prefix space */
int klab_adam_step_range(const void* desc_dev, int ndesc, long begin4, long end4, const float* grads, float* m, float* v, void* arena,
                         int dtype, float lr, float beta1, float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                         void* stream);
/* AdamW (torch.optim.AdamW's single-tensor rule, decoupled decay, no amsgrad / maximize) over the same descriptor table, with the
 * hyper-parameters of up to KLAB_ADAMW_MAX_GROUPS parameter groups in ONE launch (csrc/adamw.hip).  group_of_dev: device array of
 * ndesc ints in table order, the group (0 <= id < ngroups) of each tensor; it belongs to the caller.  groups: HOST array, read
 * before the call returns and passed to the kernel by value -- no copy to the device, nothing read back.  bias_corr{1,2} =
 * 1 - beta^step > 0.  Per element, in f32:
 *   p' = p * decay;  m' = m + (1 - beta1) (g - m);  v' = beta2 v + (1 - beta2) g^2;
 *   p'' = p' - step * (m' / (sqrt(v') * inv_sqrt_bc2 + eps));  arena copy = (dtype) p''
 * with  decay = (float)(1.0 - (double)lr * (double)weight_decay)  and  step = (float)((double)lr / bias_corr1)  formed on the host
 * from the f32 fields below, inv_sqrt_bc2 = 1.f / sqrtf(bias_corr2).  lr = 0 leaves p bit-identical.  [begin4, end4): vec4 range of
 * the table's prefix space, as klab_adam_step_range.  ngroups < 1 or > KLAB_ADAMW_MAX_GROUPS: KLAB_ERR_UNSUPPORTED, nothing is
 * launched. */
#define KLAB_ADAMW_MAX_GROUPS 16
typedef struct { float lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2; } klab_adamw_group;
int klab_adamw_step_range(const void* desc_dev, int ndesc, const int* group_of_dev, const klab_adamw_group* groups /*host*/, int ngroups,
                          long begin4, long end4, const float* grads, float* m, float* v, void* arena, int dtype, void* stream);
/* table order of the fused optimizers (klab_engine_adam_step, klab_engine_adamw_step): param_ptrs[i] = the master tensor of table
 * entry i, *n_segment0 = how many leading entries belong to backward segment 0.  Returns the number of entries (> 0), or
 * KLAB_ERR_BADARG when max_n is smaller, KLAB_ERR_UNSUPPORTED when the table is unusable.  Host data only: no synchronisation. */
int klab_engine_adam_layout(klab_engine* e, int max_n, long* param_ptrs, int* n_segment0);
/* klab_adamw_step_range on the engine's table, gradients and weight arena: segment -1 = every tensor, 0 / 1 = the tensors of that
 * backward segment (both = one full step).  Refreshes the compute-dtype copies like klab_engine_adam_step.  The group table is
 * the caller's and survives a re-bind to another batch shape (same tensors, same order).  KLAB_ERR_UNSUPPORTED when the Adam
 * table is unusable. */
int klab_engine_adamw_step(klab_engine* e, int segment /* -1 both, 0, 1 */, float* m, float* v, const int* group_of_dev,
                           const klab_adamw_group* groups, int ngroups, void* stream);
/* Exponential moving average of the weights over the same descriptor table, one launch each whatever the number of tensors
 * (csrc/ema.hip).  ema: caller-owned f32 buffer laid out like the "main" flat gradient buffer, indexed by grad_off exactly as m
 * and v are.  [begin4, end4): vec4 range of the table's prefix space, as klab_adam_step_range; all tensor lengths are multiples
 * of 4.  No floating-point atomics, nothing read back.
 *   update  per element, in f32:  e' = e + w (p - e)  (may contract to an FMA).  w is a HOST scalar passed by value, 0 <= w <= 1
 *           (the caller forms (float)(1.0 - decay) in double).  p is only read and no arena is touched: 12 bytes per parameter.
 *   swap    p and e exchange their bits -- moved, not computed: NaN payloads, -0, infinities and denormals survive -- and, for
 *           tensors with arena_off >= 0, arena copy = (dtype) new p (round-to-nearest-even bf16, or the f32 bits).  Two swaps
 *           restore p and ema bit for bit.  16 bytes per parameter + 2 for a bf16 copy.
 * KLAB_ERR_BADARG: w outside [0, 1] or NaN, a null pointer, ndesc <= 0, begin4 < 0, end4 < begin4, dtype neither KLAB_BF16 nor
 * KLAB_F32; nothing is launched.  end4 == begin4: KLAB_OK without a launch. */
int klab_ema_update_range(const void* desc_dev, int ndesc, long begin4, long end4, float* ema, float w, void* stream);
int klab_ema_swap_range(const void* desc_dev, int ndesc, long begin4, long end4, float* ema, void* arena, int dtype, void* stream);
/* the two on the engine's table, the whole range, its weight arena and compute dtype: after klab_engine_ema_swap the compute-dtype
 * copies are those of the parameters now in place, as after klab_engine_adam_step.  The ema buffer is the caller's and survives a
 * re-bind to another batch shape (same tensors, same layout).  KLAB_ERR_UNSUPPORTED when the Adam table is unusable,
 * KLAB_ERR_BADARG when the engine is unbound. */
int klab_engine_ema_update(klab_engine* e, float* ema, float w, void* stream);
int klab_engine_ema_swap(klab_engine* e, float* ema, void* stream);
/* LoRA adapters in merged-weight form (csrc/lora.hip).  desc_dev: a caller-owned device table of ndesc entries of 11 longs, one per
 * target matrix W [out, in] with lora_A [r, in], lora_B [out, r] and s = alpha / r:
 *   {W, A, B (f32 device pointers, 16-byte aligned), arena_off, grad_off (elements), out | in << 32, r | bits(s) << 32,
 *    n4_prefix (exclusive prefix sum of r * in / 4), rb_prefix (exclusive prefix sum of ceil(out / klab_lora_row_block())),
 *    slab_off (element offset of the tensor's [row blocks, r, in] dA partials in the slab), db_off}
 * in % 4 == 0, 1 <= r <= 64.  One launch whatever the number of tensors (klab_lora_grads: two); f32 FMAs only, no floating-point
 * atomics, the same bits on every run.  ndesc == 0: KLAB_OK without a launch; ndesc > 1024: KLAB_ERR_UNSUPPORTED.
 *   merge   arena[arena_off + i * in + j] = (dtype)(W[i,j] + s * sum_k B[i,k] A[k,j]): W from the f32 master, products and sums in
 *           f32 (at most r + 1 roundings), one rounding into the arena type (KLAB_BF16: nearest-even; KLAB_F32: the bits).
 *           to_master != 0: the same f32 value goes into W itself and no arena is touched (arena and dtype are ignored).
 *           A, B (and W, unless to_master) are only read.
 *   grads   dB[i,k] = s * sum_j dW[i,j] A[k,j] and dA[k,j] = s * sum_i B[i,k] dW[i,j], dW = grads + grad_off in W's own layout, read
 *           once.  dA of entry t is stored at out[4 * n4_prefix], dB at out[db_off]; both are overwritten, never added to.  slab:
 *           caller-owned f32 scratch; only the tensors' [row blocks, r, in] ranges are written. */
int klab_lora_merge(const void* desc_dev, int ndesc, void* arena, int dtype, int to_master, void* stream);
int klab_lora_grads(const void* desc_dev, int ndesc, const float* grads, float* out, float* slab, void* stream);
int klab_lora_row_block(void);
/* the engine's side of the table: out[2 i] = arena_off and out[2 i + 1] = grad_off of parameter i of the trainable T5 (parameter
 * table order; -1: none).  Fixed by the configuration: valid before and across klab_engine_bind.  Returns the number of parameters,
 * or KLAB_ERR_BADARG when max_n is smaller. */
int klab_engine_lora_layout(klab_engine* e, int max_n, long* out);
/* Registers (ndesc > 0) or clears (ndesc == 0) the adapter table.  While one is registered, every forward that casts the
 * trainable weights into the arena runs klab_lora_merge right behind that cast (captured graphs contain it and read the live A,
 * B and s on replay).  The registration survives klab_engine_bind; captured graphs are dropped.  With no table registered every call
 * issues exactly the launches it issued before.  KLAB_ERR_UNSUPPORTED: ndesc > 1024, or an fp8 engine. */
int klab_engine_lora_set(klab_engine* e, const void* desc_dev, int ndesc);
/* klab_lora_grads on the registered table and the engine's flat gradient buffer, on the caller's stream behind
 * klab_engine_backward of segments 0 and 1 (each returns with its side-stream weight gradients joined, as
 * klab_engine_adam_step relies on).  KLAB_ERR_UNSUPPORTED when no table is registered. */
int klab_engine_lora_grads(klab_engine* e, float* out, float* slab, void* stream);
/* Adafactor (the rule of transformers.optimization.Adafactor) for ALL parameters of the trainable T5 in four launches, whatever
 * the number of tensors: statistics (row / column sums of g^2 + eps0, sum p^2), their reduction (EMA into R / C, mean R, RMS(p)),
 * sum u^2, apply.  Tensors with >= 2 dims are factored (rows = product of all dims but the last), 1-D tensors keep a full second
 * moment.  No floating-point atomics: a step is bit-reproducible.  No host read: beta2t = 1 - t^decay_rate, one_minus_beta2t and
 * rel_step (min(1e-2 or 1e-6 t, 1/sqrt t), or lr) are host scalars; lr_t = rel_step * max(eps1, RMS(p)) (scale_parameter) and the
 * clip factor max(1, RMS(u) / clip_threshold) are computed on the device.  Like klab_engine_adam_step it also refreshes the
 * compute-dtype copies of the GEMM weights.  Caller-owned f32 buffers, sized by klab_engine_adafactor_state_elems:
 *   state    R | C (each padded to 4 elements) per factored tensor, V per 1-D tensor; zero before the first step
 *   m        first moment laid out like the "main" flat gradient buffer, or NULL (beta1 is then ignored); one_minus_beta1 is
 *            1 - beta1 formed in double by the caller, as one_minus_beta2t is (1.f - 0.9f is 2e-7 away from 0.1)
 *   scalars  4 per tensor: mean(R), RMS(p) before the update, RMS(u), unused
 *   scratch  the factors rsqrt(R / mean R) | rsqrt(C), per-tile partial sums and per-tile column sums
 * KLAB_ERR_UNSUPPORTED where the Adam table is unusable, for rows wider than 8192 (2048 when not a multiple of 4) and for
 * tensors of 2^31 elements or more. */
int klab_engine_adafactor_state_elems(klab_engine* e, long* state_elems, long* scalar_elems, long* scratch_elems);
int klab_engine_adafactor_step(klab_engine* e, float* state, float* m, float* scalars, float* scratch, float beta2t, float one_minus_beta2t,
                               float eps0, float eps1, float rel_step, float clip_threshold, float beta1, float one_minus_beta1,
                               float weight_decay, int scale_parameter, void* stream);
/* the engine's descriptor table copied to the host (10 longs per tensor, below), in the order of the flat-gradient views of
 * segment 0 then segment 1: where each tensor's R | C | V lives in `state`.  Returns the number of tensors (> 0) or an error;
 * synchronises. */
int klab_engine_adafactor_layout(klab_engine* e, int max_n, long* out);
/* the kernels behind it.  desc = device array of {float* p; long grad_off; long arena_off (<0: none); long rows; long cols;
 * long state_off; long tile0; long tile_len; long part_off; long factored}; klab_adafactor_plan fills, for n tensors of
 * (rows, cols, factored), out[4 i ..] = {state_off, tile0, tile_len, part_off} and totals = {state elems, tiles, scratch
 * elems, scalar elems}.  rows is ignored (1) for an unfactored tensor, whose length is cols. */
int klab_adafactor_plan(int n, const long* rows, const long* cols, const int* factored, long* out, long* totals);
int klab_adafactor_step(const void* desc_dev, int ndesc, long state_elems, long ntiles, const float* grads, float* state, float* m,
                        float* scalars, float* scratch, void* arena, int dtype, float beta2t, float one_minus_beta2t, float eps0, float eps1,
                        float rel_step, float clip_threshold, float beta1, float one_minus_beta1, float weight_decay, int scale_parameter,
                        void* stream);
/* Gradient-norm clipping (torch.nn.utils.clip_grad_norm_) over ANY set of fp32 gradient tensors of one device.  table = device
 * array of {float* ptr; long n}, one entry per tensor, n >= 1, ptr 4-byte aligned (16-byte aligned tensors are read and written
 * in 16-byte vectors).  Tensor i owns ceil(n_i / chunk) consecutive fp64 partials of `parts`, chunk = klab_grad_norm_chunk().
 * klab_grad_norm (kind 0: L2, squares and sums in fp64; kind 1: max |g|, NaN kept) is two launches: one partial per chunk, then
 * one workgroup that writes norms[i] for i < nt and the total norms[nt] (nt = 0: a total of 0).  No floating-point atomics, a
 * fixed order of summation: the same input gives the same bits on every run.  nparts < nt is a bad argument; the exact count
 * is known to the device only, which never writes past parts[nparts - 1] and gives NaN for a tensor whose partials are cut off.
 * klab_grad_clip is one launch: coef_dev[0] = min(max_norm / (*total_dev + 1e-6f), 1) with NaN kept (torch's clamp), and every
 * element times coef in place -- unless coef >= 1, when nothing is read or written. */
int klab_grad_norm_chunk(void);
int klab_grad_norm(const void* table_dev, int nt, int kind, double* parts, long nparts, float* norms, void* stream);
int klab_grad_clip(const void* table_dev, int nt, const float* total_dev, float max_norm, float* coef_dev, void* stream);
/* decoding over a K/V cache: one query row per (row, head) of R rows against cached keys / values (element strides; bias_row
 * [H, bias_ld] or NULL; scores are unscaled, HF/t5:196-197).  Key j of query row r is read at row  s*kv_bstride + j*ldk  (element
 * offsets from k / v) where s = kv_slot[r*slot_ld + j] when kv_slot (int32 [R, slot_ld]) is given (beam search: the beams' key-slot
 * tables), else s = r / kv_group (kv_group 1: every row its own keys; cross-attention: the kv_group rows of a sample share its
 * encoder K/V).                                                                                                             */
int klab_t5_beam_decode_attn(int dtype, const void* q, long q_bstride, const void* k, const void* v, long kv_bstride, long ldk,
                             int kv_group, const int* kv_slot, long slot_ld, const float* bias_row, long bias_ld, void* ctx,
                             long ctx_bstride, int R, int H, int Lk, int dk, void* stream);
/* the attention probabilities of the same query rows, averaged over the heads (csrc/attn_map.hip; HF's `cross_attentions` with
 * output_attentions=True, head mean): map[r*map_bstride + j] = (1/H) * sum_h softmax_j(q_h . k_{h,j} + bias_row[h, j]), f32, for
 * r < R, j < Lk <= map_bstride.  Row r's query is read at q + (r / q_div)*q_bstride (q_div n: the prefill's one row per sample),
 * its keys as klab_t5_beam_decode_attn reads them without a slot table (sample r / kv_group, key j at j*ldk, head h at column
 * h*dk); V is not read and no context is written.  bias_row [H, bias_ld >= Lk] or NULL; done (int32 [R]) or NULL: a row with
 * done[r] != 0 gets Lk zeros.  dtype bf16 or f32 (arithmetic in f32), dk in {8, 16, 32, 64, 128} (KLAB_ERR_UNSUPPORTED
 * otherwise), any H >= 1, Lk >= 1.  The head sum runs in ascending h in f32 without atomics (bit-reproducible) and the mean is
 * that sum times 1.0f / H.                                                                                                  */
int klab_t5_decode_attn_map(int dtype, const void* q, long q_bstride, int q_div, const void* k, long kv_bstride, long ldk, int kv_group,
                            const float* bias_row, long bias_ld, const int* done, float* map, long map_bstride, int R, int H, int Lk,
                            int dk, void* stream);

/* ---- beam search (HF `_beam_search`, transformers/generation/utils.py; csrc/beam.hip) ------------------------------------
 * klab_beam_topk: per sample b, the 2k best of  log_softmax(logits row b*k+j) + run_score[b*k+j]  over all j < k and tokens,
 * as (score, flat index j*V + token), sorted descending; equal scores rank by the LOWER flat index.  Logits row r is read at
 * logits + (r / row_div) * ld (row_div k: one row per sample, e.g. the prefill's).  row_score / row_idx: scratch [B*k, 2k];
 * out_score / out_idx: [B, 2k].  1 <= k <= 16, V >= 2k.                                                                   */
int klab_beam_topk(int dtype, const void* logits, long ld, int row_div, const float* run_score, int B, int k, int V, float* row_score,
                   int* row_idx, float* out_score, int* out_idx, void* stream);
/* fixed-shape beam state of B samples x k beams, rows r = b*k + j; sequences are [B*k, max_length] int64 (position 0 = the
 * decoder start token).  *_in / *_out are the previous and the next step's buffers (ping-pong); slot_in / slot_out: the key-slot
 * tables of klab_t5_beam_decode_attn (both NULL: none).  early_stopping: 0 False, 1 True, 2 "never".                        */
typedef struct {
  int B, k, V, max_length, eos_id, early_stopping;
  float length_penalty;
  const float* cand_score; const int* cand_idx;         /* [B, 2k] from klab_beam_topk */
  const long long* run_seq_in; long long* run_seq_out;  /* running hypotheses */
  float* run_score;                                     /* [B*k] running scores (HF running_beam_scores) */
  const long long* fin_seq_in; long long* fin_seq_out;  /* finished pool (HF sequences) */
  float* fin_score; int* fin_flag; int* fin_len;        /* [B*k] HF beam_scores, is_sent_finished, generated tokens */
  int* unsat;                                           /* [B] HF is_early_stop_heuristic_unsatisfied */
  const int* slot_in; int* slot_out;                    /* [B*k, max_length] or NULL */
  long long* prev_tokens; int* parent;                  /* [B*k] next decoder input ids; parent row of every new beam */
  int* stop_word;                                       /* [max_length]: bits OR-ed into stop_word[cur_len] */
} klab_beam_update_args;
/* one step of HF's bookkeeping at cur_len (1 <= cur_len < max_length; the candidates' tokens go to position cur_len):
 * running beams, finished pool, early-stop heuristic.  stop_word[cur_len] |= 1 (some sample's heuristic is unsatisfied),
 * 2 (some sample's pool holds an unfinished entry), 4 (some candidate did not hit EOS / max_length).  The search goes on
 * iff bit 1 and bit 4 are set and, with early_stopping True, bit 2.                                                       */
int klab_beam_update(const klab_beam_update_args* a, int cur_len, void* stream);
/* the state before the first update (writes run_seq_in / fin_seq_in = start_id then fill_id, slot_in[r][0] = r, the scores,
 * flags, unsat and every stop word): HF's running_beam_scores 0 / -1e9, beam_scores -1e9, nothing finished               */
int klab_beam_init(const klab_beam_update_args* a, int start_id, int fill_id, void* stream);
/* dst row r = src row r / src_div (elem_bytes 2, 4 or 8; element strides) */
int klab_beam_copy_rows(int elem_bytes, const void* src, long src_ld, int src_div, void* dst, long dst_ld, int rows, int cols,
                        void* stream);

/* ---- sampling (HF `_sample` with temperature -> top-k -> top-p; csrc/sample.hip) ------------------------------------------
 * klab_sample_rows: one drawn token per row r < rows from logits row (r / row_div) (element stride ld), V <= 32768
 * (KLAB_ERR_UNSUPPORTED above).  Scores = fp32 logits / temperature; top_k = 0 or >= V: no top-k, else every score below the
 * k-th largest is removed (ties at it stay); top_p >= 1: no top-p, else token i stays iff the softmax mass of the top-k-kept
 * tokens with a strictly larger score is < top_p (the arg-max always stays; unlike HF's sort-and-cumsum, a tie exactly at the
 * boundary stays whole).  Draw: the smallest kept id j whose running kept probability (ascending id) exceeds u * (kept total);
 * u = u_in[r] when given, else a counter hash of (seed, step, r) in [0, 1).
 * Optional outputs (NULL: not written): warped [rows, ld_warped] f32, the processed scores (-inf = removed); done [rows]: a row
 * with done[r] != 0 draws pad_id, a row that draws eos_id gets done[r] = 1; tokens [rows]: the token; seq: seq[r*ld_seq + pos]
 * = the token (and seq[r*ld_seq] = start_id when pos == 1); stop_word: set to 1 by every row still unfinished (the caller
 * clears it); logprob: logprob[r*ld_logprob + pos] = the token's log-probability under the processed scores, log_softmax(s)[tok]
 * = (s[tok] - M) - logf(G) with the row max M and the kept mass G = sum exp(s - M) the draw used (HF's compute_transition_scores
 * with normalize_logits), 0 for a row with done[r] != 0 on entry.                                                           */
typedef struct {
  int dtype;
  const void* logits; long ld; int row_div;
  int rows, V;
  float temperature; int top_k; float top_p;
  unsigned long long seed; int step;
  const float* u_in;
  float* warped; long ld_warped;
  int* done; int eos_id, pad_id, start_id;
  long long* tokens;
  long long* seq; long ld_seq; int pos;
  int* stop_word;
  float* logprob; long ld_logprob; /* optional: logprob[r*ld_logprob + pos] (pos >= 1, ld_logprob > pos) */
} klab_sample_args;
int klab_sample_rows(const klab_sample_args* a, void* stream);
/* The scores of finished sampling / pick rows from their per-token log-probabilities (csrc/sample.hip): one wave per image b < B
 * over its n <= 64 rows b*n + j (KLAB_ERR_UNSUPPORTED above).  logprob [B*n, ld] f32 and seq [B*n, ld_seq] int64 hold positions
 * 1 .. length - 1 (2 <= length <= ld, ld_seq).  len[r] = the generated tokens through the first eos_id, length - 1 without one (so
 * never 0); score[r] = sum_{p = 1 .. len} logprob[r, p] / powf(len, length_penalty), summed in ascending p in fp32 by one thread
 * (bit-reproducible; beam search's convention); order[b*n_out + i] = the row (b*n + j) of image b's i-th best score, i < n_out <= n,
 * equal scores (two -inf included) in ascending row.  score, len and order are optional (NULL: not written).                 */
int klab_gen_finalize(const float* logprob, long ld, const long long* seq, long ld_seq, int B, int n, int length, int eos_id,
                      float length_penalty, int n_out, float* score, int* len, int* order, void* stream);

/* ---- forced decoding (csrc/force.hip) -----------------------------------------------------------------------------------------
 * klab_force_rows: position pos of every row r < rows is TOLD, not chosen: the token is forced[r*ld_forced + pos] (int64, device;
 * ld_forced > pos), with the bookkeeping of the two choosing kernels: a row with done[r] != 0 on entry gets pad_id; with
 * finish_on_eos != 0 a forced eos_id sets done[r] = 1 (scoring given captions), with 0 it does not (a decoder prompt: HF does
 * not finish a row on an EOS inside its prompt); tokens [rows], seq[r*ld_seq + pos] (and seq[r*ld_seq] = start_id when pos == 1)
 * and stop_word as in klab_sample_rows (done, tokens, seq, stop_word optional).
 * logprob != NULL: logprob[r*ld_logprob + pos] = log_softmax(x)[token] = (x[token] - M) - logf(sum exp(x - M)) over the raw fp32
 * logits row (r / row_div) (element stride ld, dtype bf16 or f32; any V >= 1: no register row, so no 32768 cap), 0 for a row with
 * done[r] != 0 on entry, -inf for a token outside [0, V) (nothing is read for it).  logprob == NULL: logits is not read at all
 * (may be NULL).                                                                                                            */
typedef struct {
  int dtype;
  const void* logits; long ld; int row_div;
  int rows, V;
  const long long* forced; long ld_forced;
  int finish_on_eos;
  int* done; int eos_id, pad_id, start_id;
  long long* tokens;
  long long* seq; long ld_seq; int pos;
  int* stop_word;
  float* logprob; long ld_logprob;
} klab_force_args;
int klab_force_rows(const klab_force_args* a, void* stream);
int klab_sizeof_force_args(void);

/* ---- logits processors (HF's RepetitionPenalty, NoRepeatNGram, NoBadWords, MinLength, MinNewTokensLength, in that order;
 * csrc/logits_proc.hip) --------------------------------------------------------------------------------------------------
 * klab_logits_process_rows: one processed fp32 row per row r < rows from logits row (r / row_div) (element stride ld),
 * V <= 32768 (KLAB_ERR_UNSUPPORTED above).  Scores = fp32 logits, or their log_softmax when log_softmax != 0 (beam search).
 * History of row r: seq[r*ld_seq + p] for 1 <= p < cur_len, position 0 read as start_id (seq may hold anything there);
 * cur_len <= 1024.  Then, in HF's order:
 *   repetition_penalty != 1: every token of the history (once, however often it occurs) s -> s < 0 ? s * p : s / p;
 *   no_repeat_ngram_size n > 0, cur_len >= n: every window w <= cur_len - n whose n-1 tokens equal the last n-1 bans token w+n-1;
 *   bad words (n_bad entries; entry i = bad_tok[bad_off[i] .. bad_off[i+1]), device, bad_off[n_bad] <= 1024): a 1-token entry is
 *     always banned; a longer entry of length L <= cur_len bans its last token when the history ends with its first L-1;
 *   cur_len < min_length or cur_len - 1 < min_new_tokens: eos_id banned.
 * Banned = -inf.  Outputs: out [rows, ld_out] f32 (NULL allowed only with pick).  pick != 0: also the arg-max of the processed
 * row (the lowest id among equal maxima, 0 when every score is -inf) with klab_sample_rows' bookkeeping: done [rows], eos_id,
 * pad_id, tokens [rows], seq[r*ld_seq + cur_len] (and seq[r*ld_seq] = start_id when cur_len == 1), stop_word; logprob (pick
 * only, ignored otherwise; ld_logprob > cur_len): logprob[r*ld_logprob + cur_len] = log_softmax(processed row)[token], 0 for a row
 * with done[r] != 0 on entry, -inf when every score is -inf.                                                             */
typedef struct {
  int dtype;
  const void* logits; long ld; int row_div;
  int rows, V, log_softmax;
  long long* seq; long ld_seq; int cur_len, start_id;
  float repetition_penalty; int no_repeat_ngram_size, min_length, min_new_tokens, eos_id;
  int n_bad; const int* bad_off; const int* bad_tok;
  float* out; long ld_out;
  int pick; int* done; int pad_id; long long* tokens; int* stop_word;
  float* logprob; long ld_logprob; /* optional, pick only */
} klab_logits_proc_args;
int klab_logits_process_rows(const klab_logits_proc_args* a, void* stream);
/* the beam top-2k of klab_beam_topk over scores that are already log-probabilities (f32, e.g. klab_logits_process_rows with
 * log_softmax): per sample b, the 2k best of  scores row b*k+j + run_score[b*k+j], same order, ties and buffers.           */
int klab_beam_topk_scores(const float* scores, long ld, int row_div, const float* run_score, int B, int k, int V, float* row_score,
                          int* row_idx, float* out_score, int* out_idx, void* stream);
/* ---- trie-constrained decoding (HF's PrefixConstrainedLogitsProcessor without the host callback; csrc/constrain.hip) -----------
 * The trie (klab_multimodalmodel_amd/constrain.py), int32 on the device, CSR: node i's edges are child_tok[child_off[i] ..
 * child_off[i+1]) (token ids, ascending) and lead to child_node[same index]; child_off is [n_nodes + 1], the other two [n_edges].
 * EOS is an ordinary edge to a leaf.  A row's state is the node it stands on: >= 0 a node, -1 off the trie.
 * klab_constrain_rows: one launch advances every row's node and masks its scores.
 *   advance: first != 0: node_out[r] = root[r / root_div]; else node_out[r] = the child of node_in[parent ? parent[r] : r] behind
 *     token last_tok[r] (int64), -1 when that node is -1 or has no such edge (a wave-cooperative 64-ary search over child_tok).
 *     node_in and node_out are different buffers when parent is given (rows read each other's state).
 *   mask: scores = the fp32 value of logits row (r / row_div) (element stride ld, dtype bf16 or f32), or with log_softmax != 0 their
 *     log_softmax over the WHOLE row (the reduction of klab_logits_process_rows, bit for bit); out[r*ld_out + j] = the score where
 *     j is a child token of node_out[r], -inf elsewhere.  A node without children and the state -1 allow exactly eos_id.  out is
 *     f32 [rows, ld_out >= V]; columns >= V are never written.  out may be the f32 input itself (row_div 1, ld_out == ld).
 * V <= 32768 (KLAB_ERR_UNSUPPORTED above).  KLAB_ERR_BADARG: a NULL among logits, out, node_out, child_off, the tables of a trie
 * with edges, root (first) or node_in / last_tok (not first); ld or ld_out < V; n_nodes < 1, n_edges < 0 or n_edges > n_nodes - 1.
 * Indices read from the tables are checked against n_nodes / n_edges / V on the device before they are used.                 */
typedef struct {
  int dtype;
  const void* logits; long ld; int row_div;
  int rows, V, log_softmax;
  const int* child_off; const int* child_tok; const int* child_node; int n_nodes, n_edges;
  int first; const int* root; int root_div;
  const int* node_in; const int* parent; const long long* last_tok;
  int* node_out;
  int eos_id;
  float* out; long ld_out;
} klab_constrain_args;
int klab_constrain_rows(const klab_constrain_args* a, void* stream);
int klab_sizeof_constrain_args(void);
/* The constraint of a decoding session: the trie's tables (device memory, owned by the caller and alive while the session runs, as
 * the forced table; not copied) and root_dev [B] int32 on the device, the start node of every image, shared by its n rows.   */
typedef struct {
  const int* child_off; const int* child_tok; const int* child_node; int n_nodes, n_edges;
  const int* root_dev;
} klab_constraint_cfg;
/* Logits-processor settings of a decoding session (host memory; bad_off / bad_tok are copied at klab_engine_gen_begin).
 * KLAB_ERR_BADARG for penalty <= 0, negative sizes, empty entries or ids >= vocab; KLAB_ERR_UNSUPPORTED for more than 1024
 * bad-word tokens in all.                                                                                                 */
typedef struct {
  float repetition_penalty; int no_repeat_ngram_size, min_length, min_new_tokens;
  int n_bad; const int* bad_off; const int* bad_tok;
} klab_logits_proc_cfg;

/* ---- decoding sessions on an engine binding: HF's `_beam_search`, `_sample` and greedy decoding (ref/models/model.py:27-28,
 * HF/t5:308-332) -- the one way the engine decodes over a K/V cache --------------------------------------------------------------
 * One prefill at B rows, then M = B*n rows on the device (row b*n + j: beam / sample j of image b, HF's
 * `_expand_inputs_for_generation`; the n rows of an image share its cross-attention K/V).  The workspace
 * (klab_engine_gen_workspace_bytes; 0 = unsupported settings) is caller-owned and separate from the binding's: decoder scratch
 * and logits for M rows, the per-layer self-attention cache [M*max_length, 3*inner], the mode's state, the next decoder inputs
 * and the stop words; with processors also an f32 [M, vocab] buffer (not for pick) and the bad-words table.
 * mode KLAB_GEN_BEAM: n = num_beams <= 16, vocab >= 2n; pad_id = HF's output fill value (pad_token_id, or eos when that is 0);
 *   early_stopping 0 False, 1 True, 2 "never"; length_penalty.  Each position: klab_beam_topk (with processors:
 *   klab_logits_process_rows on log_softmax(logits), then klab_beam_topk_scores) and klab_beam_update.  Beam r's self-attention
 *   keys are in the slots of its key-slot table.
 * mode KLAB_GEN_SAMPLE: n = num_return_sequences; temperature > 0, top_k >= 0, 0 <= top_p <= 1, seed.  Each position: the
 *   processors when set (f32 rows), then klab_sample_rows.
 * mode KLAB_GEN_PICK: greedy decoding, one klab_logits_process_rows with pick per position (procs NULL: neutral settings).
 * The processors (procs, NULL = none) need vocab <= 32768, as do sampling and pick.  A begun session keeps the settings it
 * began with; beginning another ends it.
 * gen_begin: after a klab_engine_forward in evaluation mode at B rows with Lt >= max_length - 1; copies position 0's self
 *   K/V into every row's cache slot, initialises the mode's state and chooses position 1 (HF's first step, cur_len 1) from the
 *   prefill's position-0 logits.
 * gen_step(t): the decoder over position t (1 <= t <= max_length - 2, in order) for all M rows, then position t + 1.
 * gen_stop_word: device address of the stop word of position pos, written by the step that chose it.  Beam search goes on iff
 *   bits 1 and 4 are set and, with early_stopping True, bit 2 (see klab_beam_update); sampling and pick go on while it is
 *   non-zero (some row unfinished).
 * gen_buffer: a view into ws for tests and diagnostics (NULL before gen_begin or for another name) -- "logits": [M, vocab] in the
 *   compute dtype, the logits gen_step decoded last; "tokens": [M, 1] int64 (*dtype is left alone), the decoder inputs of the
 *   next gen_step.
 * gen_result: beam search: the first n <= num_beams of each sample's finished pool (sorted by score), length = max_length:
 *   seq [B*n, max_length] int64, scores [B*n] f32, len [B*n] int32 (generated tokens, the start token excluded).  Sampling
 *   and pick: n = the session's n, the first length <= (last position chosen) + 1 columns of the sequences into seq
 *   [B*n, length] int64 (start token, pad_id after EOS); scores and len unused (NULL).
 * want_logprobs (sampling and pick; with beam search the workspace size is 0, unsupported -- it keeps its own scores): the session
 *   also keeps an f32 [M, max_length] buffer of per-token log-probabilities (gen_buffer "logprobs"), zeroed by gen_begin and
 *   written by klab_sample_rows / the pick at every position (column 0 and everything after a row's EOS stay 0).  Without it a
 *   session launches exactly what it launched before the field existed.
 * gen_scores (want_logprobs sessions): klab_gen_finalize over the first length <= (last position chosen) + 1 columns: score [M]
 *   f32, len [M] int32, order [B*n_out] int32 (n_out <= n <= 64; order may be NULL), and the log-probabilities themselves into
 *   token_logprobs [M, length] f32 when not NULL.  All device memory.
 * gen_set_attn / gen_attn_bytes (sampling, pick and force): the session also writes the head-mean cross-attention map of every
 *   position into a caller-owned f32 [n_dec_layers, M, max_length, Le] buffer armed in front of gen_begin (below).
 * gen_set_constraint (pick, sampling and beam search; vocab <= 32768; KLAB_GEN_FORCE with one: KLAB_ERR_BADARG at gen_begin): every
 *   row may only choose a child of the trie node it stands on (klab_constrain_rows).  As the forced table and the maps, the
 *   constraint is armed in front of gen_begin and klab_gen_cfg keeps its fields and its size (below).  The workspace grows, behind everything else, by two int32 [M] node buffers used ping-pong and, where the session has none, by the
 *   f32 [M, vocab] rows.  Every constrained position costs one launch more than the same position unconstrained:
 *     pick, sampling: klab_constrain_rows on the logits into the f32 rows, then the existing chooser over them -- the processors
 *       (the session's settings, for pick neutral ones without) with pick, or the processors in place and klab_sample_rows;
 *     beam search: klab_constrain_rows with log_softmax, then klab_beam_topk_scores; with processors klab_logits_process_rows with
 *       log_softmax, then the constraint in place (a mask of -inf commutes with every processor).
 *   The advance reads the tokens chosen last (the next decoder inputs) and, under beam search, klab_beam_update's parent rows; the
 *   first chosen position (1, or n_forced + 1 behind a decoder prompt, which is not walked) starts every row at root_dev[image].
 *   gen_buffer "nodes": [M, 1] int32, the node every row stood on when the last position was chosen (the walk over the tokens
 *   chosen before it).  The log-probabilities of a want_logprobs session are those of the masked scores.  A session begun without
 *   a constraint armed launches exactly what it launched before the setter existed, and every buffer lies where it lay.        */
#define KLAB_GEN_PICK 0
#define KLAB_GEN_SAMPLE 1
#define KLAB_GEN_BEAM 2
#define KLAB_GEN_FORCE 3
typedef struct {
  int mode, n, max_length, eos_id, pad_id;
  float temperature; int top_k; float top_p; unsigned long long seed; /* sampling only */
  float length_penalty; int early_stopping;                           /* beam search only */
  const klab_logits_proc_cfg* procs;
  int want_logprobs;
} klab_gen_cfg;
/* The forced-token table of the NEXT klab_engine_gen_begin (one-shot, as klab_engine_set_loss_out: gen_begin takes it whether it
 * succeeds or fails, so a session begun without this call never sees a table): tokens_dev int64 [B*n, ld] on the device, owned by
 * the caller and alive while the session runs; row r's token of position p is tokens_dev[r*ld + p], 1 <= p <= n_forced < ld
 * (column 0, the start token's, is not read).  NULL with n_forced 0 disarms.  stream is unused today: the session's own launches
 * read the table on the streams they are given.
 * mode KLAB_GEN_FORCE (scoring given sequences): needs the table with n_forced >= max_length - 1, want_logprobs and no
 *   processors; any vocabulary.  Every position is one klab_force_rows with finish_on_eos = 1 and the log-probability of the
 *   forced token under the raw logits; workspace, gen_result and gen_scores as a pick session with want_logprobs.
 * modes KLAB_GEN_PICK / KLAB_GEN_SAMPLE with a table (a decoder prompt, n_forced <= max_length - 1, without want_logprobs):
 *   positions 1 .. n_forced are klab_force_rows with finish_on_eos = 0 and no logits read, the later ones run as without a
 *   table; the processors see the prompt as history.  KLAB_GEN_BEAM with a table: KLAB_ERR_BADARG.                          */
int klab_engine_gen_set_forced(klab_engine* e, const long long* tokens_dev, long ld, int n_forced, void* stream);
/* Cross-attention maps of the NEXT klab_engine_gen_begin (one-shot in the same way: gen_begin takes the arming whether it succeeds
 * or fails, and a session begun without it launches exactly what it launched before these two functions existed, keeps no maps and
 * returns bit-identical results).  maps_dev: f32 [n_dec_layers, B*n, max_length, Le] on the device (Le = image + source tokens, the
 * encoder length of the binding), owned by the caller, alive while the session runs and NOT part of the session workspace
 * (gen_workspace_bytes is what it is without maps); gen_attn_bytes is its size, 0 for beam search (its rows are re-parented every
 * step; as with want_logprobs it carries no maps) and for settings gen_workspace_bytes returns 0 for.  NULL with 0 bytes disarms.
 * gen_begin returns KLAB_ERR_BADARG when the armed buffer is smaller than gen_attn_bytes or the mode is KLAB_GEN_BEAM.
 * maps[i, r, p, :] = the head mean of layer i's cross-attention probabilities (klab_t5_decode_attn_map) of row r's query at
 * decoder position p - 1, i.e. the attention that produced the token of position p (the column convention of the
 * log-probabilities).  gen_begin clears the buffer with one asynchronous memset and fills column 1 from the prefill's cross q
 * of position 0; gen_step(t) fills column t + 1, one launch per layer beside the unchanged klab_t5_beam_decode_attn.  Column 0,
 * columns not reached and everything after a row's EOS (the session's done flags, as the choosing kernel of the position before
 * left them) stay 0.  No host read is added.  stream is unused today: the session's own launches clear and write the buffer on
 * the streams they are given.                                                                                                */
size_t klab_engine_gen_attn_bytes(klab_engine* e, const klab_gen_cfg* cfg);
int klab_engine_gen_set_attn(klab_engine* e, float* maps_dev, size_t bytes, void* stream);
/* The constraint of the NEXT klab_engine_gen_begin (one-shot in the same way: gen_begin takes it whether it succeeds or fails, so a
 * session begun without this call never sees one).  The struct is copied here; the tables and root_dev are device memory owned by the
 * caller and alive while the session runs.  NULL disarms.  KLAB_ERR_BADARG for a NULL child_off or root_dev, NULL edge tables of a
 * trie with edges, n_nodes < 1, n_edges < 0 or n_edges > n_nodes - 1.  While a constraint is armed klab_engine_gen_workspace_bytes
 * answers for the session the next gen_begin starts: it includes the constraint's buffers (0 for KLAB_GEN_FORCE or vocab > 32768).
 * stream is unused today: the session's own launches read the tables on the streams they are given.                          */
int klab_engine_gen_set_constraint(klab_engine* e, const klab_constraint_cfg* k, void* stream);
size_t klab_engine_gen_workspace_bytes(klab_engine* e, const klab_gen_cfg* cfg);
int klab_engine_gen_begin(klab_engine* e, const klab_gen_cfg* cfg, void* ws, void* stream);
int klab_engine_gen_step(klab_engine* e, int t, void* ws, void* stream);
const int* klab_engine_gen_stop_word(klab_engine* e, void* ws, int pos);
const void* klab_engine_gen_buffer(klab_engine* e, void* ws, const char* name, long* rows, long* cols, int* dtype);
int klab_engine_gen_result(klab_engine* e, void* ws, int n, int length, long long* seq, float* scores, int* len, void* stream);
int klab_engine_gen_scores(klab_engine* e, void* ws, int length, int n_out, float length_penalty, float* token_logprobs, float* score,
                           int* len, int* order, void* stream);
/* segment 0: LM head + decoder + tied embedding; 1: encoder; 2: Swin (no-op unless train_swin).
 * dloss_dev: device scalar d(objective)/d(loss) (NULL = 1).                                       */
int klab_engine_backward(klab_engine* e, int segment, const float* dloss_dev, void* stream);
/* timing probes: when enabled, selected launches are bracketed by two HIP events ON THE STREAM THEY ARE LAUNCHED ON; read back
 * after a synchronize.  channel 0: the LM-head logits GEMM of every forward (symbol klab_lmhead_gemm, compute stream);
 * channel 1: every grouped weight-gradient launch of the T5 backward (symbol gemm_glds_grouped_tn_kernel, the engine's side
 * stream).  probe_read returns the launch count, the summed duration and the summed algorithmic FLOPs (2*M*N*K) of a channel. */
int klab_engine_probe_enable(klab_engine* e, int on);
int klab_engine_probe_read(klab_engine* e, int channel, int* launches, float* total_ms, double* flops_total);
const float* klab_engine_loss_ptr(const klab_engine* e);
/* One-shot: the NEXT klab_engine_forward writes its mean loss to `out` (a device float owned by the caller) instead of the engine's
 * slot -- a caller that hands out a fresh tensor per step (MyModel.forward, ref/models/model.py:26) then needs no copy launch behind
 * the cross-entropy.  Returns 1 if it will be honoured, 0 under graph replay (the loss stays at klab_engine_loss_ptr), < 0 on error. */
int klab_engine_set_loss_out(klab_engine* e, float* out);
/* Options of the training loss.  eps (label smoothing, 0 <= eps < 1) and z (z-loss, >= 0) persist until changed.  `weights` (device,
 * B*n*Lt floats, or NULL) is one-shot like klab_engine_set_loss_out: the NEXT klab_engine_forward copies it into the workspace beside
 * the labels and never reads the caller's tensor again; a caller whose forward failed early passes NULL to disarm it.  With
 * eps == z == 0 and no weights the forward issues klab_ce_fwd as before (graph slots included); otherwise klab_ce_wsum and
 * klab_ce_fwd_opts, eagerly -- never from a captured graph, which would replay the options of the capture. */
int klab_engine_set_loss_options(klab_engine* e, float eps, float z, const float* weights);
/* Knowledge distillation in the training loss (klab_ce_fwd_distill).  alpha (in [0, 1]) and temperature (finite, > 0) persist until
 * changed.  `teacher` (device, B*n*Lt x V logits of dtype t_dtype = KLAB_BF16 or KLAB_F32, row stride V, finite; or NULL) is one-shot
 * and NOT staged: the NEXT klab_engine_forward reads it in place in its loss launch and then forgets the pointer, so it has to stay
 * alive and unchanged until that launch has run; it must not overlap the engine's own logits (KLAB_ERR_BADARG).  A caller whose
 * forward failed early passes NULL to disarm it.  With alpha > 0 and a teacher armed the forward issues klab_ce_wsum and
 * klab_ce_fwd_distill, eagerly -- never from a captured graph, which would replay the teacher's address and the options of the
 * capture; with alpha == 0 or no teacher armed it issues exactly the launches described above.  The per-token kl is the buffer
 * "kl_row" of klab_engine_buffer. */
int klab_engine_set_distill(klab_engine* e, float alpha, float temperature, const void* teacher, int t_dtype);
/* Normaliser of the weighted training loss (klab_ce_fwd_opts / klab_ce_fwd_distill).  mode 0 (the default): sum w l / sum w, as
 * described above.  mode 1: sum w l / N with N the number of labels != -100 -- the forward's two eager loss branches then fill
 * inv_w with klab_ce_count instead of klab_ce_wsum, and weights of either sign are meaningful (signed advantages, whose sum is near
 * zero).  Persists until changed.  With no weights and eps == z == 0 the forward issues klab_ce_fwd in either mode. */
int klab_engine_set_weight_norm(klab_engine* e, int mode);
const int* klab_engine_err_ptr(const klab_engine* e);
/* device words {seed of the current step, base seed, forwards since seeding} (for stream-ordered snapshots; see klab_engine_get_rng) */
const uint32_t* klab_engine_rng_ptr(const klab_engine* e);
const void* klab_engine_buffer(const klab_engine* e, const char* name, long* rows, long* cols, int* dtype);

/* ---- self-critical sequence training (csrc/scst.hip) ------------------------------------------------------------------------
 * klab_ciderd_rewards: out[r] (f32 [rows]) = CIDEr-D, over units = token ids, of hypothesis row r of hyp (int64 [rows, L] as
 * generate returns them: column 0 the start token, pads after EOS; rows = B * n_h, row r belongs to image r / n_h) against the
 * present references of its image in refs (int64 [B, R, Lr] in label format: closed by EOS, whatever follows ignored; a row whose
 * first entry is negative is absent).  Units: the tokens through the first EOS, the EOS itself when count_eos; an id < 0 or
 * >= 0xFFFF ends the sequence.  (keys, idf): the document-frequency table, cap slots (a power of two >= 2), key = t0 | t1 << 16 |
 * t2 << 32 | t3 << 48 with 0xFFFF in absent positions, all ones = empty slot, home slot (key * 0x9E3779B97F4A7C15) >> (64 - log2
 * cap), linear probing with wrap-around; an n-gram it does not hold weighs log_n.  Exactly 0 when the image has no present
 * reference or the hypothesis no units.  One launch; the same bits on every run.
 * KLAB_ERR_UNSUPPORTED (before anything is enqueued): L > 65, Lr > 64, R outside 1..16.
 * klab_scst_targets: seq int64 [rows, L] (rows = B * n), rewards f32 [rows] -> labels int64 [rows, Lt] (seq's columns 1.. through
 * the row's first EOS, all L - 1 without one; -100 behind), weights f32 [rows, Lt] (the row's advantage on its scored columns, 0
 * elsewhere) and advantages f32 [rows].  mode 0: reward - baseline[b] (f32 [B]); 1: leave-one-out, reward - (sum of the image's
 * other rewards, in index order) / (n - 1), n >= 2; 2: the reward.  Lt >= L - 1.  Every output element is stored exactly once. */
int klab_ciderd_rewards(const long long* hyp, int rows, int n_h, int L, const long long* refs, int R, int Lr,
                        const unsigned long long* keys, const float* idf, long cap, float log_n, float sigma, int eos, int count_eos,
                        float* out, void* stream);
int klab_scst_targets(const long long* seq, int rows, int n, int L, const float* rewards, const float* baseline, int mode, int eos, int Lt,
                      long long* labels, float* weights, float* advantages, void* stream);

/* ---- caption metrics (csrc/metrics.hip) ----------------------------------------------------------------------------------------
 * klab_caption_stats: stats (int32 [rows, 16]) = the integer sufficient statistics of BLEU-1..4 and ROUGE-L of hypothesis row r of
 * hyp against the present references of image r / n_h.  hyp, rows, n_h, L, refs, R, Lr, eos, count_eos and the units rule are
 * klab_ciderd_rewards' (hyp int64 [rows, L], column 0 the start token; refs int64 [B, R, Lr] in label format, a row whose first
 * entry is negative is absent; units = the tokens through the first EOS, the EOS itself when count_eos; an id < 0 or >= 0xFFFF
 * ends the sequence).  Columns:
 *   0..3   match_n, n = 1..4: sum over the hypothesis' distinct n-grams g of min(count_h(g), max_j count_j(g)), j over the present
 *          references (BLEU's clipped matches)
 *   4..7   guess_n = max(0, len_h - n + 1)
 *   8      len_h, the number of units            9  the present reference length closest to len_h, the shorter one on a tie
 *   10     max_j LCS(h, r_j) (ROUGE-L's precision numerator)
 *   11,12  the pair (lcs_j, len_j) with the largest lcs_j / len_j, decided by integer cross-multiplication: it starts as (0, 0); a
 *          present reference with len_j >= 1 replaces it when its length is 0 or lcs_j * len_best > lcs_best * len_j (the lowest
 *          index wins a tie, references without units are skipped)
 *   13     the number of present references      14, 15  0
 * A present reference without units counts in column 13 and takes part in column 9 with length 0; an image without present
 * references gives a row of zeros.  No floating point, no atomics; every element is stored exactly once; one launch.
 * KLAB_ERR_UNSUPPORTED (before anything is enqueued): L > 65, Lr > 64, R outside 1..16. */
int klab_caption_stats(const long long* hyp, int rows, int n_h, int L, const long long* refs, int R, int Lr, int eos, int count_eos,
                       int* stats, void* stream);

/* ---- crash diagnostics (opt-in; csrc/diag.cpp) -------------------------------------------------------------------------
 * klab_segv_trace_install: on SIGSEGV / SIGBUS / SIGABRT / SIGFPE / SIGILL write the context string and the native backtrace
 * of the faulting thread to file descriptor fd (< 0: stderr), then re-raise with the default action.
 * klab_segv_set_context: the string to print (the test harness passes the running pytest node id).                       */
int klab_segv_trace_install(int fd);
int klab_segv_set_context(const char* text);

#ifdef __cplusplus
}
#endif
#endif /* KLAB_MM_H */
