/* fervit.h — C ABI of libfervit.so, the MI355X (gfx950) kernels behind the
 * FER-ViT training hot path.
 *
 * The reference (yuki-ominato/FER-ViT) is pure PyTorch: its hot-path "ABI" is the
 * set of torch.nn modules its models compose. Each entry point below replaces
 * one of those calls (reference file:line given per function); the Python host
 * (`fer-vit_amd/fervit/`) binds them with ctypes behind the reference's own
 * model constructors (`models_fer_vit/`, `modules/`).
 *
 * Conventions
 *  - Plain pointers to device memory owned by the caller (the PyTorch caching
 *    allocator); the library never allocates or frees caller memory. Optional
 *    pointers may be NULL.
 *  - Activations are row-major [rows][cols]; `dtype` selects FER_BF16 (fast path,
 *    fp32 accumulation) or FER_F32 (exact parity path); any other code is an
 *    error ("<entry>: unknown dtype"; the size queries that take a dtype then
 *    return -1), checked before anything else. Parameters, their
 *    gradients, LayerNorm statistics and logits are always fp32.
 *  - Every call enqueues on `stream` and never synchronises the host.
 *  - Return 0 on success, a negative code on error; fer_last_error() then
 *    returns a thread-local message. No C++ exception crosses the ABI.
 *  - Dropout masks are regenerated from (seed, element index): element i is
 *    dropped iff its 16-bit uniform u16(i) < drop_thresh. Callers pass
 *    drop_thresh = round(p * 65536) clamped to [1, 65535] for 0 < p < 1,
 *    0 = dropout off (p = 0), 65536 = drop everything (p = 1, with drop_scale 0);
 *    drop_scale = 1/(1-p). (fervit/ops.py drop_args is the reference encoder.)
 *  - Gradient all-reduce (DDP) is NOT in this ABI: the Python host issues it through
 *    torch.distributed's "nccl" backend (= RCCL on ROCm) on a side stream, ordered against
 *    these kernels by HIP events (fervit/ddp.py). No fer_rccl_* entry points exist.
 */
#ifndef FERVIT_H
#define FERVIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* fer_stream_t; /* == hipStream_t */

enum { FER_BF16 = 0, FER_F32 = 1 };
enum { FER_ACT_NONE_ = 0, FER_ACT_GELU_ = 1, FER_ACT_RELU_ = 2, FER_ACT_MUL_ = 3 /* aux_act only */ };
enum { FER_PRE_GATE_ = 16 /* act flag, see fer_epilogue */ };

/* C = epilogue(sum_k A(m,k) B(n,k)); A(m,k) = a_kc ? A[m*lda+k] : A[k*lda+m],
 * B(n,k) = b_kc ? B[n*ldb+k] : B[k*ldb+n].
 * Replaces nn.Linear forward/dgrad/wgrad (`image_vit.py:101-113`, `latent_vit.py:20,24-31`,
 * `hybrid_latent_vit.py:79`) and nn.Conv2d(k=P,s=P) patch embedding (`image_vit.py:27-32`)
 * once the input is in im2col order. ws: optional fp32 split-K workspace. */
typedef struct {
  int dtype;
  const void* A; int64_t lda; int a_kc;
  const void* B; int64_t ldb; int b_kc;
  int M, N, K;
  float* ws; int64_t ws_bytes;
} fer_gemm_desc;

/* Epilogue, applied per element in this order:
 *   v = alpha*acc (+ bias[n]); pre[m][n] = v; v = act(v); v = dropout(v, seed, m*drop_ld+n);
 *   v *= *post_scale; v *= act'(aux[m][n]); v += res[m][n]; c[m][n] (+)= v
 * act | FER_PRE_GATE_: pre[m][n] receives the backward gate act'(v) * keep * drop_scale (the
 * same keep bit as v's dropout) instead of v; the input-gradient GEMM of the next layer then
 * applies act' and the dropout in one multiply with aux_act = FER_ACT_MUL_ (v *= aux[m][n]). */
typedef struct {
  void* c; int64_t ldc; int c_f32; int accumulate; float alpha;
  const float* bias; int act;
  void* pre; int64_t ldp;
  const void* res; int64_t ldr;
  uint32_t drop_thresh; float drop_scale; uint64_t seed; int64_t drop_ld;
  const void* aux; int64_t ldx; int aux_act;
  const float* post_scale;
  /* optional fp32 column sums of the final output (the bias gradient of a layer whose input
   * gradient this GEMM produces, e.g. linear1.bias from the linear2 dgrad): colsum[n] (+)=
   * sum_m c[m][n]. Fused into the tile epilogue (per-tile partials + a fixed-order reduction,
   * deterministic); needs the desc workspace ws (>= fer_gemm_colsum_ws bytes). */
  float* colsum; int colsum_accumulate;
} fer_epilogue;

int fer_gemm(const fer_gemm_desc* d, const fer_epilogue* e, fer_stream_t stream);

/* Grouped weight gradients: dw[n][k] (+)= sum_m dy[m][n] x[m][k] (bf16 dy [M][N] row stride ld_dy,
 * bf16 x [M][K] row stride ld_x, fp32 dw [N][K] row stride ld_dw) for up to 8 nn.Linear weights
 * that share the token count M, in one launch -- the weight-gradient half of nn.Linear's backward
 * (`latent_vit.py:20,24-31`, `image_vit.py:101-113` TransformerEncoderLayer linears) for the
 * small-token configurations, where each weight alone is too few output tiles to fill the GPU.
 * splits: K (token) split per tile, 0 = automatic; a split run needs ws >= fer_wgrad_group_ws
 * bytes (fp32 slabs + tile tickets; the reduction is in-launch, fixed split order). */
typedef struct {
  const void* dy; int64_t ld_dy;
  const void* x; int64_t ld_x;
  float* dw; int64_t ld_dw;
  int M, N, K; int accumulate;
} fer_wgrad_item;
int fer_wgrad_group(const fer_wgrad_item* items, int n, int splits, float* ws, int64_t ws_bytes, fer_stream_t stream);
int64_t fer_wgrad_group_ws(const fer_wgrad_item* items, int n, int splits);

/* Workspace bytes fer_gemm needs for the fused column sums of an M x N output. */
int64_t fer_gemm_colsum_ws(int M, int N);

/* Tuning/testing hook (no reference counterpart): force the bf16 GEMM tile configuration for
 * every later fer_gemm call of the process. Accepted values (csrc/gemm.hip FER_TILE_CFGS):
 *   -1  automatic (default; it chooses among the four below)
 *    3  double-buffered 128x128 tiles, two workgroups per CU
 *    5  BK=32 ring, 256x256 tiles (the automatic choice for MN x MN weight gradients)
 *    8  8-phase persistent kernel, 256x256 tiles
 *   11  double-buffered 128x64 tiles, three workgroups per CU (128x128 when B is MN-contiguous)
 * Any other value returns non-zero, sets fer_last_error and leaves the selection unchanged.
 * Results are identical up to fp32 summation order. */
int fer_gemm_set_config(int cfg);

/* Testing / A/B hook (no reference counterpart): the persistent kernels (8-phase GEMM, persistent
 * attention; one workgroup per CU) take their items from a per-(device, stream) work queue
 * (mode 0, default) or walk a fixed blockIdx stride (mode 1; FERVIT_FIXED_STRIDE=1 sets it at
 * start-up). Results are bit-identical between the modes. */
int fer_set_persistent_mode(int mode);

/* A HIP stream whose kernels run only on the CUs set in mask (nwords 32-bit words, bit i = CU i in
 * the driver's CU numbering; hipExtStreamCreateWithCUMask), or with nwords = 0 an unmasked stream
 * of the given priority. For the weight-gradient side stream of the backward
 * (`train/train_image_vit.py:124` loss.backward(): this path's dgrad / wgrad split over streams);
 * the caller owns the stream (fer_stream_destroy). With a mask the stream is a BLOCKING stream
 * (it serialises with the legacy null stream) at the default priority, and a non-zero priority is
 * an error; without one it is non-blocking. Destroy a stream only once no live tensor of the
 * caller's allocator has it recorded (torch record_stream). */
int fer_stream_create_cu_mask(const uint32_t* mask, int nwords, int priority, fer_stream_t* out);
int fer_stream_destroy(fer_stream_t stream);

/* LayerNorm forward over rows of x [M][D] (nn.LayerNorm, biased variance;
 * post-norm `nn.TransformerEncoderLayer` norm1/norm2, heads `image_vit.py:162-163`,
 * `latent_vit.py:33-36`, timm pre-norm eps 1e-6). gamma/beta are [gamma_rows][D]:
 * row r uses gamma[(r / row_div) % gamma_rows] (gamma_rows=1: shared; LayerWiseNorm
 * `modules/layer_wise_norm.py:35-46` uses gamma_rows=L, row_div=1).
 * Saves mean/rstd [M] (fp32). y may alias nothing. */
int fer_layernorm_fwd(int dtype, const void* x, int64_t ldx, const float* gamma, const float* beta,
                      int gamma_rows, int row_div, void* y, int64_t ldy, float* mean, float* rstd,
                      int M, int D, float eps, fer_stream_t stream);

/* LayerNorm backward. dx = LN'(dy) (+ res), optional dx_drop = dropout_bwd(dx) (mask of
 * the branch feeding the norm's input, post-norm residual `x + Drop(h)`).
 * Column partial sums go to ws ([nblk][3][D] fp32, ws_bytes >= fer_layernorm_bwd_ws(M,D));
 * dgamma/dbeta/dbias (optional, [D] fp32) receive sum(dy*xhat), sum(dy), sum(dx_drop or dx)
 * over all rows; accumulate != 0 adds to them. They need a shared gamma: with gamma_rows > 1
 * asking for any of them is an error ("parameter grads need shared gamma"; LayerWiseNorm's
 * per-layer gradients come from fer_wplus_bwd). dx_drop has dx's row stride lddx. */
int64_t fer_layernorm_bwd_ws(int M, int D);
int fer_layernorm_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* mean,
                      const float* rstd, const float* gamma, int gamma_rows, int row_div, const void* res,
                      int64_t ldr, void* dx, int64_t lddx, void* dx_drop, uint32_t drop_thresh, float drop_scale,
                      uint64_t seed, float* dgamma, float* dbeta, float* dbias, int accumulate, float* ws,
                      int64_t ws_bytes, int M, int D, fer_stream_t stream);

/* Multi-head self-attention core, softmax(Q K^T * scale) V with dropout on the
 * probabilities (F.multi_head_attention_forward -> scaled_dot_product_attention inside
 * nn.TransformerEncoderLayer; timm Attention for the hybrid). qkv: [B*N][ld_qkv] with
 * q|k|v column blocks of width H*dh (in_proj rows order); out: [B*N][ld_out].
 * `saved` (saved_floats fp32 words, >= fer_attention_saved_floats(...)) is the state kept for the
 * backward: lse [B*H*N] (natural log), padded to a multiple of 64 words, then -- bf16 with dropout,
 * N <= 224, dh <= 64 -- the probability-dropout keep bits, [B*H][NB][NB][32] uint32 (NB = ceil(N/32);
 * word (kb, qb, j) = bits over the 32 queries of block qb for key kb*32 + j; words of padding keys
 * kb*32 + j >= N unspecified), so the backward does not re-hash them. bf16: any N, dh <= 128,
 * dh % 8 == 0. Which kernels a call runs is decided in one place, attn_plan() in csrc/attention.hip:
 * with dh <= 64, N <= 224 runs the persistent family (workgroups walking the (batch, head) units) and
 * 224 < N <= 256 one workgroup per unit; everything else streams 128-row chunks through LDS. */
int64_t fer_attention_ws(int dtype, int B, int N, int H);
/* Forward kernel of the persistent family: 0 automatic (the occupancy form for N > 96 with dropout on,
 * else the persistent kernel), 1 the persistent producer / consumer kernel, 2 the occupancy form (one
 * workgroup per (batch, head), two per CU). Same results bit for bit. */
int fer_attention_set_fwd_kernel(int k);
int64_t fer_attention_saved_floats(int dtype, int B, int N, int H, int dh, uint32_t drop_thresh);
int fer_attention_fwd(int dtype, const void* qkv, int64_t ld_qkv, void* out, int64_t ld_out, float* saved,
                      int64_t saved_floats, int B, int N, int H, int dh, float scale, uint32_t drop_thresh,
                      float drop_scale, uint64_t seed, float* ws, int64_t ws_bytes, fer_stream_t stream);
/* Backward: dqkv [B*N][ld_dqkv] (dq|dk|dv). Optional colsum [3*H*dh] fp32 (+)= column sums of
 * dqkv over the B*N rows = in_proj.bias gradient, fused into the kernel (per-(batch) partials
 * + fixed-order reduction). ws >= fer_attention_ws bytes (fp32 path scratch / colsum partials). */
int fer_attention_bwd(int dtype, const void* qkv, int64_t ld_qkv, const void* out, int64_t ld_out,
                      const void* dout, int64_t ld_dout, const float* saved, int64_t saved_floats, void* dqkv,
                      int64_t ld_dqkv, float* ws, int64_t ws_bytes, int B, int N, int H, int dh, float scale,
                      uint32_t drop_thresh, float drop_scale, uint64_t seed, float* colsum, int colsum_accumulate,
                      fer_stream_t stream);

/* Attention maps (eval semantics, no dropout): probs = fp32 softmax(Q K^T * scale) of the query rows
 * q0 .. q0+nq-1 of every batch element -- what nn.MultiheadAttention(need_weights=True) returns
 * (`image_vit.py:101`, `latent_vit.py:24` encoder layers) and what a forward hook on timm's
 * Attention sees (hybrid); the fused forward above never materialises them. qkv: the layout
 * fer_attention_fwd takes ([B*N][ld_qkv], q|k|v column blocks of width H*dh).
 *   head_avg = 0: probs [B][H][nq][N];  head_avg = 1: probs [B][nq][N], the mean over heads, summed in
 *   head order 0..H-1 inside one workgroup (deterministic, no atomics; the per-head tensor is never
 *   written). probs_floats: capacity of probs in floats, >= B*(head_avg ? 1 : H)*nq*N.
 * A row-selected call returns the same bits as the matching rows of a full call. No workspace:
 * Q K^T is computed twice (max / sum pass, then normalise-and-store pass).
 * bf16: any N >= 1, dh <= 128, dh % 8 == 0, ld_qkv % 8 == 0, qkv 16-byte aligned, H <= 128;
 * fp32: exact parity path (plain FMA), any dh. q0 < 0, nq < 1, q0 + nq > N, a short probs buffer or an
 * unsupported dh return a negative code and launch nothing. */
int fer_attention_probs(int dtype, const void* qkv, int64_t ld_qkv, int B, int N, int H, int dh, float scale,
                        int head_avg, int q0, int nq, float* probs, int64_t probs_floats, fer_stream_t stream);
/* CLS row of the attention rollout (Abnar & Zuidema 2020) over L layers of head-averaged maps
 * [L][B][N][N] fp32: r [B][N] = row 0 of A'_L ... A'_1, A'_l = residual*I + (1-residual)*A_l, as a
 * chain of vector-matrix products (r = e_0; for l = L..1: r <- residual*r + (1-residual)*(r A_l)),
 * O(L N^2). One workgroup per batch element, fixed summation order (deterministic). Any L >= 1,
 * 1 <= N <= 7680 (r is double-buffered in LDS); residual outside [0, 1) is an error. */
int fer_attention_rollout_cls(const float* maps, int L, int B, int N, float residual, float* r, fer_stream_t stream);

/* Evaluation metrics (`eval/evaluate_model.py:135-159`: softmax, argmax and the host's sklearn
 * confusion_matrix / classification_report; `eval/evaluate_model.py:231-296`: cosine similarity of the
 * final tokens). One kernel per call, no host read, no allocation: each call can be captured.
 *
 * fer_cls_stats: one batch of fp32 logits [B][C] (row stride ld) and int64 labels [B]. Outputs, each
 * optional (NULL skips it):
 *   preds int64 [B]       lowest index of the row maximum; a NaN counts as the maximum and the first NaN
 *                         wins (torch.argmax's CPU rule: [1, 5, 5, 2] -> 1, [1, nan, 5, nan] -> 1)
 *   probs fp32 [B][C]     exp(z_i - m) / sum_j exp(z_j - m), m the row maximum, fp32, the sum in one fixed
 *                         order (row stride ld_probs)
 *   conf fp32 [B]         probs[pred]
 *   confusion int64 [C][C], contiguous, row = label, column = prediction: ACCUMULATED (64-bit atomic adds;
 *                         integer adds give the same bits in any order); the caller zeroes it once per epoch
 *   counters int64 [2]    rows counted, rows skipped: accumulated too
 * A label outside [0, C) (-100, -1, C) adds nothing to confusion and one to the skipped counter; preds,
 * conf and probs of that row are still written. C < 1, ld < C, ld_probs < C, NULL logits or labels: a
 * negative code, a message, nothing launched. B <= 0 is a no-op.
 *
 * fer_cls_report: confusion [C][C] -> out fp64 [4 + 4*C]: accuracy, f1_macro, f1_weighted, n, then per
 * class precision, recall, f1, support. One workgroup, fp64, fixed order. A zero denominator gives 0
 * (sklearn's zero_division default); f1_macro averages over the classes present in labels or predictions
 * (row sum + column sum > 0: sklearn's rule for labels=None); n = 0 gives all zeros.
 *
 * fer_token_cosine: tokens [B][N][D] (bf16 or fp32; row stride ld, batch stride N*ld), cos(x, y) =
 * x.y / (max(|x|, eps) * max(|y|, eps)) (torch.cosine_similarity's per-vector clamp). cls_sim fp32
 * [B][N-1] (row stride ld_cls): row 0 against rows 1..N-1; tok_sim fp32 [B][N-1][N-1] (row stride ld_tok,
 * batch stride (N-1)*ld_tok): rows 1..N-1 against each other. Each optional, at least one required; alone
 * or together they hold the same bits. bf16: MFMA Gram tiles, D % 32 == 0, ld % 8 == 0; fp32: FMA,
 * D % 4 == 0, ld % 4 == 0; tokens 16-byte aligned; N >= 2. Squared norms in fp32. */
int fer_cls_stats(const float* logits, int64_t ld, const int64_t* labels, int B, int C, int64_t* preds, float* conf,
                  float* probs, int64_t ld_probs, int64_t* confusion, int64_t* counters, fer_stream_t stream);
int fer_cls_report(const int64_t* confusion, int C, double* out, fer_stream_t stream);
int fer_token_cosine(int dtype, const void* tokens, int64_t ld, int B, int N, int D, float eps, float* cls_sim,
                     int64_t ld_cls, float* tok_sim, int64_t ld_tok, fer_stream_t stream);

/* Batched linear-SVM passes (`latent_analysis/compute_expression_direction.py:58-116`: LinearSVC(C = 0.1,
 * class_weight = 'balanced') on the flattened w+ latents; fervit/directions.py holds the solver). Column p of a
 * launch is the one-vs-rest problem of class classes[p]:
 *   f_p(w, b) = 1/2 |w|^2 + 1/2 b^2 + sum_i c_i max(0, m_i)^2,  m_i = 1 - s_i (w.x_i + b),
 *   s_i = +1 if labels[i] == classes[p] else -1,  c_i = Cp[p] for s_i = +1, Cn[p] for s_i = -1
 * (liblinear's L2-regularised squared hinge with a regularised bias). All fp32, fp32 accumulation, 1 <= P <= 8
 * columns per launch, every row stride an argument (in floats, >= the row length; rows need no alignment: a
 * 16-byte aligned operand with a stride that is a multiple of 4 moves in 16-byte pieces, any other element by
 * element, with the same bits). No host read, no allocation: capturable. ws: 16-byte aligned,
 * >= fer_svm_ws(N, F) bytes. Every sum has a fixed partition and order (no floating-point atomics): the same
 * input gives the same bits on every call.
 *
 * fer_svm_forward: Z[N][P] = X[N][F] W[P][F]^T + bias[P] (Z optional), then
 *   epilogue 0 (hinge): labels int64 [N], classes int64 [P], Cp, Cn fp32 [P] -> R[i][p] = c a s m (the
 *     residual: grad_w f_p = w - 2 sum_i R[i][p] x_i, d f_p / d b = b - 2 sum_i R[i][p]), Dw[i][p] = c a with
 *     a = [m > 0] (the curvature weights: the Hessian is I + 2 X^T diag(Dw) X, bias column included), and
 *     loss[p] = sum_i c a m^2, summed per 256 rows and then over those sums in row order;
 *   epilogue 1 (scale): Dw is read, R[i][p] = Dw[i][p] Z[i][p]: the inner half of a Hessian-vector product
 *     (W holds the direction, bias its bias component).
 * fer_svm_xtr: G[P][F] = sum_i R[i][p] X[i][f], gb[P] = sum_i R[i][p] (each optional, one required). Rows are
 * cut into slabs of FER_SVM_SLAB; a sum runs over a slab's rows in order, over the slabs of a group in order
 * (ceil(slabs / FER_SVM_MAX_GROUPS) consecutive slabs per group), then over the groups in order.
 * N <= 0 is a no-op; a bad argument returns a negative code and a message and launches nothing. */
#define FER_SVM_SLAB 32
#define FER_SVM_MAX_GROUPS 128
int fer_svm_slab(void);
int fer_svm_max_groups(void);
int64_t fer_svm_ws(int N, int F);
int fer_svm_forward(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, int N, int F, int P,
                    int epilogue, const int64_t* labels, const int64_t* classes, const float* Cp, const float* Cn,
                    float* Z, int64_t ldz, float* R, int64_t ldr, float* Dw, int64_t ldd, float* loss, float* ws,
                    int64_t ws_bytes, fer_stream_t stream);
int fer_svm_xtr(const float* X, int64_t ldx, const float* R, int64_t ldr, int N, int F, int P, float* G, int64_t ldg,
                float* gb, float* ws, int64_t ws_bytes, fer_stream_t stream);

/* Column sums: out[n] (+)= scale * sum_m x[m][n]  (bias gradients). ws >= fer_colsum_ws(M,N). */
int64_t fer_colsum_ws(int M, int N);
int fer_colsum(int dtype, const void* x, int64_t ldx, int M, int N, float* out, int accumulate,
               const float* scale_ptr, float* ws, int64_t ws_bytes, fer_stream_t stream);

/* Deferred gradient reductions (the framework's backward pass; no reference counterpart: the
 * reference's bias / LayerNorm gradients come out of torch autograd one kernel each). mode 1
 * opens (or resumes) a window: fer_layernorm_bwd / fer_attention_bwd / fer_colsum / fused GEMM
 * column sums issued on `stream` write their per-block column partials into `arena` and queue the
 * fixed-order partial sum instead of launching it; mode 2 pauses (the queue stays, new calls run
 * immediately); mode 0 flushes and closes. fer_reduce_flush runs every queued sum as ONE launch on
 * that stream (bit-identical to the immediate path). Callers flush before anything reads those
 * gradients. Host state is per process (one window at a time, on one device: opening it from another
 * device while open is an error). Only part_reduce writers (the entry points above) are ordered
 * against the queue -- a queued sum runs first when a later reduction's output range overlaps its
 * own; any OTHER kernel that writes a queued gradient inside the window must flush first. */
int fer_reduce_defer(int mode, void* arena, int64_t arena_bytes, fer_stream_t stream);
int fer_reduce_flush(void);

/* Patch im2col (nn.Conv2d k=P,s=P, `image_vit.py:27-43`): x fp32 NCHW [B][C][Hh][Ww] ->
 * cols [B*gh*gw][ldc] in (c,kh,kw) order, cast to dtype. */
int fer_im2col_patch(int dtype, const float* x, int B, int C, int Hh, int Ww, int P, void* cols, int64_t ldc,
                     fer_stream_t stream);

/* Token assembly: t[b][0] = cls + pos[0]; t[b][1+i] = emb[b*n+i] + pos[1+i] (emb may be
 * dtype; `image_vit.py:151-156`, `latent_vit.py:42-44`, `hybrid_latent_vit.py:218-222`),
 * optional embedding dropout. Backward: dcls += sum_b dt[b][0], dpos += sum_b dt[b],
 * demb[b*n+i] = dt[b][1+i] (dropout-masked). ws >= fer_tokens_bwd_ws(B,N,D). */
int fer_tokens_fwd(int dtype, const void* emb, const float* cls, const float* pos, void* t, int B, int n, int D,
                   uint32_t drop_thresh, float drop_scale, uint64_t seed, fer_stream_t stream);
int64_t fer_tokens_bwd_ws(int B, int N, int D);
int fer_tokens_bwd(int dtype, const void* dt, void* demb, float* dcls, float* dpos, int accumulate, int B, int n,
                   int D, uint32_t drop_thresh, float drop_scale, uint64_t seed, float* ws, int64_t ws_bytes,
                   fer_stream_t stream);

/* Classification head on the CLS rows: logits = LN(t[b*N]) W^T + b (fp32 out), W [C][D].
 * (`image_vit.py:161-164`, `latent_vit.py:33-36,46-47`, `hybrid_latent_vit.py:110-114,236-237`) */
int fer_head_fwd(int dtype, const void* t, int64_t row_stride, const float* ln_w, const float* ln_b, float eps,
                 const float* W, const float* bias, float* logits, float* stats, int B, int D, int C,
                 uint32_t drop_thresh, float drop_scale, uint64_t seed, fer_stream_t stream);
/* Backward: dt rows b*row_stride get d(CLS); all other rows of dt are zeroed when
 * zero_rest != 0. Parameter grads accumulate when accumulate != 0. */
int64_t fer_head_bwd_ws(int B, int D, int C);
int fer_head_bwd(int dtype, const void* t, int64_t row_stride, const float* ln_w, const float* ln_b,
                 const float* W, const float* stats, const float* dlogits, void* dt, int zero_rest, int rows_total,
                 int D_ld, float* dln_w, float* dln_b, float* dW, float* dbias, int accumulate, int B, int D, int C,
                 uint32_t drop_thresh, float drop_scale, uint64_t seed, float* ws, int64_t ws_bytes,
                 fer_stream_t stream);

/* ---- LatentCNN baseline (`models_fer_vit/latent_cnn.py`), csrc/convbn.hip. Token-major [M = B*L][C]:
 * the reference's x.transpose(1, 2) (`latent_cnn.py:146,326`) is free and BatchNorm's channel axis is the
 * column axis. Rows are moved in 16-byte pieces: C (3*C for cols) must be a multiple of 8 (bf16) or 4
 * (fp32), row strides likewise, base pointers 16-byte aligned. A rejected call launches nothing. */

/* nn.Conv1d(kernel_size=3, padding=1, stride=1) (`latent_cnn.py:22-23,49,51,282,287,292`) as im2col
 * around fer_gemm: cols[b*L + l][cin*3 + k] = x[b*L + l + k - 1][cin] for 0 <= l + k - 1 < L, else 0
 * (never the neighbouring sample); dtype in = dtype out, values copied bit for bit. The (cin, k) column
 * order is the memory order of nn.Conv1d.weight [Cout][Cin][3], so the parameter (and its bf16 shadow)
 * is fer_gemm's B operand with K = 3*Cin as it stands and the weight gradient lands in its own layout. */
int fer_conv1d_cols(int dtype, const void* x, int64_t ldx, void* cols, int64_t ldc, int B, int L, int C,
                    fer_stream_t stream);
/* Its adjoint: dx[b*L + l][c] = (res[b*L + l][c] +) sum_k dcols[b*L + l - k + 1][c*3 + k] over
 * 0 <= l - k + 1 < L. res (optional): the gradient arriving over a residual connection
 * (LatentResBlock1D `latent_cnn.py:56,61`), added first. */
int fer_conv1d_cols_bwd(int dtype, const void* dcols, int64_t ldd, const void* res, int64_t ldr, void* dx,
                        int64_t lddx, int B, int L, int C, fer_stream_t stream);

/* nn.BatchNorm1d over the M rows of x [M][C] (`latent_cnn.py:24,50,52,117,283,288,293`), fp32
 * statistics, with the model's epilogues fused: y = dropout(relu?(gamma * xhat + beta (+ res))).
 * train != 0: per-channel mean and biased variance of this call's rows (two passes: mean, then squared
 * deviations), running_mean / running_var (optional) updated on the device with `momentum` and the
 * unbiased variance M/(M-1), *num_batches_tracked (optional, int64) += 1; needs M >= 2.
 * train == 0: normalises with running_mean / running_var (required), updates nothing.
 * mean / rstd (optional, [C] fp32) receive the statistics used, for the backward. relu: 0 / 1. res
 * optional (LatentResBlock1D `latent_cnn.py:60-62`). No workspace; repeat calls are bit-identical. */
int fer_batchnorm_fwd(int dtype, const void* x, int64_t ldx, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, int train,
                      float momentum, float eps, const void* res, int64_t ldr, int relu, uint32_t drop_thresh,
                      float drop_scale, uint64_t seed, void* y, int64_t ldy, float* mean, float* rstd, int M, int C,
                      fer_stream_t stream);
/* Backward: g = dy * [pre-ReLU value > 0] * keep * drop_scale with the gate and the keep bits recomputed
 * from x, res and the seed (no mask is stored); dbeta (+)= sum g, dgamma (+)= sum g * xhat over the rows;
 * dx = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat)) (train) or gamma * rstd * g (train == 0);
 * dres (optional) = g, the gradient of the residual branch. dx, dres, dgamma, dbeta are each optional
 * (at least one). mean / rstd: what the forward saved. */
int fer_batchnorm_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, const void* res, int64_t ldr,
                      int relu, uint32_t drop_thresh, float drop_scale, uint64_t seed, int train, void* dx,
                      int64_t lddx, void* dres, int64_t lddr, float* dgamma, float* dbeta, int accumulate, int M,
                      int C, fer_stream_t stream);

/* nn.AdaptiveAvgPool1d(1) + nn.Flatten (`latent_cnn.py:109,115,157,297,328`): y[b][c] = mean over l of
 * x[b*L + l][c]; backward dx[b*L + l][c] = dy[b][c] / L. */
int fer_seq_mean_fwd(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int B, int L, int C,
                     fer_stream_t stream);
int fer_seq_mean_bwd(int dtype, const void* dy, int64_t lddy, void* dx, int64_t lddx, int B, int L, int C,
                     fer_stream_t stream);

/* The final nn.Linear(D, C) of the classifiers (`latent_cnn.py:120,304`; C = 7 is below fer_gemm's
 * N % 4 and fer_head_fwd has a LayerNorm built in): logits[b][c] = sum_d x[b][d] W[c][d] + bias[c], fp32
 * out, W [C][D] and bias fp32 (bias optional). Backward: dx[b][d] = (sum_c dlogits[b][c] W[c][d]) *
 * gate[b][d] (gate optional: the act' * keep * scale a fer_gemm FER_PRE_GATE_ epilogue wrote for x),
 * dW[c][d] (+)= sum_b dlogits[b][c] x[b][d], dbias[c] (+)= sum_b dlogits[b][c]; each output optional,
 * every sum a fixed-order loop (deterministic). */
int fer_logits_fwd(int dtype, const void* x, int64_t ldx, const float* W, const float* bias, float* logits, int B,
                   int D, int C, fer_stream_t stream);
int fer_logits_bwd(int dtype, const void* x, int64_t ldx, const float* W, const float* dlogits, const void* gate,
                   int64_t ldg, void* dx, int64_t lddx, float* dW, float* dbias, int accumulate, int B, int D, int C,
                   fer_stream_t stream);

/* ---- LatentCNNDeep (`latent_cnn.py:164-261`), csrc/attnpool.hip. Same layout and 16-byte piece rules
 * as the LatentCNN baseline above. */

/* Attention pooling (`latent_cnn.py:207-211, 256-257`): Conv1d(C, 1, kernel_size=1) -> Softmax over the
 * sequence -> weighted sum. x [B*L][C]; w [C] fp32 (the Conv1d weight [1][C][1] read in place, 16-byte
 * aligned); bias one fp32 value on the device (optional).
 *   s[b][l] = sum_c x[b*L + l][c] w[c] + bias,  a[b][.] = softmax_l(s[b][.]) (max-subtracted),
 *   y[b][c] = sum_l a[b][l] x[b*L + l][c].
 * y [B][C] in dtype; probs (optional, [B*L] fp32) receives a for the backward. One workgroup per sample,
 * the L scores in LDS: L <= FER_ATTNPOOL_MAX_L, larger L is rejected. fp32 arithmetic, no atomics, no
 * workspace; repeat calls are bit-identical. */
#define FER_ATTNPOOL_MAX_L 4096
int fer_attnpool_fwd(int dtype, const void* x, int64_t ldx, const float* w, const float* bias, void* y, int64_t ldy,
                     float* probs, int B, int L, int C, fer_stream_t stream);
/* Backward from the saved probs: da[b][l] = sum_c dy[b][c] x[b*L + l][c],
 * ds[b][l] = a[b][l] (da[b][l] - sum_l' a[b][l'] da[b][l']), dx[b*L + l][c] = a[b][l] dy[b][c] + ds[b][l] w[c];
 * the parameter gradients leave as per-sample partials, dw_part[b][c] = sum_l ds[b][l] x[b*L + l][c]
 * ([B][C] fp32, 16-byte aligned) and dbias_part[b] = sum_l ds[b][l] ([B] fp32), for the caller to sum over
 * b with fer_colsum (deterministic). dx, dw_part, dbias_part are each optional (at least one). */
int fer_attnpool_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* w,
                     const float* probs, void* dx, int64_t lddx, float* dw_part, float* dbias_part, int B, int L,
                     int C, fer_stream_t stream);

/* ReLU -> Dropout behind input_proj's LayerNorm (`latent_cnn.py:183-188`), element-wise over x [M][C]:
 * y = keep * drop_scale * max(x, 0); backward dx = dy * [x > 0] * keep * drop_scale with the gate and the
 * keep bits recomputed from x and the seed (element index r * C + c; nothing is stored). */
int fer_relu_dropout_fwd(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int M, int C,
                         uint32_t drop_thresh, float drop_scale, uint64_t seed, fer_stream_t stream);
int fer_relu_dropout_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, void* dx, int64_t lddx,
                         int M, int C, uint32_t drop_thresh, float drop_scale, uint64_t seed, fer_stream_t stream);

/* ---- LatentCNN2D (`latent_cnn.py:333-409`), csrc/conv2d.hip: the (18, 512) code as a one-channel image.
 * Activations are pixel-major [M = B*H*W][C] (NHWC) in dtype, the 2-D form of [B*L][C]: BatchNorm2d
 * (`:354,359,365`) is fer_batchnorm_fwd/_bwd with M = B*H*W, AdaptiveAvgPool2d(1) + Flatten (`:372,376`) is
 * fer_seq_mean_fwd/_bwd with L = H*W. Same 16-byte piece rules as the LatentCNN baseline: C a multiple of 8
 * (bf16) / 4 (fp32), row strides likewise, base pointers 16-byte aligned. No atomics, nothing stored for the
 * backward; repeat calls are bit-identical. */

/* im2col of nn.Conv2d(kernel_size=3, stride=1, padding=1) (`latent_cnn.py:358,364`):
 *   cols[(b*H + h)*W + w][cin*9 + kh*3 + kw] = x[(b*H + h+kh-1)*W + (w+kw-1)][cin] inside the image, else 0
 * (never the neighbouring row's or sample's pixel; values copied bit for bit). The (cin, kh, kw) column order
 * is the memory order of nn.Conv2d.weight [Cout][Cin][3][3]: the parameter is fer_gemm's B operand with
 * K = 9*Cin as it stands, and the weight gradient dy^T cols lands in the parameter's layout. x [M][C],
 * cols [M][9*C]. */
int fer_conv2d_cols(int dtype, const void* x, int64_t ldx, void* cols, int64_t ldc, int B, int H, int W, int C,
                    fer_stream_t stream);
/* Its adjoint: dx[m][c] = the sum over (kh, kw), in scan order, of dcols[m - (kh-1)*W - (kw-1)][c*9 + kh*3 + kw]
 * over the output pixels inside the image (fp32 sum, rounded once). */
int fer_conv2d_cols_bwd(int dtype, const void* dcols, int64_t ldd, void* dx, int64_t lddx, int B, int H, int W,
                        int C, fer_stream_t stream);

/* The first layer nn.Conv2d(1, Cout, kernel_size=3, padding=1) (`latent_cnn.py:353`), direct: x [M] scalars
 * at element stride ldx (the model input (B, H, W) as it lies), w [Cout][9] and bias [Cout] (optional) fp32,
 *   y[m][co] = bias[co] + sum_k x9[m][k] w[co][k],  x9[m][kh*3 + kw] = the pixel at (h+kh-1, w+kw-1) or 0,
 * k in order, fmaf in fp32. Precision on the bf16 path: x is read as bf16, the weights and the bias are the
 * fp32 parameters themselves (no bf16 shadow), the sum is fp32 and only y is rounded to bf16.
 * Cout <= FER_CONV2D_C1_MAX_COUT (the weights sit in LDS). */
#define FER_CONV2D_C1_MAX_COUT 1024
int fer_conv2d_c1_fwd(int dtype, const void* x, int64_t ldx, const float* w, const float* bias, void* y, int64_t ldy,
                      int B, int H, int W, int Cout, fer_stream_t stream);
/* Backward. dw_part (optional, [n_parts][Cout*9] fp32, 16-byte aligned): row g = sum over the pixels m of
 * strip g (ceil(M / n_parts) consecutive pixels) of dy[m][co] x9[m][k], in the parameter's layout; the caller
 * adds the rows with fer_colsum (Cout*9 is a multiple of 4) and takes dbias from fer_colsum of dy. A strip
 * without pixels is written as zeros. dx (optional, [M] scalars at stride lddx, needs w):
 * dx[m] = sum_k sum_co dy[m - (kh-1)*W - (kw-1)][co] w[co][k] over the pixels inside the image. x is needed for
 * dw_part only. Every sum is a fixed-order fp32 loop. */
int fer_conv2d_c1_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* w,
                      float* dw_part, int n_parts, void* dx, int64_t lddx, int B, int H, int W, int Cout,
                      fer_stream_t stream);

/* The stages behind BatchNorm2d + ReLU, nn.MaxPool2d((2, 2)) -> nn.Dropout2d (`latent_cnn.py:361-362,367-368`;
 * pool = 0: Dropout2d alone, `:356`) in one launch. x [B*H*W][C] -> y [B*Ho*Wo][C], Ho = H / 2, Wo = W / 2
 * (floor: a last odd row or column takes no part) with pool = 1, which needs H >= 2 and W >= 2; Ho = H, Wo = W
 * with pool = 0. Dropout2d drops whole (sample, channel) planes: keep = the library's hash at element index
 * b*C + c (u16 >= drop_thresh), y = keep ? max * drop_scale : exactly 0; drop_thresh = 0 (eval) passes the
 * values bit for bit. The maximum is the window's first in (kh, kw) scan order under a strict > (PyTorch's
 * tie rule). */
int fer_pool2_chdrop_fwd(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int B, int H, int W, int C,
                         int pool, uint32_t drop_thresh, float drop_scale, uint64_t seed, fer_stream_t stream);
/* dx [B*H*W][C] = dy * keep * drop_scale at each window's argmax pixel, recomputed from the forward's x by
 * the same rule, and exactly 0 elsewhere (the pixels floor division leaves out included). x is read with
 * pool = 1 only. */
int fer_pool2_chdrop_bwd(int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx, void* dx, int64_t lddx,
                         int B, int H, int W, int C, int pool, uint32_t drop_thresh, float drop_scale, uint64_t seed,
                         fer_stream_t stream);

/* ---- AFS style extractor (`afs/style_extractor.py`), csrc/grouped.hip: G structurally identical blocks, one
 * launch per stage over all of them. Every operand of group g is `base + g * group_stride` (gs*, in
 * elements) with its own row stride (ld*), so a [B][G][K] tensor is one operand with ld = G*K, gs = K.
 * Activations in dtype, biases and every gradient of a parameter fp32. fp32 accumulation in a fixed order,
 * no atomics, no workspace: repeat calls are bit-identical.
 *
 * Shapes the kernels take (anything else is rejected with a message): K a multiple of 32, N a multiple
 * of 16; x / w / y / dy / dx 16-byte aligned with row and group strides that are multiples of 8 elements and
 * rows at least as long as the operand is wide; dw 16-byte aligned, strides multiples of 4; G <= 65535.
 * Up to three weight sets share one launch (a highway layer's nonlinear / linear / gate linears read the
 * same input): sets are given from 0 upwards, a null w1 / w2 (dy1 / dy2) ends the list. M is any count >= 1;
 * rows beyond M are never read.
 *
 * forward: y_s[g] = x[g] w_s[g]^T + b_s[g], w in nn.Linear layout [N][K], x [M][K], y_s [M][N]; b_s optional.
 * bf16: v_mfma_f32_16x16x32_bf16; fp32: FMA. */
int fer_grouped_linear_fwd(int dtype, const void* x, int64_t ldx, int64_t gsx, const void* w0, const void* w1,
                           const void* w2, int64_t ldw, int64_t gsw, const float* b0, const float* b1,
                           const float* b2, int64_t gsb, void* y0, void* y1, void* y2, int64_t ldy, int64_t gsy,
                           int G, int M, int N, int K, fer_stream_t stream);
/* dgrad: dx[g] = sum_s dy_s[g] w_s[g]  (dy_s [M][N], dx [M][K]). */
int fer_grouped_linear_dgrad(int dtype, const void* dy0, const void* dy1, const void* dy2, int64_t lddy, int64_t gsdy,
                             const void* w0, const void* w1, const void* w2, int64_t ldw, int64_t gsw, void* dx,
                             int64_t lddx, int64_t gsdx, int G, int M, int N, int K, fer_stream_t stream);
/* wgrad: dw_s[g] (+)= dy_s[g]^T x[g] ([N][K] fp32), db_s[g] (+)= the column sums of dy_s[g] ([N] fp32), from
 * the same launch; each dw_s / db_s is optional (at least one). accumulate: add to what the outputs hold.
 * skip_mask: bit g set = group g's outputs are left untouched (a frozen block; G <= 64 when non-zero). */
int fer_grouped_linear_wgrad(int dtype, const void* dy0, const void* dy1, const void* dy2, int64_t lddy, int64_t gsdy,
                             const void* x, int64_t ldx, int64_t gsx, float* dw0, float* dw1, float* dw2,
                             int64_t lddw, int64_t gsdw, float* db0, float* db1, float* db2, int64_t gsdb,
                             int accumulate, uint64_t skip_mask, int G, int M, int N, int K, fer_stream_t stream);

/* Highway mix (`style_extractor.py:36-40`) over pre-activations pn, pl, pg [G][B][C] (ldp, gsp):
 *   y = s n + (1 - s) pl,  s = sigmoid(pg),  n = act(BatchNorm(pn)),  act = LeakyReLU(0.2) or ReLU,
 * BatchNorm1d per (group, channel) over the B rows. train: biased batch variance (two-pass) for the
 * normalisation; running_mean / running_var (fp32, gs_stat; optional) move by `momentum` towards the batch
 * mean / UNBIASED variance and num_batches_tracked[g * gs_nbt] (optional) is advanced; B >= 2. eval: the
 * running statistics. gamma / beta fp32 at group stride gs_par. mean / rstd (optional, [G][C] fp32)
 * receive the statistics used, for the backward. Any C >= 1, no alignment rule. */
enum { FER_HIGHWAY_LRELU = 0, FER_HIGHWAY_RELU = 1 };
int fer_highway_fwd(int dtype, const void* pn, const void* pl, const void* pg, int64_t ldp, int64_t gsp,
                    const float* gamma, const float* beta, int64_t gs_par, float* running_mean, float* running_var,
                    int64_t gs_stat, int64_t* num_batches_tracked, int64_t gs_nbt, int train, float momentum,
                    float eps, int act, void* y, int64_t ldy, int64_t gsy, float* mean, float* rstd, int G, int B,
                    int C, fer_stream_t stream);
/* Backward from dy and the forward's pn, pl, pg, mean, rstd: dpg = dy (n - pl) s (1 - s), dpl = dy (1 - s),
 * dpn = dy s act'(.) through the BatchNorm adjoint (train: batch statistics; eval: gamma rstd only).
 * dgamma / dbeta (fp32, group stride gs_par, optional) receive or accumulate; skip_mask as in wgrad. */
int fer_highway_bwd(int dtype, const void* dy, int64_t lddy, int64_t gsdy, const void* pn, const void* pl,
                    const void* pg, int64_t ldp, int64_t gsp, const float* mean, const float* rstd,
                    const float* gamma, const float* beta, int64_t gs_par, int train, int act, void* dpn, void* dpl,
                    void* dpg, int64_t lddp, int64_t gsdp, float* dgamma, float* dbeta, int accumulate,
                    uint64_t skip_mask, int G, int B, int C, fer_stream_t stream);

/* Softmax cross-entropy with label smoothing and optional class weights, mean reduction
 * normalised by sum w[y] (nn.CrossEntropyLoss, `train_image_vit.py:262-267`). Writes the
 * scalar loss and dlogits = grad_scale * dloss/dlogits. */
int fer_cross_entropy(const float* logits, const int64_t* labels, const float* weight, int B, int C,
                      float label_smoothing, float grad_scale, float* loss, float* dlogits, fer_stream_t stream);

/* w+ prologue (LatentViTv2 order SPE -> LWN -> LEAM, `latent_vit_v2.py:82-84`):
 * SemanticPE add (`semantic_pe.py:36-48`), LayerWiseNorm (+ residual gate,
 * `layer_wise_norm.py:35-50`), LEAM scale (`leam.py:31-40`). x,y fp32 [B][L][D]. */
int64_t fer_wplus_ws(int B, int L, int D);
int fer_wplus_fwd(const float* x, float* y, int B, int L, int D, const float* spe_group, const float* spe_layer,
                  const int64_t* groups, const float* lwn_w, const float* lwn_b, const float* lwn_gate,
                  const float* leam_w, float eps, float* saved, fer_stream_t stream);
int fer_wplus_bwd(const float* x, const float* saved, const float* dy, float* dx, int B, int L, int D,
                  const float* spe_group, const float* spe_layer, const int64_t* groups, const float* lwn_w,
                  const float* lwn_b, const float* lwn_gate, const float* leam_w, float eps, float* d_spe_group,
                  float* d_spe_layer, float* d_lwn_w, float* d_lwn_b, float* d_lwn_gate, float* d_leam_w,
                  int accumulate, float* ws, int64_t ws_bytes, fer_stream_t stream);

/* LatentDecomposer (`latent_decomposer.py:82-173`): dirs [C][L*D] (unit rows),
 * output_mode 0 expr_only, 1 id_only, 2 enhanced, 3 concat; decompose_mode 0 all_classes,
 * 1 max_class. y: [B][L or 2L][D] fp32. scores (optional) [B][C]. */
int fer_decompose(const float* w, const float* dirs, int B, int C, int LD, int output_mode, float alpha,
                  int decompose_mode, float* y, float* scores, fer_stream_t stream);

/* Elementwise helpers. */
int fer_cast_f32_bf16(const float* x, void* y, int64_t n, fer_stream_t stream);
int fer_cast_bf16_f32(const void* x, float* y, int64_t n, fer_stream_t stream);
/* y = x + s * t (s = *scale_ptr) over n elements, dtype; dot: out (+)= sum(a*b) fp32. */
int fer_axpy(int dtype, const void* x, const void* t, const float* scale_ptr, void* y, int64_t n,
             fer_stream_t stream);
int fer_dot(int dtype, const void* a, const void* b, int64_t n, float* out, int accumulate, float* ws,
            int64_t ws_bytes, fer_stream_t stream);
/* y = dropout(x) (p encoded by thresh); used for standalone dropout sites. */
int fer_dropout(int dtype, const void* x, void* y, int64_t n, uint32_t drop_thresh, float drop_scale, uint64_t seed,
                fer_stream_t stream);

/* Fused AdamW over a flat fp32 parameter buffer (torch.optim.AdamW semantics,
 * `train_image_vit.py:270-276`), segments with per-group lr / weight decay,
 * grad_scale multiplies the gradient (e.g. 1/world after an all-reduce sum, or a
 * clip factor read from clip_coef if non-NULL). Optionally refreshes the bf16 shadow copy. */
typedef struct {
  int64_t offset, numel;
  float lr, weight_decay, beta1, beta2, eps;
  int step;
} fer_adamw_segment;
int fer_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16,
              const fer_adamw_segment* segs_device, int nsegs, int64_t max_seg_numel, float grad_scale,
              const float* clip_coef, const uint64_t* step_add, fer_stream_t stream);

/* Transposed bf16 weight shadow (no reference counterpart: layout only). segs: device int64
 * [nseg][4] = {offset, rows, cols, first_tile} into the flat buffers, first_tile the running
 * count of 64x64 tiles (ceil(rows/64)*ceil(cols/64) per segment), total_tiles their sum:
 * dst[off + c*rows + r] = src[off + r*cols + c]. The dgrad GEMMs read W^T K-contiguous. */
int fer_transpose_bf16_segments(const void* src, void* dst, const int64_t* segs, int nseg, int64_t total_tiles,
                                fer_stream_t stream);

/* LatentAugment (`data/latent_dataset.py:6-49`) on a device batch x fp32 [B][LD], in place:
 * x += N(0, noise_std); x *= U(scale_lo, scale_hi) per sample; x *= (U(0,1) > mask_prob).
 * Counter-based draws keyed by seed (and the step counter below, when set). */
int fer_latent_augment(float* x, int64_t B, int LD, float noise_std, float scale_lo, float scale_hi,
                       float mask_prob, uint64_t seed, fer_stream_t stream);

/* Latents pushed along direction vectors (`sefa/verify_directions.py:57-58`, `data/augment_latents.py:56`:
 * w + step * direction), csrc/latent_dirs.hip. Everything fp32:
 *   out[r][l][:] = x[src(r)][l][:] + steps[c % S] * dirs[c / S][l or 0][:]
 * x [n][L][D] at sample stride ldx, out at sample stride ldo (both >= L*D, in floats), steps [S],
 * dirs [K][D] (dir_layers = 1: one vector broadcast over the layers, a SeFa direction) or [K][L][D]
 * (dir_layers = L: a w+ direction), contiguous. The product and the sum are rounded separately (no FMA):
 * bit-equal to torch's `x + step * d` on the CPU.
 *   choice == NULL (grid mode): out holds K*S*n rows, row r = (k*S + s)*n + i is sample i shifted by pair
 *     c = k*S + s. out must not overlap x.
 *   choice != NULL (choice mode): int32 [n], out holds n rows, src(r) = r, c = choice[r]; a value outside
 *     [0, K*S) copies the row bit for bit and reads neither dirs nor steps. out == x is allowed.
 * 16-byte loads and stores when D % 4 == 0, both strides are multiples of 4 and x, out and dirs are 16-byte
 * aligned; element by element otherwise, same bits. K < 1, S < 1, dir_layers outside {1, L}, a stride below
 * L*D or more than 2^31 - 1 output elements: a negative code, a message, nothing launched. n <= 0 is a no-op. */
int fer_latent_shift(const float* x, int64_t ldx, const float* dirs, int dir_layers, const float* steps,
                     const int32_t* choice, float* out, int64_t ldo, int64_t n, int K, int S, int L, int D,
                     fer_stream_t stream);
/* The per-sample draw for fer_latent_shift's choice mode: choice[i] = -1 (unchanged) when
 * u01(hash(seed', 2i)) <= p_keep, else floor(hash(seed', 2i + 1) * n_choices / 2^32), uniform over
 * [0, n_choices). seed' = the seed mixed with the step counter below (when set) xor a constant of this
 * entry point, so the stream differs from fer_latent_augment's under the same seed. p_keep = 1 / (1 + K*S) is
 * the share of originals in the reference's expanded directory (`data/augment_latents.py:47-71`). */
int fer_latent_dir_draw(int32_t* choice, int64_t n, int n_choices, float p_keep, uint64_t seed, fer_stream_t stream);
/* `sefa/verify_directions.py:48-69` on logits: base fp32 [n][C] (row stride ld_base), shifted fp32
 * [K*S*n][C] (row stride ld_shifted) in fer_latent_shift's grid order. One wave per (k, i): argmax by
 * fer_cls_stats' rule of the base row and of the S shifted rows, changed = any of them differs from the base.
 *   preds int64 [K][S][n]   the shifted rows' predictions (optional)
 *   changed uint8 [K][n]    0 / 1 (optional)
 *   counts int64 [K]        ACCUMULATED: samples of direction k whose label changed (required)
 *   step_counts int64 [K][S] ACCUMULATED: per step, samples whose prediction differs from the base (optional)
 * 64-bit integer atomic adds: any order, same bits. A caller chunks over directions or over samples by
 * offsetting the pointers. No host read: capturable. n <= 0 is a no-op. */
int fer_label_change(const float* base, int64_t ld_base, const float* shifted, int64_t ld_shifted, int K, int S,
                     int n, int C, int64_t* preds, uint8_t* changed, int64_t* counts, int64_t* step_counts,
                     fer_stream_t stream);

/* ImageViT input transforms (`data/image_dataset.py:139-173`, torchvision on PIL images) on the
 * device, SURVEY §8(f) row 4. Sources: B decoded uint8 HWC images (C = 1 or 3) packed in one
 * device buffer, image b at src + offsets[b], hwc[3b..3b+2] = H, W, C. Output fp32 NCHW
 * [B][3][S][S] normalised with mean3/std3 (host arrays).
 *   train = 0: Resize((S,S)) -> ToTensor -> Normalize (get_val_transforms)
 *   train = 1: Resize -> HorizontalFlip -> Rotation -> ColorJitter -> Affine -> ... (get_train_transforms)
 * with per-image parameter records params[B][16] (fer_image_aug_draw, or given by the caller):
 * [0] flip, [1] angle deg, [2..5] brightness/contrast/saturation/hue factors, [6..9] jitter op
 * order (0 b, 1 c, 2 s, 3 h), [10] tx, [11] ty (pixels), [12] scale, [13] hue enabled.
 * Every stage follows PIL's own arithmetic (fixed-point resampling and rotation, uint8 blends,
 * 8-bit HSV), so the output equals the reference pipeline's for the same parameters.
 * S <= 1024; any source size (shrinking widens the resize filter, as in PIL). */
typedef struct {
  float flip_p, degrees, brightness, contrast, saturation, hue, translate, scale_lo, scale_hi;
} fer_image_aug;
int fer_image_aug_draw(float* params, int B, int S, const fer_image_aug* aug, uint64_t seed, fer_stream_t stream);
int fer_image_augment(const uint8_t* src, const int64_t* offsets, const int32_t* hwc, int B, int S,
                      const float* params, int train, const float* mean3, const float* std3, float* out,
                      fer_stream_t stream);

/* Graph-replayed training steps (hipGraph capture of a whole step; no reference counterpart,
 * the reference trains eagerly). counter: caller-owned device uint64. After
 * fer_set_step_counter(counter) every dropout kernel mixes *counter into its seed, so a replayed
 * launch with a captured (constant) seed still draws a fresh mask each step; fer_adamw adds
 * *step_add to each segment's step. fer_step_advance(counter) (+1, a 1-thread kernel) is the
 * first node of the captured step. NULL disables (default). */
int fer_set_step_counter(const uint64_t* counter);
int fer_step_advance(uint64_t* counter, fer_stream_t stream);

/* ---- Mixup on the device (csrc/mixup.hip; `train/train_latent_vit_v2.py:118-130`), so that a captured step
 * draws a new lam and a new permutation on every replay.
 *
 * fer_mixup_draw: n_sets independent draws, one workgroup each. Set s draws from the seed mixed with the step
 * counter above (when set) and then with s; production uses n_sets = 1.
 *   lam[s]           fp32, Beta(alpha, alpha) for alpha > 0 (not folded to >= 0.5, as the reference), exactly 1
 *                    for alpha <= 0: g1 / (g1 + g2) of two Gamma(alpha) draws by Marsaglia-Tsang (below 1:
 *                    Gamma(alpha + 1) U^(1/alpha)), at most 16 attempts each (a draw that exhausts them, chance
 *                    < 1e-18, takes the proposal's central value)
 *   perm[s*B + i]    int32, the rank of (hash(perm seed, i), i) among the B pairs, ties on i: a permutation,
 *                    integers only, reproduced exactly on the host
 * 1 <= B <= 2048, n_sets >= 1 and both outputs given; anything else returns a negative code and a message.
 *
 * fer_mixup_apply: out[b][:] = lam * x[b][:] + (1 - lam) * x[perm[b]][:], fp32 rows of L elements, lam read
 * from device memory (one float). 16-byte loads and stores when L % 4 == 0 and x and out are 16-byte aligned,
 * element by element otherwise, same bits. A perm entry outside [0, B) takes the row itself. out must not
 * overlap x (the gather reads rows an in-place mix would have overwritten); B <= 65535. B <= 0 or L <= 0: no-op.
 *
 * fer_cross_entropy_mix: lam * CE(z, y) + (1 - lam) * CE(z, y[perm]) with fer_cross_entropy's semantics per
 * term (each divided by its own sum w[target]), loss and dlogits = grad_scale * dloss/dlogits in one launch,
 * one log-sum-exp per row. perm NULL: the identity; dlogits NULL: loss only; B <= 0: no-op. */
int fer_mixup_draw(float alpha, int B, uint64_t seed, int n_sets, float* lam, int32_t* perm, fer_stream_t stream);
int fer_mixup_apply(const float* x, const int32_t* perm, const float* lam, float* out, int B, int64_t L,
                    fer_stream_t stream);
int fer_cross_entropy_mix(const float* logits, const int64_t* labels, const int32_t* perm, const float* lam,
                          const float* weight, int B, int C, float label_smoothing, float grad_scale, float* loss,
                          float* dlogits, fer_stream_t stream);

/* sum of squares of grad (for clip_grad_norm_), out fp32 scalar; ws >= fer_colsum_ws(1, 4096). */
int fer_sumsq(const float* x, int64_t n, float* out, float* ws, int64_t ws_bytes, fer_stream_t stream);
/* clip coefficient: coef = min(1, max_norm / (sqrt(sumsq*sq_scale) + 1e-6)) (torch clip_grad_norm_). */
int fer_clip_coef(const float* sumsq, float sq_scale, float max_norm, float* coef, fer_stream_t stream);

/* ---- Low-latency inference (csrc/skinny.hip; fervit/infer.py InferenceSession). One launch, bf16, M <= 64 rows:
 *   out[M][N] = act(A' W^T + bias) + R'
 *   A' = A, or LN(A; gamma_a, beta_a, eps_a) when gamma_a is given (normalised on load, row width K)
 *   R' = nothing (res NULL), res, or LN(res; gamma_r, beta_r, eps_r) when gamma_r is given (row width N)
 *   act = FER_ACT_NONE_, FER_ACT_GELU_ (erf) or FER_ACT_RELU_
 * A [M][lda], W [N][ldw] (K-contiguous, nn.Linear's layout), res [M][ldr] and out [M][ldc] are bf16; bias,
 * gamma and beta are fp32. Accumulation is fp32; the LayerNorm statistics are fp32, taken from the stored bf16
 * values (biased variance); A' is rounded to bf16 as the matrix operand, LN(res) is added in fp32 without
 * being rounded to bf16 first. A post-norm encoder layer is five launches with both LayerNorms folded into
 * their consumers.
 * Contract: 1 <= M <= 64; K % 8 == 0 and N % 8 == 0; every ld covers its row and is a multiple of 8; every
 * base pointer is 16-byte aligned; gamma and beta come in pairs. Anything else returns a negative code and
 * sets fer_last_error before any launch. N / 16 workgroups that never communicate: the result is
 * deterministic, and row m of the output does not depend on M or on the other rows. out may alias nothing. */
int fer_skinny_linear(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, int act,
                      const float* gamma_a, const float* beta_a, float eps_a, const void* res, int64_t ldr,
                      const float* gamma_r, const float* beta_r, float eps_r, void* out, int64_t ldc, int M, int N,
                      int K, fer_stream_t stream);

/* The AdapterModule of the pre-norm models as one launch of the same plan (csrc/skinny_adapter.hip), bf16,
 * M <= 64 rows:
 *   out[M][D] = X + alpha * ( GELU_erf(X W1^T + b1) W2^T + b2 )
 * X [M][ldx], W1 [R][ldw1], W2 [D][ldw2] (nn.Linear's layout) and out [M][ldc] are bf16; b1 [R], b2 [D] and
 * alpha are fp32. alpha is a DEVICE pointer to one float (the module's parameter): the kernel reads it, the
 * host never does, so the launch is sync-free and a captured launch follows later changes of the value.
 * Accumulation is fp32; the hidden tile GELU(.) is rounded to bf16 once, as the second product's matrix
 * operand; x + alpha * (. + b2) is formed in fp32 and rounded once on the store.
 * Contract: 1 <= M <= 64; D % 16 == 0; R % 16 == 0 and 16 <= R <= 128; every ld covers its row and is a
 * multiple of 8; every base pointer is 16-byte aligned (alpha: 4-byte); out must not overlap X (every
 * workgroup reads the whole of X). Anything else returns a negative code and sets fer_last_error before any
 * launch. D / 16 workgroups that never communicate, each recomputing the hidden tile (DESIGN.md section
 * 2.13): the result is deterministic, and row m of the output does not depend on M or on the other rows. */
int fer_skinny_adapter(const void* X, int64_t ldx, const void* W1, int64_t ldw1, const float* b1, const void* W2,
                       int64_t ldw2, const float* b2, const float* alpha, void* out, int64_t ldc, int M, int D,
                       int R, fer_stream_t stream);

const char* fer_last_error(void);
const char* fer_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FERVIT_H */
